"""What ``helpers_bwd.edge_scene`` promises, asserted from the ORACLE's forward on any machine: every case of
tests/test_backward_edges_gpu.py renders these scenes, so the branches of csrc/backward.hip they are meant to reach are
known to be reached before a GPU is involved."""
import numpy as np
import pytest

from tests import helpers_bwd as hb

P = 3000


def _view_space(case):
    inp = case["inp"]
    pv = np.c_[inp["means3D"].astype(np.float64), np.ones(len(inp["means3D"]))] @ inp["viewmatrix"].reshape(4, 4)
    return pv[:, 0], pv[:, 1], pv[:, 2]


def test_the_camera_is_rotated_about_all_three_axes_and_off_the_origin():
    cam = hb.rotated_camera(48, 32)
    R = cam.world_view_transform.numpy()[:3, :3].astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6
    angle = np.degrees(np.arccos((np.trace(R) - 1.0) / 2.0))
    assert angle > 20.0, angle
    assert np.abs(R - np.eye(3))[~np.eye(3, dtype=bool)].min() > 0.1  # no axis left alone
    assert np.abs(R - R.T).max() > 0.3  # a transposed index changes the matrix
    assert np.linalg.norm(cam.camera_center.numpy()) > 1.0
    assert (cam.tanfovx, cam.tanfovy) == pytest.approx((hb.TANFOVX, hb.TANFOVY)) and cam.tanfovx > 1.5 * cam.tanfovy


@pytest.mark.parametrize("W,H", hb.IMAGE_SIZES)
@pytest.mark.parametrize("aa", [False, True])
def test_edge_scene_conditions(W, H, aa):
    case = hb.edge_case(P, W, H, aa=aa)
    vis, kind, g = case["visible"], case["kind"], case["fwd"]["geom"]
    # culled Gaussians: who, how many, and where they sit among the visible ones
    np.testing.assert_array_equal(~vis, hb.expect_culled(kind))
    assert (~vis).mean() >= 0.05
    assert not vis[256:512].any()
    assert vis[512:768].sum() == 1 and vis[600]
    for b in range((P + 255) // 256):
        if b in (1, 2):
            continue
        v = vis[256 * b:256 * (b + 1)]
        assert v.any() and not v.all() and (np.diff(v.astype(np.int8)) != 0).sum() >= 20, b  # interleaved, not two runs
    # the Jacobian's clamp branch, in x and in y
    tx, ty, tz = _view_space(case)
    assert (vis & (np.abs(tx / tz) > 1.3 * hb.TANFOVX)).sum() >= 20
    assert (vis & (np.abs(ty / tz) > 1.3 * hb.TANFOVY)).sum() >= 20
    # clamped colour channels: one, two and all three of a Gaussian's
    per_gaussian = g["clamped"][vis].astype(bool).sum(1)
    assert (per_gaussian > 0).sum() >= 10 and {1, 2, 3} <= set(per_gaussian.tolist())
    # alpha reaches the 0.99 cap: opacity above 0.99 with the centre on the screen
    m2d = g["means2D"]
    on_screen = (m2d[:, 0] >= 0) & (m2d[:, 0] <= W - 1) & (m2d[:, 1] >= 0) & (m2d[:, 1] <= H - 1)
    if not aa:  # (antialiasing scales the opacity by at most 1)
        assert (vis & on_screen & (g["conic_opacity"][:, 3] > 0.99)).sum() >= 10
    # pixels the compositor leaves before the end of their tile's list
    sat = hb.saturated_pixels(case)
    assert sat >= 10, sat
    # more than two staging rounds of 256 in render_backward_kernel
    assert case["fwd"]["n_contrib"].max() > 512
    # the gradients that come out are worth comparing: most visible Gaussians receive one
    assert (np.abs(case["ref"]["dL_dopacity"].reshape(-1)[vis]) > 0).mean() > 0.25


def test_edge_scene_deep_variant_takes_many_staging_rounds():
    case = hb.edge_case(P, 48, 32, deep=True)
    fwd = case["fwd"]
    np.testing.assert_array_equal(~case["visible"], hb.expect_culled(case["kind"]))
    deep = case["kind"] == hb.DEEP
    assert deep.sum() > 600 and case["visible"][deep].all()
    # the faint cluster in front of pixel (24, 8) is walked to its end, every member contributing, before the scene behind
    # it takes the pixel below T = 1e-4
    assert fwd["n_contrib"][4:12, 21:29].min() > 768 and fwd["n_contrib"].max() > 1024
    assert (np.abs(case["ref"]["dL_dopacity"].reshape(-1)[deep]) > 0).all()


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 515, 1022, 2049])
def test_edge_scene_tails(n):
    """The sizes of the P-tail cases: a visible Gaussian in each of them, culled ones where there is room, and the last
    workgroup all culled (257, 515) as well as mixed (255, 1022) and a single visible Gaussian (2049)."""
    case = hb.edge_case(n, 48, 32)
    vis = case["visible"]
    np.testing.assert_array_equal(~vis, hb.expect_culled(case["kind"]))
    assert vis[0] and (n < 2 or not vis[1])
    last = vis[(n - 1) // 256 * 256:]
    if n in (257, 515):
        assert not last.any()
    elif n == 2049:
        assert last.tolist() == [True]
    else:
        assert last.any()
    assert np.abs(case["ref"]["dL_dsh"]).max() > 0
