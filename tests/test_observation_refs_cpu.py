"""The binary64 references of tests/ref_observations.py without a GPU: known answers, and agreement with the float32
restatements (tests/test_maps_cpu.py restate_maps, tests/test_pointcloud_cpu.py restate_pointcloud) off the borderline
pixels and points, on oracle-rendered synthetic inputs at sizes whose tile grids and pixel counts are odd."""
import math

import numpy as np
import pytest

from gsworld_amd import scenes
from gsworld_amd.camera import look_at_view
from gsworld_amd.pointcloud import PointCloudSpec, sim_from_scene
from tests import helpers as hp
from tests import ref_observations as ro
from tests.test_maps_cpu import restate_maps
from tests.test_pointcloud_cpu import fps, restate_pointcloud, unproject

F32 = np.float32


def _frame(W, H, recs, lists):
    """A hand-made oracle frame: ``recs`` (x, y, depth, A, B, C, opacity) per Gaussian, ``lists`` {tile: [indices]}."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = np.asarray(recs, F32)
    geom = dict(means2D=r[:, 0:2].copy(), depths=r[:, 2].copy(), conic_opacity=r[:, 3:7].copy())
    ranges = np.zeros((gx * gy, 2), np.uint32)
    pl = []
    for t in range(gx * gy):
        ranges[t] = (len(pl), len(pl) + len(lists.get(t, [])))
        pl += lists.get(t, [])
    return geom, dict(ranges=ranges, point_list=np.asarray(pl, np.uint32))


def test_opaque_splat_across_a_tile_border_on_an_odd_grid():
    # 48 x 20: 3 x 2 tiles (odd gx, partial last tile row).  A wide opaque splat centred on the border of tiles 0 and 1,
    # listed in both; tile 2 and the second row list nothing.
    geom, binning = _frame(48, 20, [(16.0, 8.0, 2.5, 1e-6, 0.0, 1e-6, 0.99)], {0: [0], 1: [0]})
    lab, dep, bd = ro.maps_f64(geom, binning, 48, 20, labels=np.array([7.0], F32), depth_scale=2.0)
    assert lab.shape == (20, 48) and not bd.any()
    assert (lab[:16, :32] == 7).all() and (dep[:16, :32] == 5.0).all()
    assert (lab[:, 32:] == -1).all() and (lab[16:] == -1).all() and (dep[16:] == 0.0).all()


def test_two_splats_cross_one_half_at_the_second():
    # 0.3 then 0.3: T = 0.7, then 0.49 < 0.5 -- the second one is the median
    geom, binning = _frame(16, 16, [(8.0, 8.0, 1.0, 1e-9, 0.0, 1e-9, 0.3), (8.0, 8.0, 2.0, 1e-9, 0.0, 1e-9, 0.3)], {0: [0, 1]})
    lab, dep, bd = ro.maps_f64(geom, binning, 16, 16, labels=np.array([1.0, 2.0], F32), depth_scale=0.5)
    assert (lab == 2).all() and (dep == 1.0).all() and not bd.any()


def test_background_pixel_and_borderline_bands():
    geom, binning = _frame(16, 16, [(8.0, 8.0, 1.0, 1e-9, 0.0, 1e-9, 0.3)], {0: [0]})
    lab, dep, bd = ro.maps_f64(geom, binning, 16, 16, labels=np.array([1.0], F32))
    assert (lab == -1).all() and (dep == 0.0).all() and not bd.any()
    # T = 0.5 (1 + 5e-5) after the only contributor: inside the T band, background in binary64 but borderline
    geom, binning = _frame(16, 16, [(8.0, 8.0, 1.0, 0.0, 0.0, 0.0, 0.5 - 2.5e-5)], {0: [0]})
    lab, _, bd = ro.maps_f64(geom, binning, 16, 16, labels=np.array([1.0], F32))
    assert (lab == -1).all() and bd.all()
    # an alpha at 1/255 (1 + 1e-6) in front of the median: borderline; at 1/255 (1 + 1e-3): not
    for a, want in ((1.0 / 255.0 * (1 + 1e-6), True), (1.0 / 255.0 * (1 + 1e-3), False)):
        geom, binning = _frame(16, 16, [(8.0, 8.0, 1.0, 0.0, 0.0, 0.0, a), (8.0, 8.0, 2.0, 0.0, 0.0, 0.0, 0.9)], {0: [0, 1]})
        lab, _, bd = ro.maps_f64(geom, binning, 16, 16, labels=np.array([1.0, 2.0], F32))
        assert (lab == 2).all() and bool(bd.all()) == want


def test_optical_axis_pixel_unprojects_onto_the_axis():
    D = np.zeros((5, 7), F32)
    D[2, 3] = 3.0
    q, ok = ro.unproject_f64(D, np.eye(4, dtype=F32).reshape(-1), 0.7, 0.4)
    assert ok.sum() == 1 and q[2 * 7 + 3].tolist() == [0.0, 0.0, 3.0]
    # a rotated, translated camera: the axis pixel lies at centre + z (camera z axis in the world)
    cam = look_at_view([0.4, -0.3, 0.9], [0.0, 0.1, 0.0], [0, 0, 1], 1.1, 0.6, 7, 5)
    W2C = cam.world_view_transform.double().numpy().T
    q, _ = ro.unproject_f64(D, cam.world_view_transform.numpy().reshape(-1), cam.tanfovx, cam.tanfovy, depth_scale=1.5)
    C2W = np.linalg.inv(W2C)
    want = C2W[:3, 3] + 2.0 * C2W[:3, 2]
    assert np.abs(q[2 * 7 + 3] - want).max() < 1e-12


def test_fps_check_on_a_known_answer():
    P = np.zeros((6, 3))
    P[:, 0] = [0.0, 0.3, 0.45, 1.0, 0.6, 0.8]
    # from 0 the farthest is 1.0; then 0.45, whose distance^2 to {0, 1.0} is 0.2025, the largest
    ro.fps_check(P, [0, 3, 2])
    with pytest.raises(AssertionError):
        ro.fps_check(P, [0, 5])  # (0.8 is not the farthest from 0)
    with pytest.raises(AssertionError):
        ro.fps_check(P, [1, 3])  # (pick 0 must be candidate 0)
    with pytest.raises(AssertionError):
        ro.fps_check(P, [0, -1])  # (a pick that is no candidate)
    assert ro.fps_check(P, fps(P.astype(F32), 6)) == pytest.approx(1.0)


def test_stride_ranks_in_exact_integers():
    assert ro.stride_ranks(5, 5).tolist() == [0, 1, 2, 3, 4]
    assert ro.stride_ranks(10, 4).tolist() == [0, 2, 5, 7]
    assert ro.stride_ranks(16_000_000, 8192)[-1] == (8191 * 16_000_000) // 8192
    assert ro.stride_ranks(0, 0).size == 0


# ---- agreement with the float32 restatements ---------------------------------------------------------------------------
def _oracle_frame(W, H, n, seed, fov=(60.0, 60.0)):
    raw = scenes.random_scene_camera_frame(n, seed=seed)
    from gsworld_amd.camera import view_params

    cam = view_params(np.eye(3), np.zeros(3), math.radians(fov[0]), math.radians(fov[1]), W, H)
    inp = hp.np_inputs(raw, cam)
    st = hp.oracle_settings(cam)
    return hp.oracle_forward(inp, st, np.zeros(3, F32)), cam


def _splat_records(geom):
    """The oracle's geometry in the GPU's splat record layout (what restate_maps reads)."""
    P = geom["depths"].shape[0]
    splat = np.zeros((P, 12), F32)
    splat[:, 0:2] = geom["means2D"]
    splat[:, 2] = geom["depths"]
    with np.errstate(divide="ignore"):
        splat[:, 3] = F32(1.0) / geom["depths"]
    splat[:, 4:8] = geom["conic_opacity"]
    return splat


@pytest.mark.parametrize("W,H,fov", [(33, 17, (60.0, 60.0)), (70, 50, (50.0, 70.0)), (9, 5, (40.0, 40.0))])
def test_maps_f64_agrees_with_the_restatement(W, H, fov):
    o, _ = _oracle_frame(W, H, 4000, seed=W, fov=fov)
    P = o["geom"]["depths"].shape[0]
    labels = (np.arange(P) % 997).astype(F32)
    L64, D64, B64 = ro.maps_f64(o["geom"], o["binning"], W, H, labels, 1.75)
    L32, D32, B32 = restate_maps(_splat_records(o["geom"]), o["binning"]["point_list"], o["binning"]["ranges"], W, H,
                                 labels, 1.75)
    off = ~(B64 | B32)
    assert (L64 == L32)[off].all()
    fg = off & (L64 >= 0)
    assert fg.sum() > 0.2 * W * H, "the frame is (nearly) empty: the comparison shows nothing"
    rel = np.abs(D32[fg].astype(np.float64) / D64[fg] - 1.0)
    assert rel.max() <= 5e-7
    assert ((D64 == 0.0) == (L64 == -1)).all()
    assert B64.sum() <= 5e-3 * W * H


def _cloud_views(seed, sizes=((33, 17), (9, 5))):
    rng = np.random.default_rng(seed)
    views = []
    for k, (W, H) in enumerate(sizes):
        cam = look_at_view([0.5 - 0.3 * k, 0.4, 0.6], [0.0, 0.05 * k, 0.0], [0, 0, 1], 1.2, 0.5 + 0.2 * k, W, H)
        D = (0.3 + 1.2 * rng.random((H, W))).astype(F32)
        D[rng.random((H, W)) < 0.15] = 0.0
        views.append(dict(depth=D, label=rng.integers(-1, 9, (H, W)).astype(np.int16), rgb=None,
                          viewmatrix=cam.world_view_transform.numpy().reshape(-1), tanfovx=F32(cam.tanfovx),
                          tanfovy=F32(cam.tanfovy)))
    return views


def _rigid():
    th = 0.4
    M = np.eye(4)
    M[:3, :3] = [[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]]
    M[:3, 3] = [0.2, -0.1, 0.05]
    return M


@pytest.mark.parametrize("spec", [
    PointCloudSpec(out_from_scene=sim_from_scene(_rigid(), 1.3), crop=((-2.0, -2.0, -0.3), (2.0, 2.0, 2.0)),
                   exclude_labels=(-1, 3)),
    PointCloudSpec(num_points=100, sample="stride", exclude_labels=(5,)),
    PointCloudSpec(num_points=40, sample="fps", fps_candidates=300, out_from_scene=sim_from_scene(_rigid(), 0.8))])
def test_cloud_f64_agrees_with_the_restatement(spec):
    views = _cloud_views(7)
    ds = 1.5
    mode = "dense" if spec.num_points is None else spec.sample
    A = np.asarray(spec.affine(), F32)
    xyzw, _, seg, count, sel = restate_pointcloud(views, mode, K=spec.num_points or 0, fps_candidates=spec.fps_candidates,
                                                  A=A, crop=spec.crop, exclude=spec.exclude_labels, depth_scale=ds)
    ref = ro.cloud_f64(views, spec, depth_scale=ds)
    q32 = np.concatenate([unproject(v["depth"], v["viewmatrix"], v["tanfovx"], v["tanfovy"], ds, A)[0] for v in views])
    tol = ro.CROP_TOL * (1.0 + np.abs(ref["q"]))
    pts = ref["valid"]
    assert np.all(np.abs(q32[pts] - ref["q"][pts]) <= tol[pts])
    assert not ref["border"].any(), "a point on a crop face: pick another seed"
    assert count == (ref["n"] if mode == "dense" else min(ref["sel"].size, spec.num_points))
    if mode == "dense":
        assert np.array_equal(xyzw[:, 3] == 1.0, ref["valid"])
    elif mode == "stride":
        assert np.array_equal(sel, ref["sel"])
    else:
        cand = q32[ref["sel"]].astype(np.float64)
        pos = {int(p): i for i, p in enumerate(ref["sel"])}
        ro.fps_check(cand, [pos.get(int(p), -1) for p in sel])
