"""Segmentation / depth maps (csrc/maps.hip) at the shapes where the kernel's edge branches fire: odd tile grids (the
super-tile row stride), partial tiles, frames past the super-tile limit, launches over frames of several sizes and modes
(grid sized by the largest, more than 8 frames cut into launches, an overflowed frame among good ones), a permuted model,
and a closed loop of 10 lanes.  The maps are held to the binary64 walk over the oracle's lists (tests/ref_observations.py
maps_f64), to the float32 restatement (tests/test_maps_cpu.py restate_maps) and to single-frame calls, bit for bit."""
import numpy as np
import pytest
import torch

from gsworld_amd import _C, _lib
from gsworld_amd import closed_loop as cl
from gsworld_amd import scenes
from gsworld_amd.pointcloud import PointCloudSpec
from gsworld_amd.renderer import FrameRenderer
from tests import helpers as hp
from tests import ref_observations as ro
from tests.test_maps_gpu import MAPS, _against_restatement, _loop_setup, _render, _wrist

pytestmark = pytest.mark.gpu

N_GAUSS = 20_000
DS = 1.75
SIZES = [(9, 5), (16, 16), (33, 17), (70, 50), (48, 200), (200, 48), (640, 480)]
_cache = {}


def _scene(dev):
    if "scene" not in _cache:
        raw = scenes.random_scene_camera_frame(N_GAUSS, seed=3, near_fraction=0.0)
        means, shs, op, sc, rot = raw.to(dev).activated()
        labels = (torch.arange(N_GAUSS, device=dev) % 997).to(torch.float32)
        _cache["scene"] = (raw, dict(means3D=means, opacities=op, shs=shs, scales=sc, rotations=rot), labels)
    return _cache["scene"]


def _camera(W, H):
    # (a 90-degree field on both axes: the scene, |x|, |y| <= 1 at z >= 1.5, leaves background round it; pixels are not square
    #  where W != H)
    return scenes.identity_camera(W, H, 90.0)


def _oracle_maps(raw, cam, labels):
    key = ("f64", cam.image_width, cam.image_height)
    if key not in _cache:
        o = hp.oracle_forward(hp.np_inputs(raw, cam), hp.oracle_settings(cam), np.zeros(3, np.float32))
        _cache[key] = ro.maps_f64(o["geom"], o["binning"], cam.image_width, cam.image_height, labels.cpu().numpy(), DS)
    return _cache[key]


def _frame(dev, cam, m, forward_only):
    r = FrameRenderer(dev, forward_only=forward_only)
    _render(r, cam, m, times=1 if not forward_only else 2, exact=not forward_only)
    return r


def _super(r):
    st, P, permuted, cap = r._map_meta
    return bool(_lib.plan_query(st.image_width, st.image_height, P, permuted=permuted, forward_only=bool(st.forward_only),
                                r_capacity=cap if cap > 0 else 0)["super"])


def _against_f64(lab, dep, ref, what):
    torch.cuda.synchronize()
    L, D, B = ref
    H, W = L.shape
    gl, gd = lab.reshape(H, W).cpu().numpy(), dep.reshape(H, W).cpu().numpy().astype(np.float64)
    assert not ((gl != L) & ~B).any(), f"{what}: {int(((gl != L) & ~B).sum())} labels differ from binary64 off borderline"
    fg = ~B & (L >= 0)
    err = float(np.max(np.abs(gd[fg] / D[fg] - 1.0))) if fg.any() else 0.0
    assert err <= 5e-7, f"{what}: depth {err:.2e} from binary64"
    assert ((gd == 0.0) == (gl == -1))[~B].all()
    assert B.sum() <= 5e-3 * W * H, f"{what}: {int(B.sum())} borderline pixels"
    print(f"{what}: borderline {int(B.sum())} of {W * H}, depth rel err {err:.2e}, covered {float((L >= 0).mean()):.3f}")
    return err


@pytest.mark.parametrize("mode", ["exact", "forward_only"])
@pytest.mark.parametrize("W,H", SIZES)
def test_sizes_and_frame_modes(cuda_device, W, H, mode):
    dev = cuda_device
    raw, m, labels = _scene(dev)
    cam = _camera(W, H)
    r = _frame(dev, cam, m, mode == "forward_only")
    lab, dep = r.render_maps(labels, DS)
    ref = _oracle_maps(raw, cam, labels)
    assert 0.0 < float((ref[0] >= 0).mean()) < 1.0, "the frame shows no background or no scene: half the branches go untested"
    _against_f64(lab, dep, ref, f"{W}x{H} {mode}")
    _against_restatement(r, labels, DS, lab, dep, f"{W}x{H} {mode}")
    assert _super(r) == (mode == "forward_only"), "every one of these sizes takes super-tile lists in a forward_only frame"


def test_super_tile_plans_with_odd_tile_columns():
    odd = [(W, H) for W, H in SIZES if _lib.plan_query(W, H, N_GAUSS, forward_only=True)["super"] and ((W + 15) // 16) % 2]
    assert len(odd) >= 2, odd
    for W, H in SIZES:
        assert not _lib.plan_query(W, H, N_GAUSS, forward_only=False, r_capacity=0)["super"]


@pytest.mark.parametrize("W,H", [(1280, 720), (1920, 1080)])
def test_past_the_super_tile_limit(cuda_device, W, H):
    dev = cuda_device
    raw, m, labels = _scene(dev)
    cam = _camera(W, H)
    fo = _frame(dev, cam, m, True)
    assert fo.r_capacity > 0 and fo._map_meta[3] > 0, "not a capacity (inference) frame"
    assert not _super(fo), "a frame past the super-tile limit keeps per-tile lists"
    lab, dep = fo.render_maps(labels, DS)
    ex = _frame(dev, cam, m, False)
    want_l, want_d = ex.render_maps(labels, DS)
    torch.cuda.synchronize()
    assert torch.equal(lab, want_l) and torch.equal(dep, want_d), "inference frame maps differ from the exact frame's"
    _against_f64(lab, dep, _oracle_maps(raw, cam, labels), f"{W}x{H} forward_only (per-tile lists)")


def _mixed_frames(dev, m):
    """13 frames: several sizes (the largest third), exact and forward_only mixed, one overflowed frame in the middle."""
    plan = [((33, 17), False), ((70, 50), True), ((640, 480), True), ((9, 5), False), ((200, 48), True), ((16, 16), True),
            ((320, 240), False), ("overflow", True), ((48, 200), False), ((33, 17), True), ((70, 50), False), ((200, 48), False),
            ((9, 5), True)]
    rs = []
    for size, fo in plan:
        if size == "overflow":
            cam = _camera(640, 480)
            r = _frame(dev, cam, m, True)
            r.r_capacity = 4096
            r.render(cam, m["means3D"], m["opacities"], shs=m["shs"], scales=m["scales"], rotations=m["rotations"])
            assert r.stats().overflow
        else:
            r = _frame(dev, _camera(size[0], size[1]), m, fo)
        rs.append(r)
    return rs, plan.index(("overflow", True))


def test_one_large_mixed_call(cuda_device):
    dev = cuda_device
    _, m, labels = _scene(dev)
    rs, bad = _mixed_frames(dev, m)
    singles = [r.render_maps(labels, DS) for r in rs]
    torch.cuda.synchronize()
    assert bool((singles[bad][0] == -1).all()) and bool((singles[bad][1] == 0.0).all())
    sizes = [r._map_meta[0].image_width * r._map_meta[0].image_height for r in rs]
    assert int(np.argmax(sizes)) != 0 and len(rs) > 8
    assert _C._ext is not None and hasattr(_C._ext, "render_maps"), "the compiled binding is part of the build"
    for binding in ("ctypes", "ext"):
        # every output a slice of one buffer, with guard words between them: nothing but the frames' pixels may change
        pad = 64
        total = sum(sizes) + pad * (len(rs) + 1)
        lab_buf = torch.full((total,), 12345, dtype=torch.int16, device=dev)
        dep_buf = torch.full((total,), -7.5, dtype=torch.float32, device=dev)
        frames, outs, off = [], [], pad
        for r, n in zip(rs, sizes):
            lab, dep = lab_buf[off:off + n], dep_buf[off:off + n]
            f, _, _ = r._map_frame(labels, DS, lab, dep)
            frames.append(f)
            outs.append((lab, dep))
            off += n + pad
        _C.render_maps(frames, dev, binding=binding)
        torch.cuda.synchronize()
        guard = torch.ones(total, dtype=torch.bool, device=dev)
        for k, ((lab, dep), (l1, d1)) in enumerate(zip(outs, singles)):
            assert torch.equal(lab, l1.reshape(-1)) and torch.equal(dep, d1.reshape(-1)), f"{binding}: frame {k}"
        off = pad
        for n in sizes:
            guard[off:off + n] = False
            off += n + pad
        assert bool((lab_buf[guard] == 12345).all()) and bool((dep_buf[guard] == -7.5).all()), f"{binding}: wrote outside"


def test_permuted_model_on_an_odd_grid(cuda_device):
    from gsworld_amd.layout import SceneLayout

    dev = cuda_device
    raw, m, labels = _scene(dev)
    cam = _camera(200, 48)  # (13 x 3 tiles)
    L = SceneLayout.build(m["means3D"], m["scales"], m["rotations"], labels=labels, opacities=m["opacities"], shs=m["shs"])
    assert L.orig_index is not None
    a = L.arrays
    pm = dict(means3D=a["means3D"], opacities=a["opacities"], shs=a["shs"], scales=a["scales"], rotations=a["rotations"])
    pr = FrameRenderer(dev, forward_only=True)
    _render(pr, cam, pm, times=2, layout=L.layout)
    assert pr._map_meta[2] and _super(pr)
    lab, dep = pr.render_maps(a["labels"], DS)
    ex = _frame(dev, cam, m, False)
    want_l, want_d = ex.render_maps(labels, DS)
    torch.cuda.synchronize()
    assert torch.equal(lab, want_l) and torch.equal(dep, want_d)
    _against_f64(lab, dep, _oracle_maps(raw, cam, labels), "200x48 permuted")


@pytest.mark.parametrize("graph", [False, True])
def test_closed_loop_past_eight_lanes(cuda_device, graph):
    dev = cuda_device
    raw, rollout, parts, actors, cams = _loop_setup(150_000)
    E, steps = 5, 3
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=4, num_envs=E))
    spec = PointCloudSpec(num_points=512, sample="fps", fps_candidates=2048)
    loop = cl.ClosedLoopRenderer(raw, parts, cams, scaled_parts=actors, num_envs=E, device=dev, maps=MAPS, depth_scale=2.5,
                                 pointcloud=spec)
    loop.reset(*poses[0])
    if graph:
        loop.capture()
        assert loop.captured
    names = list(cams)
    assert len(loop.multi.lanes) == E * len(names) == 10
    for k in range(1, steps + 1):
        loop.step(*poses[k], cameras={"wrist_cam": _wrist(k, steps)}, ensure=True)
        torch.cuda.synchronize()
        got = {n: {kind: loop.maps[n][kind].clone() for kind in MAPS} for n in names}
        for e in range(E):
            for c, n in enumerate(names):
                lane = loop.multi.lanes[e * len(names) + c]
                l1, d1 = lane.render_maps(loop._map_labels, 2.5)
                torch.cuda.synchronize()
                assert torch.equal(got[n]["segmentation"][e].reshape(l1.shape), l1), f"step {k} env {e} {n}: labels"
                assert torch.equal(got[n]["depth"][e].reshape(d1.shape), d1), f"step {k} env {e} {n}: depth"
        assert int(loop.pointcloud["count"].min()) > 0
    lane = loop.multi.lanes[9]  # (environment 4's wrist camera: the second launch of the maps call)
    _against_restatement(lane, loop._map_labels, 2.5, loop.maps["wrist_cam"]["segmentation"][4],
                         loop.maps["wrist_cam"]["depth"][4], f"closed loop lane 9 graph={graph}")
