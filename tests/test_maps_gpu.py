"""Segmentation / depth maps of rendered frames (include/gsr.h gsr_render_maps, csrc/maps.hip) on the GPU: the kernel
against the NumPy restatement of the definition (tests/test_maps_cpu.py restate_maps), against the colour compositor's own
final transmittance, bit for bit across every way a frame can be rendered, and inside the closed loop."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from gsworld_amd import _C, _lib
from gsworld_amd import closed_loop as cl
from gsworld_amd import debug as dbg
from gsworld_amd import scenes
from gsworld_amd.camera import look_at_view
from gsworld_amd.renderer import FrameRenderer, MultiCameraRenderer
from tests.test_maps_cpu import restate_maps

pytestmark = pytest.mark.gpu

MAPS = ("segmentation", "depth")


def _model(raw, dev):
    means, shs, op, sc, rot = raw.to(dev).activated()
    P = means.shape[0]
    if raw.semantics is not None:
        labels = raw.semantics.reshape(-1).to(dev, torch.float32).contiguous()
    else:
        labels = (torch.arange(P, device=dev) % 997).to(torch.float32)
    return dict(means3D=means, opacities=op, shs=shs, scales=sc, rotations=rot), labels


def _render(r, cam, m, times=1, exact=False, **kw):
    for _ in range(times):
        r.render(cam, m["means3D"], m["opacities"], shs=m["shs"], scales=m["scales"], rotations=m["rotations"],
                 exact=exact, **kw)
    r.ensure_valid(lambda: r.render(cam, m["means3D"], m["opacities"], shs=m["shs"], scales=m["scales"],
                                    rotations=m["rotations"], **kw))


def _state(r):
    """(splat (P,12), point list, lists' ranges, super-tile lists?) of a renderer's last frame, from its state."""
    st, P, permuted, cap = r._map_meta
    W, H = st.image_width, st.image_height
    plan = _lib.plan_query(W, H, P, permuted=permuted, forward_only=bool(st.forward_only), r_capacity=cap if cap > 0 else 0)
    sup = bool(plan["super"])
    v = _lib.GsrStateView()
    _lib.check(_lib.lib().gsr_state_view(P, W, H, C.c_int64(max(cap, 1)), C.c_void_p(r.geom.data_ptr()),
                                         C.c_void_p(r.binning.data_ptr()), C.c_void_p(r.image.data_ptr()), C.byref(v)))
    gx, gy = (W + 15) // 16, (H + 15) // 16
    n_lists = gy * ((gx + 1) // 2) if sup else gx * gy
    splat = dbg._view(r.geom, v.splat, 12 * P, torch.float32).view(P, 12).cpu().numpy()
    ranges = dbg._view(r.image, v.ranges, 2 * n_lists, torch.int32).view(n_lists, 2).cpu().numpy()
    R = int(ranges[:, 1].max())
    pl = dbg._view(r.binning, v.point_list, R, torch.int32).cpu().numpy()
    return splat, pl, ranges, sup


def _against_restatement(r, labels, depth_scale, lab, dep, what):
    torch.cuda.synchronize()
    st = r._map_meta[0]
    W, H = st.image_width, st.image_height
    splat, pl, ranges, sup = _state(r)
    L, D, B = restate_maps(splat, pl, ranges, W, H, labels.cpu().numpy(), depth_scale, super_tiles=sup)
    gl, gd = lab.reshape(H, W).cpu().numpy(), dep.reshape(H, W).cpu().numpy()
    bad = ((gl != L) | (gd.view(np.uint32) != D.view(np.uint32))) & ~B
    print(f"{what}: {int(B.sum())} borderline pixels of {W * H}, {float((L >= 0).mean()):.3f} covered")
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ from the restatement off the borderline ones"
    # (the T band of the definition, 1e-4 of 0.5, dominates the count: pixels whose crossing contributor has a small alpha land
    #  in it often -- 1082 of 307 200 pixels, 0.35 %, at configs[1])
    assert B.sum() <= 5e-3 * W * H
    assert (L >= 0).mean() > 0.05, "the frame is (nearly) empty: the comparison shows nothing"
    return L, B


@pytest.mark.parametrize("config", ["configs0", "configs1"])
def test_maps_match_the_restatement(cuda_device, config):
    dev = cuda_device
    if config == "configs0":
        raw, cam = scenes.random_scene_camera_frame(100_000, seed=0), scenes.identity_camera(256, 256, 60.0)
    else:
        raw, cam = scenes.tabletop_scene("xarm6_align"), scenes.sensor_camera("xarm6_align")
    m, labels = _model(raw, dev)
    r = FrameRenderer(dev)
    _render(r, cam, m, exact=True)
    lab, dep = r.render_maps(labels, depth_scale=1.75)
    _against_restatement(r, labels, 1.75, lab, dep, config)


@pytest.mark.parametrize("library", ["default", "expacc"])
def test_background_exactly_where_the_compositor_leaves_half_the_light(cuda_device, library, monkeypatch):
    dev = cuda_device
    if library == "expacc":
        path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgsr_hip_expacc.so")
        if not os.path.exists(path):
            pytest.skip("libgsr_hip_expacc.so not built (make -C gsworld_amd/csrc)")
        monkeypatch.setattr(_C, "_ext", None)  # (the compiled binding is linked against the shipped library)
        monkeypatch.setattr(_lib, "_lib", None)
        monkeypatch.setattr(_lib, "LIB_PATH", path)
    raw, cam = scenes.tabletop_scene("xarm6_align"), scenes.sensor_camera("xarm6_align")
    m, labels = _model(raw, dev)
    r = FrameRenderer(dev)  # (a non-forward_only frame: the compositor writes final_T)
    _render(r, cam, m, exact=True)
    lab, dep = r.render_maps(labels)
    _, B = _against_restatement(r, labels, 1.0, lab, dep, library)
    R = int(r.stats().num_rendered)
    final_T = dbg.state_view(r._P, cam.image_width, cam.image_height, R, 0, r.geom, r.binning, r.image)["final_T"]
    bg = (final_T >= 0.5).cpu().numpy()
    gl = lab.cpu().numpy()
    assert ((gl == -1) == bg)[~B].all(), "label -1 and final_T >= 0.5 disagree off the borderline pixels"
    assert ((dep.cpu().numpy() == 0.0) == (gl == -1)).all()


def _tabletop(dev, n=300_000):
    raw = scenes.tabletop_scene("xarm6_align", n=n, seed=2)
    return raw, _model(raw, dev)


def test_same_maps_in_every_frame_mode(cuda_device):
    dev = cuda_device
    raw, (m, labels) = _tabletop(dev)
    cam = scenes.sensor_camera("xarm6_align")
    # exact frame (per-tile lists, depth in the records) against a forward_only capacity frame (super-tile lists, tau there)
    ex = FrameRenderer(dev)
    _render(ex, cam, m, exact=True)
    want_l, want_d = ex.render_maps(labels, 0.5)
    fo = FrameRenderer(dev, forward_only=True)
    _render(fo, cam, m, times=2)
    assert fo.r_capacity > 0 and _state(fo)[3], "not a super-tile capacity frame"
    got_l, got_d = fo.render_maps(labels, 0.5)
    assert torch.equal(got_l, want_l) and torch.equal(got_d, want_d)
    assert int((want_l >= 0).sum()) > 0.2 * want_l.numel()

    # gsr_forward against gsr_forward_batch with eight frames
    views = [look_at_view([0.55 - 0.02 * k, 0.35, 0.25 + 0.01 * k], [0.35, 0.05, 0.05], [0, 0, 1], 0.9715089, 0.7551448,
                          640, 480) for k in range(7)] + [cam]
    multi = MultiCameraRenderer(8, dev, forward_only=True)
    for _ in range(2):
        multi.render(views, m["means3D"], m["opacities"], shs=m["shs"], scales=m["scales"], rotations=m["rotations"])
    multi.ensure_valid(lambda: multi.render(views, m["means3D"], m["opacities"], shs=m["shs"], scales=m["scales"],
                                            rotations=m["rotations"]))
    assert multi.last_pack is not None, "the eight frames did not go through one gsr_forward_batch call"
    batched = multi.render_maps(labels, 0.5)
    for k, v in enumerate(views):
        one = FrameRenderer(dev, forward_only=True)
        _render(one, v, m, times=2)
        l1, d1 = one.render_maps(labels, 0.5)
        assert torch.equal(batched[k][0], l1) and torch.equal(batched[k][1], d1), f"frame {k}"
    assert torch.equal(batched[7][0], want_l) and torch.equal(batched[7][1], want_d)

    # the model in the caller's order against a SceneLayout-permuted copy with permuted labels
    from gsworld_amd.layout import SceneLayout

    L = SceneLayout.build(m["means3D"], m["scales"], m["rotations"], labels=labels, opacities=m["opacities"],
                          shs=m["shs"])
    assert L.orig_index is not None
    a = L.arrays
    pm = dict(means3D=a["means3D"], opacities=a["opacities"], shs=a["shs"], scales=a["scales"], rotations=a["rotations"])
    pr = FrameRenderer(dev, forward_only=True)
    _render(pr, cam, pm, times=2, layout=L.layout)
    assert pr._map_meta[2]
    pl_, pd_ = pr.render_maps(a["labels"], 0.5)
    assert torch.equal(pl_, want_l) and torch.equal(pd_, want_d)

    # the ctypes and the compiled binding
    if _C._ext is None or not hasattr(_C._ext, "render_maps"):
        pytest.skip("compiled binding not built")
    outs = []
    for binding in ("ctypes", "ext"):
        f, lab, dep = pr._map_frame(a["labels"], 0.5, None, None)
        lab.fill_(123)
        dep.fill_(-7.0)
        _C.render_maps([f], dev, binding=binding)
        outs.append((lab, dep))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], want_l) and torch.equal(outs[0][1], want_d)


def _loop_setup(n):
    raw = scenes.tabletop_scene("xarm6_align", n=n, seed=1)
    rollout = cl.xarm6_rollout()
    parts, actors = cl.xarm6_rollout_parts(rollout)
    cams = {"right_cam": scenes.sensor_camera("xarm6_align"),
            "wrist_cam": look_at_view([0.55, 0.35, 0.25], [0.35, 0.05, 0.05], [0, 0, 1], 0.9715089, 0.7551448, 640, 480)}
    return raw, rollout, parts, actors, cams


def _wrist(k, steps):
    a = 2.0 * math.pi * k / steps
    return look_at_view([0.55 - 0.10 * math.sin(a), 0.35, 0.25 + 0.05 * math.sin(2.0 * a)], [0.35, 0.05, 0.05], [0, 0, 1],
                        0.9715089, 0.7551448, 640, 480)


@pytest.mark.parametrize("num_envs,n", [(1, None), (3, 400_000)])
def test_closed_loop_maps_in_every_step_mode(cuda_device, num_envs, n):
    dev = cuda_device
    raw, rollout, parts, actors, cams = _loop_setup(n if n is not None else scenes.XARM6_ALIGN_NUM_GAUSSIANS)
    steps = 12
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=3, num_envs=num_envs))
    kw = dict(scaled_parts=actors, num_envs=num_envs, device=dev, maps=MAPS, depth_scale=2.5)
    fast = cl.ClosedLoopRenderer(raw, parts, cams, **kw)
    plain = cl.ClosedLoopRenderer(raw, parts, cams, block_cache=False, tile_reuse=False, **kw)
    assert fast._model_version != 0 and plain._model_version == 0
    fast.reset(*poses[0])
    plain.reset(*poses[0])
    fast.capture()
    assert fast.captured
    names = list(cams)
    for k in range(1, steps + 1):
        cam = {"wrist_cam": _wrist(k, steps)}
        got = fast.step(*poses[k], cameras=cam, ensure=(k % 2 == 0))  # (ahead: the kept pack; waited for: graph replay)
        want = plain.step(*poses[k], cameras=cam, ensure=True)
        torch.cuda.synchronize()
        for name in names:
            assert torch.equal(got[name], want[name]), f"step {k} {name}: frames differ"
            for kind in MAPS:
                assert torch.equal(fast.maps[name][kind], plain.maps[name][kind]), f"step {k} {name} {kind}"
        if k == steps // 2:
            # the maps of this step's state against the restatement (wrist camera of environment 0: lane 1)
            lane = plain.multi.lanes[1]
            _against_restatement(lane, plain._map_labels, 2.5, plain.maps["wrist_cam"]["segmentation"][0],
                                 plain.maps["wrist_cam"]["depth"][0], f"closed loop E={num_envs} step {k}")
    seg = plain.maps["right_cam"]["segmentation"]
    assert seg.shape == (num_envs, 480, 640, 1) and seg.dtype == torch.int16
    assert plain.maps["right_cam"]["depth"].dtype == torch.float32


def test_overflowed_frames_get_background_maps_and_recovered_steps_true_ones(cuda_device):
    dev = cuda_device
    raw, rollout, parts, actors, cams = _loop_setup(150_000)
    E, steps = 3, 30
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps, seed=1, num_envs=E))
    kw = dict(scaled_parts=actors, num_envs=E, device=dev, maps=MAPS)
    safe = cl.ClosedLoopRenderer(raw, parts, cams, bound_capacity=True, **kw)
    tight = cl.ClosedLoopRenderer(raw, parts, cams, bound_capacity=False, growth=1.0, min_capacity=1 << 16, **kw)
    safe.reset(*poses[0])
    tight.reset(*poses[0])
    safe.capture()
    tight.capture()
    for k in range(1, steps):
        safe.step(*poses[k])
        tight.step(*poses[k], ensure=True)
        torch.cuda.synchronize()
        for name in cams:
            for kind in MAPS:
                assert torch.equal(tight.maps[name][kind], safe.maps[name][kind]), f"step {k} {name} {kind}"
    assert tight.recovered_steps > 0, "the rollout never outgrew a list: the test proves nothing"

    # a frame that overflowed and was not rendered again: background maps, never what the buffers held before
    m, labels = _model(raw, dev)
    r = FrameRenderer(dev, forward_only=True)
    cam = scenes.sensor_camera("xarm6_align")
    _render(r, cam, m)
    good_l, _ = r.render_maps(labels)
    assert int((good_l >= 0).sum()) > 0
    r.r_capacity = 4096
    r.render(cam, m["means3D"], m["opacities"], shs=m["shs"], scales=m["scales"], rotations=m["rotations"])
    assert r.stats().overflow
    lab = torch.full((480, 640), 77, dtype=torch.int16, device=dev)
    dep = torch.full((480, 640), 3.0, device=dev)
    r.render_maps(labels, out_label=lab, out_depth=dep)
    torch.cuda.synchronize()
    assert bool((lab == -1).all()) and bool((dep == 0.0).all())


def test_no_maps_requested_changes_nothing(cuda_device):
    dev = cuda_device
    raw, rollout, parts, actors, cams = _loop_setup(200_000)
    steps = 6
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=5))
    off = cl.ClosedLoopRenderer(raw, parts, cams, scaled_parts=actors, device=dev)
    on = cl.ClosedLoopRenderer(raw, parts, cams, scaled_parts=actors, device=dev, maps=("depth",))
    assert off.maps is None and set(on.maps["right_cam"]) == {"depth"}
    for loop in (off, on):
        loop.reset(*poses[0])
        loop.capture()
    for k in range(1, steps + 1):
        cam = {"wrist_cam": _wrist(k, steps)}
        a = off.step(*poses[k], cameras=cam, ensure=True)
        b = on.step(*poses[k], cameras=cam, ensure=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a[n], b[n]) for n in cams), f"step {k}: frames differ with maps on"
    assert int((on.maps["right_cam"]["depth"] > 0).sum()) > 0
