"""Point-cloud observations (include/gsr.h gsr_render_pointcloud, csrc/pointcloud.hip) on the GPU: the kernels against the
NumPy restatement (tests/test_pointcloud_cpu.py) bit for bit, the geometry of a rendered frame, the closed loop in every
step mode, and both bindings."""
import math

import numpy as np
import pytest
import torch

from gsworld_amd import _C
from gsworld_amd import closed_loop as cl
from gsworld_amd import scenes
from gsworld_amd.camera import look_at_view
from gsworld_amd.pointcloud import PointCloudSpec, render_pointcloud, sim_from_scene
from gsworld_amd.renderer import FrameRenderer
from tests.test_pointcloud_cpu import restate_pointcloud

pytestmark = pytest.mark.gpu

F32 = np.float32
MAPS = ("segmentation", "depth")


def _rigid():
    th, ph = 0.6, -0.25
    Rz = np.array([[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(ph), -math.sin(ph)], [0.0, math.sin(ph), math.cos(ph)]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rz @ Rx, [0.3, -0.1, 0.05]
    return M


def _views_of(depth, labels, frames, cams, e):
    """The restatement's per-camera inputs of environment e (host copies)."""
    out = []
    for name, cam in cams.items():
        out.append(dict(depth=depth[name][e].reshape(cam.image_height, cam.image_width).cpu().numpy(),
                        label=None if labels is None else labels[name][e].reshape(cam.image_height, cam.image_width).cpu().numpy(),
                        rgb=None if frames is None else frames[name][e].cpu().numpy(),
                        viewmatrix=cam.world_view_transform.cpu().numpy().reshape(-1),
                        tanfovx=F32(cam.tanfovx), tanfovy=F32(cam.tanfovy)))
    return out


def _against_restatement(got, depth, labels, frames, cams, spec, depth_scale, what):
    torch.cuda.synchronize()
    mode = "dense" if spec.num_points is None else spec.sample
    E = got["count"].shape[0]
    A = np.asarray(spec.affine(), F32)
    for e in range(E):
        xyzw, rgb, seg, count, _ = restate_pointcloud(_views_of(depth, labels, frames, cams, e), mode,
                                                      K=spec.num_points or 0, fps_candidates=spec.fps_candidates, A=A,
                                                      crop=spec.crop, exclude=spec.exclude_labels, depth_scale=depth_scale)
        g = {k: v[e].cpu().numpy() for k, v in got.items() if k != "count"}
        assert int(got["count"][e]) == count, f"{what} env {e}: count {int(got['count'][e])} != {count}"
        bad = np.flatnonzero(np.any(g["xyzw"].view(np.uint32) != xyzw.view(np.uint32), axis=1))
        assert bad.size == 0, f"{what} env {e}: {bad.size} slots differ in xyzw, first {bad[:5]}"
        assert np.array_equal(g["rgb"], rgb), f"{what} env {e}: rgb"
        assert np.array_equal(g["segmentation"].reshape(-1), seg), f"{what} env {e}: segmentation"
    return count


def _synthetic(dev, E=3, seed=0):
    gen = torch.Generator().manual_seed(seed)
    cams = {"a": look_at_view([0.6, 0.3, 0.5], [0.0, 0.0, 0.0], [0, 0, 1], 1.1, 0.9, 128, 96),
            "b": look_at_view([-0.4, 0.5, 0.3], [0.05, 0.0, 0.1], [0, 0, 1], 0.8, 0.7, 96, 64)}
    depth, labels, frames = {}, {}, {}
    for name, cam in cams.items():
        H, W = cam.image_height, cam.image_width
        d = 0.3 + 1.2 * torch.rand((E, H, W, 1), generator=gen)
        d[torch.rand((E, H, W, 1), generator=gen) < 0.08] = 0.0
        depth[name] = d.to(dev)
        labels[name] = torch.randint(-1, 24, (E, H, W, 1), generator=gen, dtype=torch.int16).to(dev)
        frames[name] = torch.randint(0, 256, (E, H, W, 3), generator=gen, dtype=torch.uint8).to(dev)
        cam.world_view_transform = cam.world_view_transform.to(dev)
    return cams, depth, labels, frames


def test_functional_api_matches_the_restatement(cuda_device):
    dev = cuda_device
    cams, depth, labels, frames = _synthetic(dev)
    A = sim_from_scene(_rigid(), 1.3)
    common = dict(out_from_scene=A, crop=((-5.0, -5.0, -0.6), (5.0, 5.0, 5.0)), exclude_labels=(3, 7))
    for spec in (PointCloudSpec(**common), PointCloudSpec(num_points=1500, sample="stride", **common),
                 PointCloudSpec(num_points=1024, sample="fps", fps_candidates=8192, **common),
                 PointCloudSpec(num_points=1024, sample="fps", fps_candidates=500, **common),
                 PointCloudSpec(num_points=64, sample="fps", fps_candidates=16384)):
        got = render_pointcloud(depth, labels, frames, cams, spec, depth_scale=1.5)
        what = f"{spec.sample if spec.num_points else 'dense'} K={spec.num_points} M={spec.fps_candidates}"
        _against_restatement(got, depth, labels, frames, cams, spec, 1.5, what)
        cnt = got["count"].cpu()
        if spec.num_points == 1024 and spec.fps_candidates == 8192:
            assert bool((cnt == 1024).all())
        if spec.fps_candidates == 500 and spec.num_points == 1024:
            assert bool((cnt == 500).all()), "M < K: min(M, K) picks"
        if spec.num_points is None:
            assert int(cnt.min()) > 8192, "fewer valid points than the FPS candidates: the FPS cases show less"
    # no label map and no frame: segmentation -1, rgb 0 for every point
    spec = PointCloudSpec(num_points=300, sample="stride")
    got = render_pointcloud(depth, None, None, cams, spec)
    _against_restatement(got, depth, None, None, cams, spec, 1.0, "no labels / frames")
    assert bool((got["segmentation"] == -1).all()) and bool((got["rgb"] == 0).all())
    with pytest.raises(ValueError):
        render_pointcloud(depth, None, None, cams, PointCloudSpec(exclude_labels=(1,)))


def test_geometry_on_a_rendered_frame(cuda_device):
    dev = cuda_device
    raw, cam = scenes.random_scene_camera_frame(100_000, seed=0), scenes.identity_camera(256, 256, 60.0)
    means, shs, op, sc, rot = raw.to(dev).activated()
    labels = raw.semantics.reshape(-1).to(dev, torch.float32).contiguous() if raw.semantics is not None else \
        (torch.arange(means.shape[0], device=dev) % 997).to(torch.float32)
    r = FrameRenderer(dev)
    r.render(cam, means, op, shs=shs, scales=sc, rotations=rot, exact=True)
    ds = 1.75
    lab, dep = r.render_maps(labels, depth_scale=ds)
    W, H = cam.image_width, cam.image_height
    got = render_pointcloud([dep.view(1, H, W)], [lab.view(1, H, W)], None, [cam], PointCloudSpec(), depth_scale=ds)
    torch.cuda.synchronize()
    w = got["xyzw"][0, :, 3].cpu().numpy()
    ok = w == 1.0
    assert ok.sum() > 0.05 * W * H
    q = got["xyzw"][0, :, :3].cpu().numpy().astype(np.float64)[ok]
    pix = np.flatnonzero(ok)
    hom = np.c_[q, np.ones(len(q))]
    clip = hom @ cam.full_proj_transform.double().numpy()
    ndc = clip[:, :2] / clip[:, 3:4]
    px = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    py = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    err = np.hypot(px - pix % W, py - pix // W)
    print(f"re-projection: max {err.max():.2e} px over {len(pix)} points")
    assert err.max() < 1e-3
    zv = (hom @ cam.world_view_transform.double().numpy())[:, 2]
    want = dep.reshape(-1).cpu().numpy()[pix].astype(np.float64) / ds
    assert np.abs(zv / want - 1.0).max() < 1e-5

    # a few isolated opaque Gaussians at known simulator positions, seen through cam_maniskill2gs's chain
    rigid, s = _rigid(), 1.3
    X = np.array([[0.40, 0.05, 0.10], [0.55, -0.12, 0.02], [0.35, 0.15, 0.20], [0.60, 0.10, -0.05]])
    scene = (rigid @ np.c_[s * X, np.ones(len(X))].T).T[:, :3]
    n = len(X)
    means = torch.tensor(scene, dtype=torch.float32, device=dev)
    scales = torch.full((n, 3), 0.008, device=dev)
    rots = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * n, device=dev)
    ops = torch.full((n, 1), 0.99, device=dev)
    shs = torch.zeros((n, 16, 3), device=dev)
    labs = torch.arange(1, n + 1, device=dev, dtype=torch.float32)
    eye_sim = np.array([0.1, 0.0, 0.5])
    eye = rigid[:3, :3] @ (s * eye_sim) + rigid[:3, 3]
    target = rigid[:3, :3] @ (s * X.mean(0)) + rigid[:3, 3]
    cam = look_at_view(eye, target, rigid[:3, :3] @ np.array([0.0, 0.0, 1.0]), 0.9, 0.7, 160, 120)
    r = FrameRenderer(dev)
    r.render(cam, means, ops, shs=shs, scales=scales, rotations=rots, exact=True)
    lab, dep = r.render_maps(labs, depth_scale=1.0 / s)
    A = sim_from_scene(rigid, s)
    got = render_pointcloud([dep.view(1, 120, 160)], [lab.view(1, 120, 160)], None, [cam], PointCloudSpec(out_from_scene=A),
                            depth_scale=1.0 / s)
    torch.cuda.synchronize()
    seg = got["segmentation"][0, :, 0].cpu().numpy()
    pts = got["xyzw"][0, :, :3].cpu().numpy().astype(np.float64)
    W2C = cam.world_view_transform.double().numpy().T
    eye_s = eye_sim
    for g in range(n):
        mine = pts[seg == g + 1]
        assert len(mine) >= 3, f"Gaussian {g} covers {len(mine)} pixels"
        centre_depth = (W2C @ np.r_[scene[g], 1.0])[2] / s  # (view depth in simulator metres)
        # every point of its pixels: view depth = the centre's (the median contributor's depth), in simulator metres
        sc_pts = (np.linalg.inv(np.vstack([A, [0, 0, 0, 1]])) @ np.c_[mine, np.ones(len(mine))].T).T
        zs = (W2C @ sc_pts.T).T[:, 2] / s
        assert np.abs(zs - centre_depth).max() < 1e-5 * centre_depth
        # the point nearest the centre lies on the ray through it: within a pixel's footprint at that depth
        ray = (X[g] - eye_s) / np.linalg.norm(X[g] - eye_s)
        rel = mine - eye_s
        perp = np.linalg.norm(rel - (rel @ ray)[:, None] * ray, axis=1)
        footprint = 2.0 * centre_depth * cam.tanfovx / 160
        assert perp.min() < footprint, f"Gaussian {g}: nearest point {perp.min():.2e} m off its ray"


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


def _same_cloud(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("xyzw", "rgb", "segmentation", "count"))


@pytest.mark.parametrize("num_envs,maps,spec", [
    (1, (), PointCloudSpec(num_points=1024, sample="fps", fps_candidates=8192, out_from_scene=sim_from_scene(_rigid(), 1.3))),
    (3, ("depth",), PointCloudSpec(num_points=2048, sample="stride", crop=((-0.5, -0.5, -0.1), (1.0, 1.0, 1.0)),
                                   exclude_labels=(0,))),
    (1, MAPS, PointCloudSpec())])
def test_closed_loop_point_clouds_in_every_step_mode(cuda_device, num_envs, maps, spec):
    dev = cuda_device
    raw, rollout, parts, actors, cams = _loop_setup(400_000)
    steps = 8
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=3, num_envs=num_envs))
    kw = dict(scaled_parts=actors, num_envs=num_envs, device=dev, maps=maps, depth_scale=2.5, pointcloud=spec)
    fast = cl.ClosedLoopRenderer(raw, parts, cams, **kw)
    plain = cl.ClosedLoopRenderer(raw, parts, cams, block_cache=False, tile_reuse=False, **kw)
    assert (fast.maps is None) == (not maps) and (maps == () or set(fast.maps["right_cam"]) == set(maps))
    fast.reset(*poses[0])
    plain.reset(*poses[0])
    fast.capture()
    assert fast.captured
    N = 2 * 640 * 480 if spec.num_points is None else spec.num_points
    assert fast.pointcloud["xyzw"].shape == (num_envs, N, 4) and fast.pointcloud["segmentation"].shape == (num_envs, N, 1)
    for k in range(1, steps + 1):
        cam = {"wrist_cam": _wrist(k, steps)}
        got = fast.step(*poses[k], cameras=cam, ensure=(k % 2 == 0))  # (ahead: the kept pack; waited for: graph replay)
        want = plain.step(*poses[k], cameras=cam, ensure=True)
        torch.cuda.synchronize()
        for name in cams:
            assert torch.equal(got[name], want[name]), f"step {k} {name}: frames differ"
        assert _same_cloud(fast.pointcloud, plain.pointcloud), f"step {k}: clouds differ"
        if k == steps // 2:
            # the functional API fed this step's maps, frames and (device-resident) cameras
            cams_now = dict(zip(plain.names, plain.cameras))
            dep = {n: plain._map_bufs[n]["depth"] for n in plain.names}
            lab = {n: plain._map_bufs[n]["segmentation"] for n in plain.names}
            ref = render_pointcloud(dep, lab, plain.frames, cams_now, spec, depth_scale=2.5)
            torch.cuda.synchronize()
            assert _same_cloud(ref, plain.pointcloud), f"step {k}: the loop's cloud is not the functional API's"
            if num_envs == 1:
                _against_restatement(plain.pointcloud, dep, lab, plain.frames, cams_now, spec, 2.5, f"loop step {k}")
    cnt = plain.pointcloud["count"].cpu()
    assert int(cnt.min()) > 0


def test_overflowed_frames_give_no_points_and_recovered_steps_true_ones(cuda_device):
    dev = cuda_device
    raw, rollout, parts, actors, cams = _loop_setup(150_000)
    E, steps = 3, 30
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps, seed=1, num_envs=E))
    spec = PointCloudSpec(num_points=512, sample="fps", fps_candidates=4096)
    kw = dict(scaled_parts=actors, num_envs=E, device=dev, pointcloud=spec)
    safe = cl.ClosedLoopRenderer(raw, parts, cams, bound_capacity=True, **kw)
    tight = cl.ClosedLoopRenderer(raw, parts, cams, bound_capacity=False, growth=1.0, min_capacity=1 << 16, **kw)
    assert safe.maps is None
    safe.reset(*poses[0])
    tight.reset(*poses[0])
    safe.capture()
    tight.capture()
    for k in range(1, steps):
        safe.step(*poses[k])
        tight.step(*poses[k], ensure=True)
        torch.cuda.synchronize()
        assert _same_cloud(tight.pointcloud, safe.pointcloud), f"step {k}"
    assert tight.recovered_steps > 0, "the rollout never outgrew a list: the test proves nothing"

    # a frame that overflowed and was not rendered again: no points at all
    means, shs, op, sc, rot = raw.to(dev).activated()
    labels = raw.semantics.reshape(-1).to(dev, torch.float32).contiguous()
    r = FrameRenderer(dev, forward_only=True)
    cam = scenes.sensor_camera("xarm6_align")
    r.render(cam, means, op, shs=shs, scales=sc, rotations=rot)
    r.ensure_valid(lambda: r.render(cam, means, op, shs=shs, scales=sc, rotations=rot))
    lab, dep = r.render_maps(labels)
    good = render_pointcloud([dep.view(1, 480, 640)], [lab.view(1, 480, 640)], None, [cam], PointCloudSpec())
    torch.cuda.synchronize()
    assert int(good["count"][0]) > 0
    r.r_capacity = 4096
    r.render(cam, means, op, shs=shs, scales=sc, rotations=rot)
    assert r.stats().overflow
    r.render_maps(labels, out_label=lab, out_depth=dep)
    for s in (PointCloudSpec(), PointCloudSpec(num_points=256, sample="fps")):
        bad = render_pointcloud([dep.view(1, 480, 640)], [lab.view(1, 480, 640)], None, [cam], s)
        torch.cuda.synchronize()
        assert int(bad["count"][0]) == 0 and bool((bad["xyzw"] == 0).all()) and bool((bad["segmentation"] == -1).all())


def test_no_point_cloud_requested_changes_nothing(cuda_device):
    dev = cuda_device
    raw, rollout, parts, actors, cams = _loop_setup(200_000)
    steps = 6
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=5))
    base = dict(scaled_parts=actors, device=dev, maps=MAPS)
    off = cl.ClosedLoopRenderer(raw, parts, cams, **base)
    none = cl.ClosedLoopRenderer(raw, parts, cams, pointcloud=None, **base)
    on = cl.ClosedLoopRenderer(raw, parts, cams, pointcloud=PointCloudSpec(num_points=256, sample="stride"), **base)
    assert off.pointcloud is None and none.pointcloud is None and on.pointcloud is not None
    for loop in (off, none, on):
        loop.reset(*poses[0])
        loop.capture()
    for k in range(1, steps + 1):
        cam = {"wrist_cam": _wrist(k, steps)}
        a = off.step(*poses[k], cameras=cam, ensure=True)
        b = none.step(*poses[k], cameras=cam, ensure=True)
        c = on.step(*poses[k], cameras=cam, ensure=True)
        torch.cuda.synchronize()
        for n in cams:
            assert torch.equal(a[n], b[n]) and torch.equal(a[n], c[n]), f"step {k} {n}: frames differ"
            for kind in MAPS:
                assert torch.equal(off.maps[n][kind], none.maps[n][kind]), f"step {k} {n} {kind}"
                assert torch.equal(off.maps[n][kind], on.maps[n][kind]), f"step {k} {n} {kind} with a cloud"
    assert int(on.pointcloud["count"][0]) == 256


def test_both_bindings_give_the_same_bytes(cuda_device):
    if _C._ext is None or not hasattr(_C._ext, "CloudPack"):
        pytest.skip("compiled binding not built")
    dev = cuda_device
    cams, depth, labels, frames = _synthetic(dev, E=2, seed=4)
    for spec in (PointCloudSpec(out_from_scene=sim_from_scene(_rigid(), 0.8)),
                 PointCloudSpec(num_points=777, sample="stride", exclude_labels=(5,)),
                 PointCloudSpec(num_points=500, sample="fps", fps_candidates=3000, crop=((-1, -1, -1), (1, 1, 1)))):
        outs = []
        for binding in ("ctypes", "ext"):
            o = render_pointcloud(depth, labels, frames, cams, spec, depth_scale=0.75, binding=binding)
            torch.cuda.synchronize()
            outs.append({k: v.clone() for k, v in o.items()})
        assert _same_cloud(outs[0], outs[1])
