"""Per-environment appearance randomization (include/gsr.h GsrInputs.appearance; csrc/preprocess.hip prep_appearance) on
the GPU: the kernel against the NumPy restatement bit for bit, the closed loop in every step mode, block cache and tile reuse
under changing tables, and the observations that follow the frames."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsworld_amd import _C, _lib
from gsworld_amd import appearance as ap
from gsworld_amd import closed_loop as cl
from gsworld_amd import debug as dbg
from gsworld_amd import scenes
from gsworld_amd.camera import look_at_view
from gsworld_amd.renderer import FrameRenderer

pytestmark = pytest.mark.gpu

GROUPS = {"robot": list(range(1, 17)), "objects": [17, 18]}  # (tabletop_scene: 0 table / floor, 1..16 links, 17 / 18 actors)
RAW = _lib.RAW_OPACITY | _lib.RAW_SCALES | _lib.RAW_ROTATIONS


def _cam(dev, W=320, H=240, k=0):
    return look_at_view([0.75, -0.05 - 0.03 * k, 0.55], [0.3, 0.0, 0.05], [0, 0, 1], 0.9715089, 0.7551448, W, H).to(dev)


def _random_tables(rng, n, G):
    r = ap.AppearanceRandomizer(G, brightness=(0.6, 1.4), contrast=(0.7, 1.3), saturation=(0.5, 1.5), hue=(-0.5, 0.5),
                                gain=(0.8, 1.2), background=((0, 0, 0), (0.5, 0.5, 0.5)), seed=int(rng.integers(1 << 30)))
    t, b = r.sample(n)
    t[..., 3] += rng.uniform(-0.3, 0.3, size=t[..., 3].shape).astype(np.float32)  # (offsets that push some channels below 0)
    return t, b


def _rgb(r: FrameRenderer, cam):
    """The colours of the renderer's last frame in its state: rec2.xyz of the splat records (include/gsr.h GsrStateView)."""
    v = _lib.GsrStateView()
    _lib.check(_lib.lib().gsr_state_view(r._P, cam.image_width, cam.image_height, C.c_int64(1), C.c_void_p(r.geom.data_ptr()),
                                         None, None, C.byref(v)))
    return dbg._view(r.geom, v.splat, 12 * r._P, torch.float32).view(r._P, 12)[:, 8:11]


@pytest.mark.parametrize("binding", ["ext", "ctypes"])
@pytest.mark.parametrize("precomp", [False, True])
def test_kernel_matches_the_restatement_bit_for_bit(cuda_device, binding, precomp, monkeypatch):
    dev = cuda_device
    if binding == "ctypes":
        monkeypatch.setattr(_C, "_ext", None)
    elif _C._ext is None:
        pytest.fail("the compiled binding is not built")
    raw = scenes.tabletop_scene("xarm6_align", n=60_000, seed=3).to(dev)
    P = raw.xyz.shape[0]
    rng = np.random.default_rng(7 + precomp)
    labels = raw.semantics.reshape(-1).float().contiguous()
    # (links 1..8 -> 1, 9..15 -> 2, link 16 -> 7: outside G -> group 0, object 17 -> 3; object 18 lies beyond the LUT of 18
    #  entries -> group 0)
    lut = torch.tensor([0] + [1] * 8 + [2] * 7 + [7, 3], dtype=torch.int32)
    tables, _ = _random_tables(rng, 1, 4)
    kw = dict(opacities=raw.opacity, scales=raw.scaling, rotations=raw.rotation, param_space=RAW)
    if precomp:
        colours = torch.from_numpy(rng.uniform(-0.2, 1.3, size=(P, 3)).astype(np.float32)).to(dev)
        kw.update(colors_precomp=colours)
    else:
        kw.update(shs=raw.features_dc, shs_rest=raw.features_rest, sh_degree=3)
    r = FrameRenderer(dev, forward_only=True)
    cam = _cam(dev)
    r.render(cam, raw.xyz, **kw)  # (sizes the state)
    got = {}
    for app in (None, (tables[0], lut, labels)):
        _rgb(r, cam).fill_(float("nan"))  # (a Gaussian without a record of this frame keeps the NaN)
        r.render(cam, raw.xyz, appearance=app, **kw)
        torch.cuda.synchronize()
        got[app is None] = _rgb(r, cam).cpu().numpy().copy()
    plain, rand = got[True], got[False]
    rec = ~np.isnan(plain[:, 0])
    assert rec.sum() > 1000 and np.array_equal(rec, ~np.isnan(rand[:, 0]))
    lab = labels.cpu().numpy().astype(np.int64)
    assert (lab == 18).any() and (lab == 16).any()  # (a label beyond the LUT, a LUT entry beyond G)
    groups = np.where(lab < lut.numel(), lut.numpy()[np.clip(lab, 0, lut.numel() - 1)], 0)
    groups = np.where((groups >= 0) & (groups < 4), groups, 0)
    want = np.empty_like(plain)
    for g in range(4):
        m = rec & (groups == g)
        want[m] = ap.apply_table(tables[0, g], plain[m])
    assert all((rec & (groups == g)).sum() > 0 for g in range(3))  # (the camera sees the table and both halves of the arm)
    assert np.array_equal(rand[rec].view(np.uint32), want[rec].view(np.uint32))
    assert (rand[rec] == 0).any() and not np.array_equal(rand[rec], plain[rec])


def test_training_frames_refuse_appearance(cuda_device, monkeypatch):
    dev = cuda_device
    raw = scenes.tabletop_scene("xarm6_align", n=20_000, seed=3).to(dev)
    app = (np.eye(3, 4, dtype=np.float32)[None], torch.zeros(1, dtype=torch.int32), raw.semantics.reshape(-1).float())
    for binding in ("ext", "ctypes"):
        if binding == "ctypes":
            monkeypatch.setattr(_C, "_ext", None)
        r = FrameRenderer(dev, forward_only=False)
        with pytest.raises(Exception, match="forward-only"):
            r.render(_cam(dev), raw.xyz, raw.opacity, shs=raw.features_dc, shs_rest=raw.features_rest, scales=raw.scaling,
                     rotations=raw.rotation, param_space=RAW, appearance=app)


# ---- the closed loop ------------------------------------------------------------------------------------------------------
def _setup(n=120_000):
    raw = scenes.tabletop_scene("xarm6_align", n=n, seed=1)
    rollout = cl.xarm6_rollout()
    parts, actors = cl.xarm6_rollout_parts(rollout)
    return raw, rollout, parts, actors


def _cams(size=(320, 240)):
    W, H = size
    return {"right_cam": look_at_view([0.75, -0.05, 0.55], [0.3, 0.0, 0.05], [0, 0, 1], 0.9715089, 0.7551448, W, H),
            "wrist_cam": look_at_view([0.55, 0.35, 0.25], [0.35, 0.05, 0.05], [0, 0, 1], 0.9715089, 0.7551448, W, H)}


@pytest.mark.parametrize("mode", ["eager", "staged", "kept", "device"])
def test_identity_tables_are_free(cuda_device, mode):
    dev = cuda_device
    raw, rollout, parts, actors = _setup()
    E, steps = 2, 4
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=3, num_envs=E))
    kw = dict(scaled_parts=actors, num_envs=E, device=dev)
    app = cl.ClosedLoopRenderer(raw, parts, _cams(), appearance=GROUPS, **kw)
    base = cl.ClosedLoopRenderer(raw, parts, _cams(), **kw)
    if mode == "kept":
        app.eager_when_waited = True
    ident = torch.eye(3, 4).expand(E, 3, 3, 4).contiguous()
    app.set_appearance(ident.to(dev) if mode == "device" else ident)
    for loop in (app, base):
        loop.reset(*poses[0])
    if mode != "eager":
        app.capture()
    for k in range(1, steps + 1):
        a = ident.to(dev) if mode == "device" else ident
        got = app.step(*poses[k], appearance=a if k == 2 else None, ensure=(k % 2 == 0))
        want = base.step(*poses[k], ensure=True)
        torch.cuda.synchronize()
        for n in got:
            assert torch.equal(got[n], want[n]), f"{mode} step {k} {n}: identity tables changed the frame"


def test_randomized_frame_is_the_transformed_model(cuda_device):
    """A randomized loop frame against a FrameRenderer frame of the transformed model whose colours are the restated
    transform of sh.eval_sh: within 1 uint8 LSB on every pixel (colour decides nothing of the compositing)."""
    from gsworld_amd import sh as shm

    dev = cuda_device
    raw, rollout, parts, actors = _setup(60_000)
    poses = list(cl.rollout_poses(rollout, len(actors), steps=2, seed=4, num_envs=1))
    cams = _cams()
    loop = cl.ClosedLoopRenderer(raw, parts, cams, scaled_parts=actors, device=dev, appearance=GROUPS, layout=False)
    rng = np.random.default_rng(11)
    tables, bgs = _random_tables(rng, 1, 3)
    loop.set_appearance(tables, bgs)
    loop.reset(*poses[0])
    frames = loop.step(*poses[1], ensure=True)
    xyz, rot, scaling = loop.op.apply(loop.xyz, loop.rotation, *[t.to(dev) for t in poses[1]], scaling=loop.scaling)
    lab = raw.semantics.reshape(-1).numpy().astype(np.int64)
    grp = np.where((lab >= 1) & (lab <= 16), 1, np.where((lab == 17) | (lab == 18), 2, 0))
    r = FrameRenderer(dev, forward_only=True)
    for n, cam in cams.items():
        cam = cam.to(dev)
        shs = torch.cat([loop.features_dc, loop.features_rest], 1)
        d = xyz - cam.camera_center[None]
        c = shm.eval_sh(3, shs.transpose(1, 2), d / d.norm(dim=1, keepdim=True))
        c = torch.clamp_min(c + 0.5, 0.0).cpu().numpy()
        cc = np.empty_like(c)
        for g in range(3):
            cc[grp == g] = ap.apply_table(tables[0, g], c[grp == g])
        out = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.uint8, device=dev)
        r.render(cam, xyz, loop.opacity, colors_precomp=torch.from_numpy(cc).to(dev), scales=scaling, rotations=rot,
                 param_space=_lib.RAW_SCALES | _lib.RAW_ROTATIONS, bg=torch.from_numpy(bgs[0]).to(dev), rgb8_out=out)
        torch.cuda.synchronize()
        diff = (frames[n][0].int() - out.int()).abs()
        assert int(diff.max()) <= 1, f"{n}: {int(diff.max())} LSB"


def test_each_environment_renders_its_own_table(cuda_device):
    dev = cuda_device
    raw, rollout, parts, actors = _setup()
    E, steps = 3, 3
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=5, num_envs=E))
    rng = np.random.default_rng(12)
    tables, bgs = _random_tables(rng, E, 3)
    loop = cl.ClosedLoopRenderer(raw, parts, _cams(), scaled_parts=actors, num_envs=E, device=dev, appearance=GROUPS)
    refs = [cl.ClosedLoopRenderer(raw, parts, _cams(), scaled_parts=actors, num_envs=1, device=dev, appearance=GROUPS)
            for _ in range(E)]
    loop.set_appearance(tables, bgs)
    loop.reset(*poses[0])
    loop.capture()
    for e, r in enumerate(refs):
        r.set_appearance(tables[e:e + 1], bgs[e:e + 1])
        r.reset(poses[0][0][e], poses[0][1][e])
    for k in range(1, steps + 1):
        got = loop.step(*poses[k], ensure=True)
        for e, r in enumerate(refs):
            one = r.step(poses[k][0][e], poses[k][1][e], ensure=True)
            for n in got:
                assert torch.equal(got[n][e], one[n][0]), f"step {k}: frame ({e}, {n})"
        for n in got:
            assert not torch.equal(got[n][0], got[n][1])


@pytest.mark.parametrize("captured", [False, True])
def test_block_cache_and_tile_reuse_follow_the_tables(cuda_device, captured):
    """Tables that rest, change for one group, for every group, and through env_ids: every frame equals, byte for byte, a
    loop without block cache and tile reuse (a stale block or tile fails here)."""
    dev = cuda_device
    raw, rollout, parts, actors = _setup()
    E, steps = 2, 10
    poses = list(cl.rollout_poses(rollout, len(actors), steps=steps + 1, seed=6, num_envs=E))
    kw = dict(scaled_parts=actors, num_envs=E, device=dev, appearance=GROUPS)
    fast = cl.ClosedLoopRenderer(raw, parts, _cams(), **kw)
    plain = cl.ClosedLoopRenderer(raw, parts, _cams(), block_cache=False, tile_reuse=False, **kw)
    rng = np.random.default_rng(13)
    tables, bgs = _random_tables(rng, E, 3)
    for loop in (fast, plain):
        loop.set_appearance(tables, bgs)
        loop.reset(*poses[0])
    if captured:
        fast.capture()
    for k in range(1, steps + 1):
        upd = None
        if k == 3:  # one group's row of one environment (the loop redraws every word of the environments a call covers)
            t = tables.copy()
            t[1, 2, :, :3] *= 0.5
            upd = dict(tables=t)
        elif k == 5:  # every group, every environment, new backgrounds
            t, b = _random_tables(rng, E, 3)
            upd = dict(tables=t, backgrounds=b)
        elif k == 7:  # a partial reset
            t, b = _random_tables(rng, 1, 3)
            upd = dict(tables=t, backgrounds=b, env_ids=[1])
        elif k == 9:  # device tables
            t, _ = _random_tables(rng, E, 3)
            upd = dict(tables=torch.from_numpy(t).to(dev))
        got = fast.step(*poses[k], appearance=upd, ensure=True)
        want = plain.step(*poses[k], appearance=upd, ensure=True)
        torch.cuda.synchronize()
        for n in got:
            assert torch.equal(got[n], want[n]), f"step {k} {n}: a stale block or tile"


def test_maps_and_point_clouds_follow_the_frames(cuda_device):
    from gsworld_amd.pointcloud import PointCloudSpec

    dev = cuda_device
    raw, rollout, parts, actors = _setup(80_000)
    E = 2
    poses = list(cl.rollout_poses(rollout, len(actors), steps=2, seed=8, num_envs=E))
    kw = dict(scaled_parts=actors, num_envs=E, device=dev, maps=("segmentation", "depth"),
              pointcloud=PointCloudSpec(num_points=None))
    app = cl.ClosedLoopRenderer(raw, parts, _cams(), appearance=GROUPS, **kw)
    base = cl.ClosedLoopRenderer(raw, parts, _cams(), **kw)
    rng = np.random.default_rng(14)
    tables, bgs = _random_tables(rng, E, 3)
    app.set_appearance(tables, bgs)
    for loop in (app, base):
        loop.reset(*poses[0])
        loop.step(*poses[1], ensure=True)
    torch.cuda.synchronize()
    for n in app.maps:
        for m in ("segmentation", "depth"):
            assert torch.equal(app.maps[n][m], base.maps[n][m]), (n, m)
    pc = app.pointcloud
    assert torch.equal(pc["xyzw"], base.pointcloud["xyzw"])
    assert not torch.equal(app.frames["right_cam"], base.frames["right_cam"])
    # dense mode: slot j of environment e is pixel j of camera right_cam, then wrist_cam
    for e in range(E):
        rgb = torch.cat([app.frames[n][e].reshape(-1, 3) for n in app.names])
        valid = pc["xyzw"][e, :, 3] == 1.0
        assert int(valid.sum()) > 0
        assert torch.equal(pc["rgb"][e][valid], rgb[valid])


@pytest.mark.parametrize("frames", [1, 3])
def test_blocks_of_other_groups_stay_cached_when_one_row_changes(cuda_device, frames):
    """The version-word contract as a C-ABI / FrameRenderer caller uses it: one state per frame, model version + FRAME_KEPT,
    laid-out model with part labels, explicit versions.  Between frames ONE row k changes in place and only words k and G
    are bumped, then the tables rest.  Every frame equals, byte for byte, a frame without block cache and tile reuse, and
    every frame after the first keeps blocks (those of the other groups) -- so a stale group word, a wrong word or a wrong
    LUT fails here.  frames=1: the single-frame kernel; frames=3: three frames sharing the model (the group kernel)."""
    from gsworld_amd.renderer import MultiCameraRenderer

    dev = cuda_device
    raw, rollout, parts, actors = _setup()
    poses = list(cl.rollout_poses(rollout, len(actors), steps=1, seed=9, num_envs=1))
    cam = _cams()["right_cam"]
    host = cl.ClosedLoopRenderer(raw, parts, {"right_cam": cam}, scaled_parts=actors, device=dev)  # (laid-out model)
    host.reset(*poses[0])
    model = dict(shs=host.features_dc, shs_rest=host.features_rest, scales=host.scaling, rotations=host.rotation,
                 parts=host.op.parts_of_table(host._table), layout=host.layout)
    assert host.layout is not None
    cam = cam.to(dev)
    G = 3
    lut = torch.tensor([0] + [1] * 16 + [2, 2], dtype=torch.int32, device=dev)
    rng = np.random.default_rng(21 + frames)
    tabs = [torch.from_numpy(_random_tables(rng, 1, G)[0][0]).to(dev).reshape(G, 12).contiguous() for _ in range(frames)]
    vers = [torch.arange(1, G + 2, dtype=torch.int32, device=dev) * (100 + l) for l in range(frames)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    ren = dict(forward_only=True, want_radii=False, want_float=False)
    multi = MultiCameraRenderer(frames, dev, **ren)
    refs = [FrameRenderer(dev, **ren) for _ in range(frames)]
    H, W = cam.image_height, cam.image_width
    outs = [torch.zeros((H, W, 3), dtype=torch.uint8, device=dev) for _ in range(frames)]
    ref_outs = [torch.zeros((H, W, 3), dtype=torch.uint8, device=dev) for _ in range(frames)]
    cached_ps = _lib.RAW_SCALES | _lib.RAW_ROTATIONS | _lib.model_version(0x5A5A5) | _lib.FRAME_KEPT
    changes = [None, None, 1, None, 0, 2, None, 1]  # (row changed before frame f; the lanes shift it by their number)
    for f, k in enumerate(changes):
        if k is not None:
            for l in range(frames):
                row = (k + l) % G
                tabs[l][row, :9] *= 0.8 + 0.1 * l
                tabs[l][row, 3::4] += 0.05
                vers[l][row] += 1
                vers[l][G] += 1
        apps = [(tabs[l], lut, None, vers[l]) for l in range(frames)]
        multi.render([cam] * frames, host.xyz, host.opacity, rgb8_out=outs,
                     per_lane=[dict(appearance=a, bg=bg) for a in apps], param_space=cached_ps, **model)
        for l in range(frames):
            refs[l].render(cam, host.xyz, host.opacity, rgb8_out=ref_outs[l], appearance=apps[l], bg=bg,
                           param_space=_lib.RAW_SCALES | _lib.RAW_ROTATIONS, **model)
        torch.cuda.synchronize()
        for l in range(frames):
            assert torch.equal(outs[l], ref_outs[l]), f"frame {f} lane {l}: a stale block or tile (row {k} changed)"
            st = dbg.sort_state(multi.lanes[l].geom)
            if f > 0:
                assert st["kept_blocks"], f"frame {f} lane {l}: no block kept (row {k} changed: the others' should stay)"
            if f > 1 and k is None:
                assert st["kept_tiles"], f"frame {f} lane {l}: no tile kept with everything at rest"
