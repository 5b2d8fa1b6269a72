"""Backward parity helpers: HIP path (through the C ABI / the autograd Function) vs the backward oracle."""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import torch

from gsworld_amd import scenes
from gsworld_amd.camera import look_at_view
from oracle import gs_oracle as go
from tests import helpers as hp

GRAD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
              "dL_drotations")


def gpu_forward_backward(inp, st, bg, dL_dcolor, dL_dinvdepth, device="cuda", colors_precomp=None,
                         cov3D_precomp=None):
    from gsworld_amd import _C

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    empty = torch.empty(0, device=device)
    sh = empty if colors_precomp is not None else t(inp["shs"])
    colors = t(colors_precomp) if colors_precomp is not None else empty
    scales = empty if cov3D_precomp is not None else t(inp["scales"])
    rots = empty if cov3D_precomp is not None else t(inp["rotations"])
    cov = t(cov3D_precomp) if cov3D_precomp is not None else empty
    args = dict(bg=t(np.asarray(bg, np.float32)), means=t(inp["means3D"]), op=t(inp["opacities"]).reshape(-1, 1),
                view=t(inp["viewmatrix"]).reshape(4, 4), proj=t(inp["projmatrix"]).reshape(4, 4), campos=t(inp["campos"]))
    old = _C.NEAR_PLANE
    _C.NEAR_PLANE = st.near_plane
    try:
        R, color, radii, gB, bB, iB, invd = _C.rasterize_gaussians(
            args["bg"], args["means"], colors, args["op"], scales, rots, st.scale_modifier, cov, args["view"],
            args["proj"], st.tanfovx, st.tanfovy, st.image_height, st.image_width, sh, st.sh_degree, args["campos"],
            False, st.antialiasing, False)
        grads = _C.rasterize_gaussians_backward(
            args["bg"], args["means"], radii, colors, args["op"], scales, rots, st.scale_modifier, cov, args["view"],
            args["proj"], st.tanfovx, st.tanfovy, t(dL_dcolor), None if dL_dinvdepth is None else t(dL_dinvdepth), sh,
            st.sh_degree, args["campos"], gB, R, bB, iB, st.antialiasing, False)
    finally:
        _C.NEAR_PLANE = old
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(GRAD_NAMES, grads)}, color.cpu().numpy()


# the fixed-seed cases of tests/test_backward_gpu.py: every element within 2e-3 relative (observed: all of them, worst
# normalised error 5e-4 -- float atomics in another order than the oracle's sums); the randomised sweeps keep the
# wider defaults below
SUITE_TOLERANCES = dict(frac_ok=0.9995, max_norm_err=5e-3)


def compare_grads(ref: dict, got: dict, names=GRAD_NAMES, rtol=2e-3, frac_ok=0.999, max_norm_err=2e-2):
    rep = {}
    for k in names:
        a, b = ref[k], got[k].reshape(ref[k].shape)
        if a.size == 0:
            continue
        scale = float(np.abs(a).max())
        if scale == 0.0:
            assert float(np.abs(b).max()) == 0.0, f"{k}: expected all-zero gradient"
            continue
        err = np.abs(a - b) / (np.abs(a) + 1e-3 * scale)
        rep[k] = dict(max_norm_err=float(err.max()), frac_within=float((err <= rtol).mean()), scale=scale)
        assert np.isfinite(b).all(), f"{k}: non-finite gradient"
        assert rep[k]["frac_within"] >= frac_ok, (k, rep[k])
        assert rep[k]["max_norm_err"] <= max_norm_err, (k, rep[k])
    return rep


def run_case(n, W, H, seed, device="cuda", aa=False, deg=3, bg=(0.3, 0.1, 0.6), scale_boost=0.5, with_invdepth=True,
             raw=None, cam=None, M=16, **tolerances):
    """``tolerances``: rtol / frac_ok / max_norm_err of :func:`compare_grads` (its defaults are the randomised sweep's
    bounds; the fixed-seed suite tests pass the tighter SUITE_TOLERANCES).  ``cam``: the identity view at the origin
    unless given; ``M``: SH coefficients per Gaussian (the first M of the scene's 16)."""
    raw = raw if raw is not None else scenes.random_scene_camera_frame(n, seed=seed)
    if scale_boost:
        raw.scaling += scale_boost
    cam = cam if cam is not None else scenes.identity_camera(W, H, 60.0)
    inp = hp.np_inputs(raw, cam)
    inp["shs"] = np.ascontiguousarray(inp["shs"][:, :M])
    st = hp.oracle_settings(cam, antialiasing=aa, sh_degree=deg, sh_coeffs=M)
    bg = np.asarray(bg, np.float32)
    fwd = hp.oracle_forward(inp, st, bg, border_eps=0.0)
    rng = np.random.default_rng(seed)
    dLc = rng.standard_normal((3, cam.image_height, cam.image_width)).astype(np.float32)
    dLd = rng.standard_normal((1, cam.image_height, cam.image_width)).astype(np.float32) if with_invdepth else None
    ref = go.backward(st, fwd, inp, bg, dLc, dLd)
    got, color = gpu_forward_backward(inp, st, bg, dLc, dLd, device=device)
    assert np.abs(color - fwd["color"]).max() < 1e-3
    return compare_grads(ref, got, **tolerances)


def smoke_backward(device="cuda:0"):
    return run_case(5000, 96, 64, seed=41, device=device)


# ---- rotated camera, edge scenes, caller-owned gradient buffers (tests/test_backward_edges_gpu.py) ---------------------
IMAGE_SIZES = ((48, 32), (70, 50), (17, 9), (5, 37))  # the last two: narrower / lower than one 16 x 16 tile
TANFOVX, TANFOVY = 0.61, 0.37                         # unequal: an fx / fy or tanfovx / tanfovy swap shows
EDGE_BG = (0.3, 0.1, 0.6)
GUARD = 64
SENTINEL = -777.25
BASE, CULL_BEHIND, CULL_OFF, OFF_X, OFF_Y, OPAQUE, DEEP = range(7)


def rotated_camera(W, H):
    """Eye off the origin; about 12 degrees of yaw, 10 of pitch and 25 of roll against the identity view; tan(fov / 2) of
    0.61 horizontally and 0.37 vertically."""
    roll = math.radians(25.0)
    return look_at_view((0.9, -0.6, -0.8), (0.1, 0.05, 3.0), (math.sin(roll), -math.cos(roll), 0.0),
                        2.0 * math.atan(TANFOVX), 2.0 * math.atan(TANFOVY), W, H)


def random_rotated_camera(rng, W, H):
    """A random look-at camera with unequal fields of view on the camera-frame scenes of gsworld_amd.scenes (fuzz tools)."""
    roll = float(rng.uniform(-math.pi, math.pi))
    eye = rng.uniform((-1.0, -1.0, -1.5), (1.0, 1.0, 0.5))
    target = rng.uniform((-0.3, -0.3, 2.5), (0.3, 0.3, 3.5))
    return look_at_view(eye, target, (math.sin(roll), -math.cos(roll), 0.0), math.radians(float(rng.uniform(35, 100))),
                        math.radians(float(rng.uniform(35, 100))), W, H)


def edge_scene(P=3000, W=48, H=32, seed=0, deep=False, upstream_branches=True, all_culled=False):
    """-> (raw, cam, kind): ``scenes.random_scene_camera_frame(near_fraction=0)`` under :func:`rotated_camera`, with the
    positions, sizes, opacities and colours of chosen Gaussians replaced so that the paths of csrc/backward.hip are taken
    on purpose.  The scene is laid out in the CAMERA's frame and carried into the world through the inverse view matrix,
    so what it holds does not depend on the pose while every kernel sees a full view matrix.  ``kind`` (P,):

    BASE         centre on screen, z in [1.5, 4.5], sizes of a few pixels
    CULL_BEHIND  behind the near plane                                  (culled)
    CULL_OFF     small, three to five half-widths off the left / top    (culled)
    OFF_X/OFF_Y  |t/z| between 1.35 and 1.6 tan(fov/2) in x / y and large enough to reach the image: the clamp branch
    OPAQUE       on screen, large, opacity above 0.99: saturates pixels
    DEEP         (``deep``) several hundred faint splats in front of one pixel: three staging rounds of the compositor

    Block [256, 512) is culled entirely, block [512, 768) but for Gaussian 600; about 4 % of all Gaussians carry a colour
    channel far below zero (clamped).  tests/test_backward_scenes_cpu.py asserts all of it from the oracle's forward.

    ``upstream_branches=False`` leaves OFF_X / OFF_Y / OPAQUE out (they stay BASE).  In those two places upstream's backward,
    which the kernels and the oracle restate, is NOT the derivative of the forward as autograd sees it: behind the clamp
    of t/z it differentiates J as if the clamped t did not depend on z, and it lets the gradient through
    min(0.99, alpha).  A comparison with autograd (tests/test_backward_oracle.py) cannot hold such Gaussians."""
    raw = scenes.random_scene_camera_frame(P, seed=seed, near_fraction=0.0)
    cam = rotated_camera(W, H)
    rng = np.random.default_rng(1000 + seed)
    r = rng.random(P)
    kind = np.full(P, BASE)
    for k, lo, hi in ((CULL_BEHIND, 0.0, 0.06), (CULL_OFF, 0.06, 0.12), (OFF_X, 0.12, 0.16), (OFF_Y, 0.16, 0.20),
                      (OPAQUE, 0.20, 0.215)):
        kind[(r >= lo) & (r < hi)] = k
    if not upstream_branches:
        kind[:] = np.where((kind == OFF_X) | (kind == OFF_Y) | (kind == OPAQUE), BASE, kind)
    idx = np.arange(P)
    if deep:
        kind[(idx >= 1024) & (idx < 2048) & (kind == BASE)] = DEEP
    for lo, hi in ((256, 512), (512, 768)):
        sel = (idx >= lo) & (idx < hi)
        kind[sel] = np.where(idx[sel] % 2 == 0, CULL_BEHIND, CULL_OFF)
    for i, k in ((0, BASE), (1, CULL_BEHIND), (2, BASE), (600, BASE), (2048, BASE)):  # (what the P tails end on)
        if i < P:
            kind[i] = k
    if all_culled:  # (num_rendered == 0 with P > 0)
        kind[:] = np.where(idx % 2 == 0, CULL_BEHIND, CULL_OFF)
    u, v = rng.uniform(-0.95, 0.95, P), rng.uniform(-0.95, 0.95, P)
    z = rng.uniform(1.5, 4.5, P)
    logs = raw.scaling.numpy().astype(np.float64) + 1.0
    logit = raw.opacity.numpy().astype(np.float64).reshape(-1)
    side = np.where(rng.random(P) < 0.5, -1.0, 1.0)
    far, big = rng.uniform(3.0, 5.0, P), rng.uniform(1.35, 1.6, P)
    on_x = rng.random(P) < 0.5
    m = kind == CULL_BEHIND
    z[m] = rng.uniform(-2.0, 0.04, P)[m]
    m = kind == CULL_OFF
    u[m & on_x], v[m & ~on_x] = -far[m & on_x], -far[m & ~on_x]
    logs[m] = math.log(0.01)
    for k, arr in ((OFF_X, u), (OFF_Y, v)):
        m = kind == k
        arr[m] = (side * big)[m]
        z[m] = rng.uniform(2.0, 4.0, P)[m]
        logs[m] = np.log(rng.uniform(0.35, 0.6, (P, 3)))[m]
        logit[m] = rng.uniform(-3.5, -1.5, P)[m]
    m = kind == OPAQUE
    u[m], v[m] = 0.8 * u[m], 0.8 * v[m]
    z[m] = rng.uniform(3.0, 4.5, P)[m]
    logs[m] = np.log(rng.uniform(0.15, 0.35, (P, 3)))[m]
    logit[m] = rng.uniform(6.0, 9.0, P)[m]
    m = kind == DEEP
    if m.any():  # around pixel (24.5, 7.5) of the 48 x 32 image, in front of everything else
        z[m] = rng.uniform(0.8, 1.2, P)[m]
        u[m] = (2.0 * (24.5 + rng.uniform(-2.0, 2.0, P)[m]) + 1.0) / W - 1.0
        v[m] = (2.0 * (7.5 + rng.uniform(-2.0, 2.0, P)[m]) + 1.0) / H - 1.0
        logs[m] = math.log(0.08)
        logit[m] = rng.uniform(-5.0, -4.6, P)[m]
    for i in (0, 2, 600, 2048):  # a workgroup's only visible Gaussian: in the middle of the image, a few pixels wide
        if i < P and kind[i] == BASE:
            u[i], v[i], z[i], logs[i], logit[i] = 0.4 * u[i], 0.4 * v[i], 2.5, math.log(0.12), 1.0
    zz = np.where(z > 0.05, z, 3.0)  # (the lateral place of a Gaussian behind the camera does not matter)
    p_cam = np.stack((u * TANFOVX * zz, v * TANFOVY * zz, z, np.ones(P)), 1)
    Vinv = np.linalg.inv(cam.world_view_transform.numpy().astype(np.float64))
    raw.xyz = torch.from_numpy((p_cam @ Vinv)[:, :3].astype(np.float32)).contiguous()
    raw.scaling = torch.from_numpy(logs.astype(np.float32)).contiguous()
    raw.opacity = torch.from_numpy(logit.astype(np.float32).reshape(P, 1)).contiguous()
    raw.features_rest = (raw.features_rest * 4.0).contiguous()  # a view-direction term worth comparing
    dark = np.nonzero((rng.random(P) < 0.04) & ~np.isin(idx, (0, 2, 600, 2048)))[0]
    chans = rng.random((dark.size, 3)) < 0.5
    chans[~chans.any(1), 0] = True
    dc = raw.features_dc.numpy().copy()
    dc[dark, 0] = np.where(chans, -3.0, dc[dark, 0]).astype(np.float32)
    raw.features_dc = torch.from_numpy(dc).contiguous()
    return raw, cam, kind


def expect_culled(kind):
    return (kind == CULL_BEHIND) | (kind == CULL_OFF)


@functools.lru_cache(maxsize=None)
def edge_case(P=3000, W=48, H=32, aa=False, deg=3, M=16, scale_modifier=1.0, with_invdepth=True, deep=False,
              precomp=False, seed=0, upstream_branches=True, all_culled=False, raw_space=False):
    """The oracle's forward and backward on :func:`edge_scene`, computed once per argument tuple and shared by every test
    that needs it (nobody writes into the result).  ``precomp``: colours and 3D covariances are given instead of SH /
    scales / rotations.  ``raw_space``: the opacity / scale / rotation inputs are the RAW parameters (quaternions of
    length 0.2 to 5); the oracle runs on their canonical float32 activations (``go.activate_params``), and ``ref_raw``
    holds its gradients carried to the raw parameters by the chain rule in binary64 -- s (1 - s) for the opacity logit,
    the scale itself for the log scale, (g - q^ (q^ . g)) / |q| for the quaternion."""
    raw, cam, kind = edge_scene(P, W, H, seed=seed, deep=deep, upstream_branches=upstream_branches, all_culled=all_culled)
    inp = hp.np_inputs(raw, cam)
    inp["shs"] = np.ascontiguousarray(inp["shs"][:, :M])
    raw_params = None
    if raw_space:
        stretch = np.random.default_rng(99 + seed).uniform(np.log(0.2), np.log(5.0), (P, 1))
        raw_params = (raw.opacity.numpy().reshape(-1), raw.scaling.numpy(),
                      (raw.rotation.numpy() / np.linalg.norm(raw.rotation.numpy(), axis=1, keepdims=True)
                       * np.exp(stretch)).astype(np.float32))
        inp["opacities"], inp["scales"], inp["rotations"] = go.activate_params(*raw_params)
    st = hp.oracle_settings(cam, antialiasing=aa, sh_degree=deg, sh_coeffs=M, scale_modifier=scale_modifier)
    bg = np.asarray(EDGE_BG, np.float32)
    rng = np.random.default_rng(7 + seed)
    dLc = rng.standard_normal((3, H, W)).astype(np.float32)
    dLd = rng.standard_normal((1, H, W)).astype(np.float32)
    colors = cov = None
    if precomp:
        f0 = hp.oracle_forward(inp, st, bg, border_eps=0.0)
        colors = rng.random((P, 3), dtype=np.float32)
        cov = f0["geom"]["cov3D"].copy()
        cov[f0["geom"]["radii"] == 0] = np.float32([1e-4, 0, 0, 1e-4, 0, 1e-4])
    fwd = hp.oracle_forward(inp, st, bg, border_eps=0.0, colors_precomp=colors, cov3D_precomp=cov)
    ref = go.backward(st, fwd, inp, bg, dLc, dLd if with_invdepth else None, colors_precomp=colors, cov3D_precomp=cov)
    ref_raw = None
    if raw_space:
        s_, sc_ = inp["opacities"].astype(np.float64).reshape(P, 1), inp["scales"].astype(np.float64)
        q = raw_params[2].astype(np.float64)
        norm = np.linalg.norm(q, axis=1, keepdims=True)
        qh, g = q / norm, ref["dL_drotations"].astype(np.float64)
        ref_raw = dict(ref, dL_dopacity=(ref["dL_dopacity"] * s_ * (1.0 - s_)).astype(np.float32),
                       dL_dscales=(ref["dL_dscales"] * sc_).astype(np.float32),
                       dL_drotations=((g - qh * (qh * g).sum(1, keepdims=True)) / norm).astype(np.float32))
    return dict(raw=raw, cam=cam, kind=kind, inp=inp, st=st, bg=bg, fwd=fwd, dLc=dLc, dLd=dLd if with_invdepth else None,
                ref=ref, visible=fwd["geom"]["radii"] > 0, colors_precomp=colors, cov3D_precomp=cov,
                raw_params=raw_params, ref_raw=ref_raw)


# (name, floats per Gaussian) in the order gsworld_amd/_backward.py lays its arena out
def _grad_layout(M, split, precomp):
    sh = [] if precomp else ([("dL_dsh_rest", 3 * (M - 1)), ("dL_dsh", 3)] if split else [("dL_dsh", 3 * M)])
    geo = [] if precomp else [("dL_drotations", 4)]
    tail = [] if precomp else [("dL_dscales", 3)]
    return sh + geo + [("dL_dcov3D", 6), ("dL_dmeans3D", 3), ("dL_dmeans2D", 3), ("dL_dcolors", 3)] + tail + [
        ("dL_dopacity", 1)]


def _carve_inputs(a, dev, misalign=0):
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.full((GUARD + misalign + a.size + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[GUARD + misalign:GUARD + misalign + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def alloc_grads(P, M, split, precomp, arrangement, sh_misalign, dev, seed=0):
    """-> ({name: (buffer, offset, floats)}, [buffers]): NaN payloads inside buffers that are SENTINEL everywhere else.
    ``arena``: one buffer in the wrapper's order, every array moved up to the next 16-byte boundary as the wrapper
    pads them -- but with ``sh_misalign`` the SH gradients start that many floats past a boundary and touch each other;
    ``scattered``: a buffer per array, allocated in a shuffled order, 64 guard floats on either side of each."""
    layout = _grad_layout(M, split, precomp)
    where = {}
    if arrangement == "arena":
        off = GUARD + sh_misalign
        for name, per in layout:
            if not (name.startswith("dL_dsh") and sh_misalign):
                off = (off + 3) // 4 * 4
            where[name] = (off, per * P)
            off += per * P
        buf = torch.full((off + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        out = {name: (buf, o, n) for name, (o, n) in where.items()}
        bufs = [buf]
    else:
        assert arrangement == "scattered"
        out, bufs = {}, []
        for j in np.random.default_rng(seed).permutation(len(layout)):
            name, per = layout[j]
            mis = sh_misalign if name.startswith("dL_dsh") else 0
            buf = torch.full((GUARD + mis + per * P + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
            out[name] = (buf, GUARD + mis, per * P)
            bufs.append(buf)
    for name, (buf, o, n) in out.items():
        buf[o:o + n] = float("nan")
        aligned = (buf.data_ptr() + 4 * o) % 16 == 0
        if name == layout[0][0] or not name.startswith("dL_dsh"):  # (the second SH array of a misaligned pair: either)
            assert aligned == (not (name.startswith("dL_dsh") and sh_misalign % 4)), name
        elif not sh_misalign:
            assert aligned, name
    return out, bufs


def gsr_backward_owned(case, dev, split=False, arrangement="arena", sh_misalign=0, param_space=0, raw_params=None,
                       seed=0):
    """The forward through ``_C.rasterize_gaussians``, then ``gsr_backward`` of the C ABI through ctypes on gradient
    buffers this function owns (:func:`alloc_grads`).  ``raw_params``: (opacity logits, log scales, un-normalised
    rotations) for ``param_space``.  -> (gradients as numpy, payload only; visible (P,) bool of THIS forward).  Asserts
    that every float outside the payloads still holds the sentinel."""
    from gsworld_amd import _C, _backward
    from gsworld_amd._lib import GsrInputs, GsrSettings, check

    inp, st = case["inp"], case["st"]
    P = inp["means3D"].shape[0]
    precomp = case["colors_precomp"] is not None
    M = 0 if precomp else inp["shs"].shape[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    empty = torch.empty(0, device=dev)
    sh = sh_rest = None
    if not precomp:
        if split:
            sh = _carve_inputs(inp["shs"][:, :1], dev, sh_misalign)
            sh_rest = _carve_inputs(inp["shs"][:, 1:], dev, sh_misalign)
        else:
            sh = _carve_inputs(inp["shs"], dev, sh_misalign)
    op, sc, ro = (inp["opacities"], inp["scales"], inp["rotations"]) if raw_params is None else raw_params
    colors = t(case["colors_precomp"]) if precomp else empty
    cov = t(case["cov3D_precomp"]) if precomp else empty
    scales, rots = (empty, empty) if precomp else (t(sc), t(ro))
    bg, means, opac = t(case["bg"]), t(inp["means3D"]), t(op).reshape(-1, 1)
    view, proj, campos = t(inp["viewmatrix"]).reshape(4, 4), t(inp["projmatrix"]).reshape(4, 4), t(inp["campos"])
    dLc = t(case["dLc"])
    dLd = None if case["dLd"] is None else t(case["dLd"])
    old = _C.NEAR_PLANE
    _C.NEAR_PLANE = st.near_plane
    try:
        R, color, radii, gB, bB, iB, invd = _C.rasterize_gaussians(
            bg, means, colors, opac, scales, rots, st.scale_modifier, cov, view, proj, st.tanfovx, st.tanfovy,
            st.image_height, st.image_width, sh if sh is not None else empty, st.sh_degree, campos, False,
            st.antialiasing, False, sh_rest=sh_rest, param_space=param_space)
    finally:
        _C.NEAR_PLANE = old
    grads, bufs = alloc_grads(P, M, split, precomp, arrangement, sh_misalign, dev, seed=seed)
    ptr = lambda x: None if x is None or x.numel() == 0 else C.c_void_p(x.data_ptr())  # noqa: E731
    gp = lambda name: C.c_void_p(grads[name][0].data_ptr() + 4 * grads[name][1]) if name in grads else None  # noqa: E731
    L = _backward._bind()
    cst = GsrSettings(st.image_height, st.image_width, float(st.tanfovx), float(st.tanfovy), float(st.scale_modifier),
                      int(st.sh_degree), int(M), 0, int(bool(st.antialiasing)), 0, float(st.near_plane))
    cin = GsrInputs(P=P, background=ptr(bg), means3D=ptr(means), shs=ptr(sh), colors_precomp=ptr(colors),
                    opacities=ptr(opac), scales=ptr(scales), rotations=ptr(rots), cov3D_precomp=ptr(cov),
                    viewmatrix=ptr(view), projmatrix=ptr(proj), campos=ptr(campos), shs_rest=ptr(sh_rest),
                    param_space=int(param_space))
    bw = _backward.GsrBackwardInputs(ptr(dLc), ptr(dLd), ptr(radii), int(R), ptr(gB), ptr(bB), ptr(iB))
    gr = _backward.GsrGrads(gp("dL_dmeans2D"), gp("dL_dcolors"), gp("dL_dopacity"), gp("dL_dmeans3D"), gp("dL_dcov3D"),
                            gp("dL_dsh"), gp("dL_dscales"), gp("dL_drotations"), None, None, gp("dL_dsh_rest"))
    with torch.cuda.device(dev):
        check(L.gsr_backward(C.byref(cst), C.byref(cin), C.byref(bw), C.byref(gr),
                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    host = {id(b): b.cpu().numpy() for b in bufs}
    outside = {k: np.ones(v.shape, bool) for k, v in host.items()}
    got = {}
    for name, (buf, o, n) in grads.items():
        got[name] = host[id(buf)][o:o + n].copy()
        outside[id(buf)][o:o + n] = False
    sentinel = np.float32(SENTINEL).view(np.uint32)
    for k, mask in outside.items():
        assert (host[k].view(np.uint32)[mask] == sentinel).all(), "a float outside the gradient arrays was overwritten"
    return got, radii.cpu().numpy() > 0, int(R), color.cpu().numpy()


WORST = {}  # case label -> (worst normalised error over its gradients, which gradient); the edges file's last test prints it


def check_owned(case, got, visible, split=False, label=None, ref=None, **tolerances):
    """What every run on caller-owned buffers must satisfy: no NaN left, exact zeros (as bits) in the rows of culled
    Gaussians and in the SH coefficients above the active degree, and everything -- those zeros included -- against the
    oracle's gradients through :func:`compare_grads`.  With ``split`` the two SH parts are compared with the oracle's
    dL_dsh[:, :1] and dL_dsh[:, 1:], each against its own scale."""
    ref = dict(case["ref"] if ref is None else ref)
    P = visible.shape[0]
    np.testing.assert_array_equal(visible, case["visible"], err_msg="radii > 0 differs from the oracle's")
    if split:
        ref["dL_dsh"], ref["dL_dsh_rest"] = ref["dL_dsh"][:, :1], ref["dL_dsh"][:, 1:]
    nb = (case["st"].sh_degree + 1) ** 2
    for name, g in got.items():
        assert not np.isnan(g).any(), f"{name}: {int(np.isnan(g).sum())} element(s) were never written"
        rows = g.reshape(P, -1).view(np.uint32)
        assert not rows[~visible].any(), f"{name}: nonzero bits in the row of a culled Gaussian"
        first = nb - 1 if name == "dL_dsh_rest" else nb if (name == "dL_dsh" and not split) else None
        if first is not None:
            assert not rows[:, 3 * first:].any(), f"{name}: nonzero bits above the active SH degree"
    rep = compare_grads(ref, got, names=tuple(got), **tolerances)
    if label is not None and rep:
        WORST[label] = max((v["max_norm_err"], k) for k, v in rep.items())
    return rep


def saturated_pixels(case):
    """Pixels whose walk the compositor ended early: the first instance behind the last contributor that would still
    contribute (power <= 0, alpha >= 1/255) takes T below 1e-4.  (final_T itself never falls below 1e-4: it is T in front
    of that instance, so with alpha <= 0.99 a pixel that ended early has 1e-4 <= final_T < 1e-2.)  Recomputed here in
    binary64 from the oracle's own geometry and lists."""
    fwd, st = case["fwd"], case["st"]
    g, b = fwd["geom"], fwd["binning"]
    W, H = st.image_width, st.image_height
    gx = (W + 15) // 16
    count = 0
    for y in range(H):
        for x in range(W):
            lo, hi = (int(v) for v in b["ranges"][(y // 16) * gx + x // 16])
            n, T = int(fwd["n_contrib"][y, x]), float(fwd["final_T"][y, x])
            if T >= 1e-2 or n >= hi - lo:
                continue
            ids = b["point_list"][lo + n:hi]
            d = g["means2D"][ids].astype(np.float64) - (x, y)
            co = g["conic_opacity"][ids].astype(np.float64)
            power = -0.5 * (co[:, 0] * d[:, 0] ** 2 + co[:, 2] * d[:, 1] ** 2) - co[:, 1] * d[:, 0] * d[:, 1]
            alpha = np.minimum(0.99, co[:, 3] * np.exp(power))
            hit = np.nonzero((power <= 0) & (alpha >= 1.0 / 255.0))[0]
            count += int(hit.size > 0 and T * (1.0 - alpha[hit[0]]) < 1e-4)
    return count
