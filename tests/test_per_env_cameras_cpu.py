"""Per-environment cameras and the on-device camera conversion (include/gsr.h ``gsr_cameras_from_extrinsics``), on the CPU.

``restate_records`` is the NumPy statement of csrc/camera.hip's header comment (binary64 in the written order, one
rounding per output); tests/test_per_env_cameras_gpu.py holds the kernel to it bit for bit.  Here it is held to the
reference's own cameras (tests/golden/wrapper_glue.npz: the R / T / FoV ``cam_maniskill2gs`` handed to ``Camera``).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gsworld_amd import camera as gcam

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "wrapper_glue.npz")
CAMS = ("right_cam", "wrist_cam")


def _inv3(a):
    """gsr_internal.h gsr_inverse3_f64 (binary64, same order)."""
    c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1]
    c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2]
    c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0]
    det = (a[0][0] * c00 + a[0][1] * c01) + a[0][2] * c02
    return [[c00 / det, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det],
            [c01 / det, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det],
            [c02 / det, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det]]


def restate_record(ext, proj, rigid, scale) -> np.ndarray:
    """One 36-float record from a (3,4) float32 extrinsic, the (4,4) float32 projection^T, rigid (4,4) and scale."""
    E = [[float(x) for x in row] for row in np.asarray(ext, np.float32).reshape(3, 4)]
    G = [float(x) for x in np.asarray(rigid, np.float64).reshape(-1)]
    s = float(scale)
    Q = [float(x) for x in np.asarray(proj, np.float32).reshape(-1)]
    A = [row[:3] for row in E]
    t = [row[3] for row in E]
    Ai = _inv3(A)
    p = [-((Ai[i][0] * t[0] + Ai[i][1] * t[1]) + Ai[i][2] * t[2]) * s for i in range(3)]
    Rr = [[(G[4 * i] * Ai[0][j] + G[4 * i + 1] * Ai[1][j]) + G[4 * i + 2] * Ai[2][j] for j in range(3)] for i in range(3)]
    pr = [((G[4 * i] * p[0] + G[4 * i + 1] * p[1]) + G[4 * i + 2] * p[2]) + G[4 * i + 3] for i in range(3)]
    Rw = _inv3(Rr)
    v = np.zeros(16, np.float32)
    for c in range(3):
        for r in range(3):
            v[4 * r + c] = np.float32(Rw[c][r])
        v[12 + c] = np.float32(-((Rw[c][0] * pr[0] + Rw[c][1] * pr[1]) + Rw[c][2] * pr[2]))
    v[15] = 1.0
    vd = [float(x) for x in v]
    out = np.zeros(36, np.float32)
    out[:16] = v
    for r in range(4):
        for c in range(4):
            out[16 + 4 * r + c] = np.float32(((vd[4 * r] * Q[c] + vd[4 * r + 1] * Q[4 + c]) + vd[4 * r + 2] * Q[8 + c]) +
                                             vd[4 * r + 3] * Q[12 + c])
    out[32:35] = np.asarray(pr, np.float64).astype(np.float32)
    return out


def restate_records(ext, fovs, rigid, scale) -> np.ndarray:
    """(n,3,4) extrinsics, n (FoVx, FoVy) -> (n, 36) records."""
    ext = np.asarray(ext, np.float32).reshape(-1, 3, 4)
    return np.stack([restate_record(ext[k], gcam.sensor_projection(*fovs[k]).numpy(), rigid, scale)
                     for k in range(ext.shape[0])])


def random_extrinsics(rng, n):
    """n rigid OpenCV world->camera (3,4) float32 matrices (cameras within a metre or two of the origin)."""
    out = np.zeros((n, 3, 4), np.float32)
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[k, :, :3] = q
        out[k, :, 3] = rng.uniform(-1.5, 1.5, 3)
    return out


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _reference_camera(z, E, cam):
    size = z[f"E{E}.cam.{cam}.size"]
    fov = z[f"E{E}.cam.{cam}.fov"]
    return gcam.view_params(z[f"E{E}.cam.{cam}.R"], z[f"E{E}.cam.{cam}.T"], float(fov[0]), float(fov[1]), int(size[0]),
                            int(size[1]))


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("cam", CAMS)
def test_restatement_matches_the_reference_cameras(z, E, cam):
    want = _reference_camera(z, E, cam)
    rec = restate_record(z[f"E{E}.cam.{cam}.extrinsic_cv"], gcam.sensor_projection(want.FoVx, want.FoVy).numpy(),
                         z["rigid_sim2real"], z["scale_sim2real"])
    np.testing.assert_allclose(rec[:16], want.world_view_transform.numpy().reshape(-1), rtol=0, atol=5e-7)
    np.testing.assert_allclose(rec[16:32], want.full_proj_transform.numpy().reshape(-1), rtol=0, atol=5e-7)
    np.testing.assert_allclose(rec[32:35], want.camera_center.numpy(), rtol=0, atol=5e-7)
    assert rec[35] == 0.0


def test_known_answers():
    proj = gcam.sensor_projection(1.0, 0.8).numpy()
    ext = np.zeros((3, 4), np.float32)
    ext[:, :3] = np.eye(3)
    rec = restate_record(ext, proj, np.eye(4), 1.0)
    assert np.array_equal(rec[:16], np.eye(4, dtype=np.float32).reshape(-1))
    assert np.array_equal(rec[16:32], proj.reshape(-1))
    assert np.array_equal(rec[32:35], np.zeros(3, np.float32))
    # a pure translation: world->camera x -> x + t puts the camera at -t, scaled by s and moved by the rigid offset
    ext[:, 3] = (0.5, -0.25, 2.0)
    rig = np.eye(4)
    rig[:3, 3] = (1.0, 2.0, 3.0)
    rec = restate_record(ext, proj, rig, 2.0)
    centre = np.array([-1.0 + 1.0, 0.5 + 2.0, -4.0 + 3.0])
    assert np.array_equal(rec[32:35], centre.astype(np.float32))
    wv = rec[:16].reshape(4, 4)
    assert np.array_equal(wv[:3, :3], np.eye(3, dtype=np.float32)) and np.array_equal(wv[3, :3], -centre.astype(np.float32))


def test_cameras_from_sensor_params_env0_is_todays_conversion(z):
    rng = np.random.default_rng(3)
    E = 3
    params, sizes = {}, {}
    for cam in CAMS:
        ext0 = z[f"E3.cam.{cam}.extrinsic_cv"]
        ext = np.stack([ext0] + [ext0 + rng.normal(scale=0.01, size=ext0.shape).astype(np.float32) * [[0, 0, 0, 1]]
                                 for _ in range(E - 1)]).astype(np.float32)
        K = np.stack([z["intrinsic_k"]] * E)
        K[2, 0, 0] *= 1.05  # (FoV noise in environment 2)
        params[cam] = {"extrinsic_cv": torch.from_numpy(ext), "intrinsic_cv": torch.from_numpy(K)}
        sizes[cam] = tuple(int(x) for x in z[f"E3.cam.{cam}.size"])
    got = gcam.cameras_from_sensor_params(params, sizes, torch.from_numpy(z["rigid_sim2real"]),
                                          torch.from_numpy(z["scale_sim2real"]))
    for cam in CAMS:
        assert len(got[cam]) == E
        today = gcam.cam_maniskill2gs(torch.from_numpy(z[f"E3.cam.{cam}.extrinsic_cv"]), torch.from_numpy(z["intrinsic_k"]),
                                      *sizes[cam], torch.from_numpy(z["rigid_sim2real"]), torch.from_numpy(z["scale_sim2real"]))
        g0 = got[cam][0]
        assert (g0.FoVx, g0.FoVy) == (today.FoVx, today.FoVy)
        for a in ("world_view_transform", "full_proj_transform", "camera_center"):
            assert torch.equal(getattr(g0, a), getattr(today, a)), a
        assert not torch.equal(got[cam][1].world_view_transform, g0.world_view_transform)
        assert got[cam][2].FoVx != g0.FoVx


def test_symbol_is_exported_and_struct_size_is_checked():
    from gsworld_amd import _lib

    assert "gsr_cameras_from_extrinsics" in _lib.exported_symbols()
    L = _lib.lib()
    cs = _lib.GsrSensorCameras()
    cs.n = 1
    cs.scale_sim2real = 1.0
    cs.extrinsic = cs.projection = cs.out = 256  # (never dereferenced: every call below is refused first)
    for size in (C.sizeof(cs) - 8, C.sizeof(cs) + 8, 0):
        cs.struct_size = size
        assert L.gsr_cameras_from_extrinsics(C.byref(cs), None) == _lib.GSR_E_INVALID
    cs.struct_size = C.sizeof(cs)
    for n in (0, -1, _lib.CAM_MAX_VIEWS + 1):
        cs.n = n
        assert L.gsr_cameras_from_extrinsics(C.byref(cs), None) == _lib.GSR_E_INVALID
    cs.n = 1
    for s in (0.0, float("nan"), float("inf")):
        cs.scale_sim2real = s
        assert L.gsr_cameras_from_extrinsics(C.byref(cs), None) == _lib.GSR_E_INVALID
    cs.scale_sim2real = 1.0
    cs.out = None
    assert L.gsr_cameras_from_extrinsics(C.byref(cs), None) == _lib.GSR_E_INVALID
    assert L.gsr_cameras_from_extrinsics(None, None) == _lib.GSR_E_INVALID


def test_loops_refuse_bad_camera_arguments():
    from gsworld_amd.closed_loop import ClosedLoopRenderer, PipelinedClosedLoop, check_extrinsics

    a = gcam.look_at_view([0, 0, -3], [0, 0, 0], [0, -1, 0], 1.0, 0.8, 64, 48)
    b = gcam.look_at_view([0, 0, -3], [0, 0, 0], [0, -1, 0], 1.0, 0.8, 32, 48)
    for Loop in (ClosedLoopRenderer, PipelinedClosedLoop):
        with pytest.raises(ValueError):  # wrong list length
            Loop(None, {}, {"c": [a, a]}, num_envs=3, per_env_cameras=True)
        with pytest.raises(ValueError):  # mixed image sizes
            Loop(None, {}, {"c": [a, b, a]}, num_envs=3, per_env_cameras=True)
        with pytest.raises(ValueError):  # a list without per_env_cameras
            Loop(None, {}, {"c": [a, a, a]}, num_envs=3)
        for bad in ((np.eye(3), 1.0), (np.eye(4), 0.0), (np.eye(4),), np.eye(4)):
            with pytest.raises(ValueError):
                Loop(None, {}, {"c": a}, sim2real=bad)
    ok = torch.zeros(3, 3, 4)
    assert tuple(check_extrinsics("c", ok, 3, True, True).shape) == (3, 3, 4)
    assert tuple(check_extrinsics("c", torch.zeros(3, 4), 3, False, True).shape) == (1, 3, 4)
    assert tuple(check_extrinsics("c", np.zeros((1, 3, 4)), 3, False, True).shape) == (1, 3, 4)
    for shape, per_env in (((3, 4), True), ((2, 3, 4), True), ((3, 3, 4), False), ((4, 4), False), ((3, 3), True)):
        with pytest.raises(ValueError):
            check_extrinsics("c", torch.zeros(shape), 3, per_env, True)
    with pytest.raises(ValueError, match="sim2real"):
        check_extrinsics("c", ok, 3, True, False)
