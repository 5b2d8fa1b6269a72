"""Point-cloud observations (include/gsr.h gsr_render_pointcloud, csrc/pointcloud.hip) without a GPU: a NumPy restatement
of the definition -- unprojection, crop, exclusion, stride ranks and farthest-point sampling, in the kernel's binary32 order
-- with known-answer tests, the simulator-frame helper, the exported symbols and the argument checks.  The GPU suite
(tests/test_pointcloud_gpu.py) holds the kernels to this restatement bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

F32 = np.float32


def c2w(m) -> np.ndarray:
    """The (3,4) float32 camera-to-world matrix of a 16-float view matrix (W2C^T as 3DGS stores it, W2C[r][k] = m[4k + r]):
    the binary64 formula of csrc/pointcloud.hip's header comment, rounded to binary32."""
    m = [float(x) for x in np.asarray(m, F32).reshape(-1)]
    a00, a01, a02 = m[0], m[4], m[8]
    a10, a11, a12 = m[1], m[5], m[9]
    a20, a21, a22 = m[2], m[6], m[10]
    t0, t1, t2 = m[12], m[13], m[14]
    c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
    det = (a00 * c00 + a01 * c01) + a02 * c02
    r = [[c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det],
         [c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det],
         [c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det]]
    out = np.zeros((3, 4), F32)
    for i in range(3):
        out[i, :3] = [F32(x) for x in r[i]]
        out[i, 3] = F32(-((r[i][0] * t0 + r[i][1] * t1) + r[i][2] * t2))
    return out


def _affine(M, x, y, z):
    return [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)]


def unproject(D, viewmatrix, tanfovx, tanfovy, depth_scale=1.0, A=None):
    """(H,W) depth map -> (q (H*W,3) float32, is-a-point (H*W,) bool), row-major by pixel."""
    D = np.asarray(D, F32)
    H, W = D.shape
    y, x = np.mgrid[0:H, 0:W]
    z = D / F32(depth_scale)
    ndx = (2 * x + 1).astype(F32) / F32(W) - F32(1.0)
    ndy = (2 * y + 1).astype(F32) / F32(H) - F32(1.0)
    xv, yv, zv = (ndx * F32(tanfovx)) * z, (ndy * F32(tanfovy)) * z, z
    p = _affine(c2w(viewmatrix), xv, yv, zv)
    A = np.eye(3, 4, dtype=F32) if A is None else np.asarray(A, F32).reshape(-1)[:12].reshape(3, 4)
    q = _affine(A, *p)
    return np.stack([c.reshape(-1) for c in q], axis=1).astype(F32), (D > 0).reshape(-1)


def stride_ranks(n: int, M: int) -> np.ndarray:
    """Slot j < M holds the valid point of rank floor(j n / M) (64-bit integers)."""
    return (np.arange(M, dtype=np.int64) * np.int64(n)) // np.int64(max(M, 1))


def fps(P, K: int) -> np.ndarray:
    """Farthest-point sampling of the (M,3) float32 points from index 0: min(M, K) indices in pick order."""
    P = np.asarray(P, F32)
    M = P.shape[0]
    n = min(M, K)
    if n == 0:
        return np.zeros(0, np.int64)
    picks = [0]
    dmin = np.full(M, np.inf, F32)
    s = P[0]
    for _ in range(1, n):
        dx, dy, dz = P[:, 0] - s[0], P[:, 1] - s[1], P[:, 2] - s[2]
        d = ((dx * dx) + (dy * dy)) + dz * dz
        dmin = np.where(d < dmin, d, dmin)
        i = int(np.argmax(dmin))  # (the first of equal maxima: ties to the lowest index)
        picks.append(i)
        s = P[i]
    return np.asarray(picks, np.int64)


def restate_pointcloud(views, mode="dense", K=0, fps_candidates=8192, A=None, crop=None, exclude=(), depth_scale=1.0):
    """The cloud of ONE environment.  ``views``: per camera dicts with ``depth`` (H,W), ``label`` (H,W) int16 or None,
    ``rgb`` (H,W,3) uint8 or None, ``viewmatrix`` (16,), ``tanfovx`` / ``tanfovy`` (the float32 values the frames used).
    -> (xyzw (S,4) float32, rgb (S,3) uint8, segmentation (S,) int16, count, picked pixel indices)."""
    qs, ok, labs, cols = [], [], [], []
    for v in views:
        q, pt = unproject(v["depth"], v["viewmatrix"], v["tanfovx"], v["tanfovy"], depth_scale, A)
        n = q.shape[0]
        lab = np.asarray(v["label"], np.int16).reshape(-1) if v.get("label") is not None else np.full(n, -1, np.int16)
        col = np.asarray(v["rgb"], np.uint8).reshape(-1, 3) if v.get("rgb") is not None else np.zeros((n, 3), np.uint8)
        if crop is not None:
            lo, hi = np.asarray(crop[0], F32), np.asarray(crop[1], F32)
            pt = pt & np.all((q >= lo) & (q <= hi), axis=1)
        if len(exclude):
            pt = pt & ~np.isin(lab, np.asarray(exclude, np.int16))
        qs.append(q)
        ok.append(pt)
        labs.append(lab)
        cols.append(col)
    q, ok, lab, col = np.concatenate(qs), np.concatenate(ok), np.concatenate(labs), np.concatenate(cols)
    idx = np.flatnonzero(ok)
    n = idx.size
    if mode == "dense":
        sel, S = np.arange(q.shape[0]), q.shape[0]
        keep = ok
        count = n
    else:
        M = min(n, K if mode == "stride" else fps_candidates)
        cand = idx[stride_ranks(n, M)]
        sel = cand if mode == "stride" else cand[fps(q[cand], K)]
        S = K
        count = sel.size
        keep = np.ones(sel.size, bool)
    xyzw = np.zeros((S, 4), F32)
    rgb = np.zeros((S, 3), np.uint8)
    seg = np.full(S, -1, np.int16)
    k = sel.size
    xyzw[:k, :3] = np.where(keep[:, None], q[sel], F32(0))
    xyzw[:k, 3] = np.where(keep, F32(1), F32(0))
    rgb[:k] = np.where(keep[:, None], col[sel], 0)
    seg[:k] = np.where(keep, lab[sel], -1)
    return xyzw, rgb, seg, count, sel


def _identity_vm():
    return np.eye(4, dtype=F32).reshape(-1)


# ---- known answers of the restatement -----------------------------------------------------------------------------------
def test_pixel_on_the_optical_axis_unprojects_to_the_axis():
    D = np.zeros((5, 7), F32)
    D[2, 3] = 3.0
    q, ok = unproject(D, _identity_vm(), 0.7, 0.4)
    assert ok.sum() == 1
    assert q[2 * 7 + 3].tolist() == [0.0, 0.0, 3.0]
    # a translated camera: the same pixel sits on the axis through the camera centre (W2C t = -centre for R = I)
    vm = np.eye(4, dtype=F32)
    vm[3, :3] = [-1.0, 2.0, -0.5]
    q, _ = unproject(D, vm.reshape(-1), 0.7, 0.4, depth_scale=2.0)
    assert q[2 * 7 + 3].tolist() == [1.0, -2.0, 2.0]


def test_c2w_inverts_the_view_matrix():
    rng = np.random.default_rng(0)
    a = rng.normal(size=3)
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx
    W2C = np.eye(4)
    W2C[:3, :3], W2C[:3, 3] = R, [0.3, -1.2, 2.0]
    m = W2C.T.astype(F32).reshape(-1)
    M = c2w(m).astype(np.float64)
    back = np.vstack([M, [0, 0, 0, 1]]) @ W2C.astype(F32).astype(np.float64)
    assert np.abs(back - np.eye(4)).max() < 1e-6


def test_fps_takes_the_two_ends_of_collinear_points_first():
    P = np.zeros((6, 3), F32)
    P[:, 0] = [0.0, 0.3, 0.45, 1.0, 0.6, 0.8]
    order = fps(P, 6)
    assert order[:2].tolist() == [0, 3]
    assert sorted(order.tolist()) == list(range(6))


def test_fps_ties_go_to_the_lowest_index():
    P = np.zeros((5, 3), F32)
    P[:, 1] = [0.0, 2.0, -1.0, -2.0, 1.0]
    assert fps(P, 2).tolist() == [0, 1]  # (1 and 3 are both 2 away)
    P = np.zeros((4, 3), F32)  # (all equal: every distance 0, every pick the lowest index)
    assert fps(P, 4).tolist() == [0, 0, 0, 0]


def test_fewer_points_than_slots_leave_empty_slots():
    D = np.zeros((4, 4), F32)
    D[0, 1], D[2, 2], D[3, 0] = 1.0, 2.0, 3.0
    lab = np.arange(16, dtype=np.int16).reshape(4, 4)
    v = dict(depth=D, label=lab, rgb=None, viewmatrix=_identity_vm(), tanfovx=0.5, tanfovy=0.5)
    for mode in ("stride", "fps"):
        xyzw, rgb, seg, count, _ = restate_pointcloud([v], mode, K=8, fps_candidates=16)
        assert count == 3
        assert (xyzw[:3, 3] == 1).all() and (xyzw[3:] == 0).all()
        assert (seg[3:] == -1).all() and sorted(seg[:3].tolist()) == [1, 10, 12]
        assert (rgb == 0).all()
    xyzw, _, seg, count, _ = restate_pointcloud([v], "dense")
    assert count == 3 and xyzw.shape == (16, 4) and int((xyzw[:, 3] == 1).sum()) == 3
    assert seg[1] == 1 and seg[0] == -1


def test_stride_ranks():
    assert stride_ranks(7, 7).tolist() == list(range(7))
    r = stride_ranks(1_000_003, 1024)
    assert r[0] == 0 and r[-1] == (1023 * 1_000_003) // 1024 and (np.diff(r) >= 976).all()
    # beyond 32 bits: j n overflows int32, the ranks must not
    r = stride_ranks(16_000_000, 8192)
    assert r[-1] == (8191 * 16_000_000) // 8192


def test_crop_and_exclusion():
    D = np.full((3, 3), 2.0, F32)
    lab = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int16)
    v = dict(depth=D, label=lab, rgb=None, viewmatrix=_identity_vm(), tanfovx=1.0, tanfovy=1.0)
    # x of the columns: -4/3, 0, 4/3 (ndc -2/3, 0, 2/3 at z = 2); keep x >= -0.1 and drop labels 4 and 8
    xyzw, _, seg, count, _ = restate_pointcloud([v], "dense", crop=((-0.1, -9, -9), (9, 9, 9)), exclude=(4, 8))
    assert count == 4
    assert sorted(seg[seg >= 0].tolist()) == [1, 2, 5, 7]


# ---- the simulator frame ----------------------------------------------------------------------------------------------
def test_sim_from_scene_inverts_cam_maniskill2gs_chain():
    from gsworld_amd.camera import cam_maniskill2gs
    from gsworld_amd.pointcloud import sim_from_scene

    th = 0.7
    rigid = np.eye(4)
    rigid[:3, :3] = [[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]]
    rigid[:3, :3] = rigid[:3, :3] @ np.array([[1.0, 0.0, 0.0], [0.0, math.cos(0.3), -math.sin(0.3)],
                                               [0.0, math.sin(0.3), math.cos(0.3)]])
    rigid[:3, 3] = [0.12, -0.4, 0.05]
    s = 1.37
    A = sim_from_scene(torch.tensor(rigid), s)
    assert A.shape == (3, 4) and A.dtype == np.float64
    X = np.random.default_rng(1).normal(size=(20, 3))
    scene = (rigid @ np.c_[s * X, np.ones(20)].T).T  # (a simulator point as the chain places it in the scene)
    back = (A @ scene.T).T
    assert np.abs(back - X).max() < 1e-12
    # the chain itself: a simulator camera placed by cam_maniskill2gs has its centre where sim_from_scene says
    ext = np.eye(4)
    ext[:3, :3] = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    ext[:3, 3] = [0.2, 0.3, 0.6]
    K = torch.tensor([[300.0, 0.0, 64.0], [0.0, 300.0, 48.0], [0.0, 0.0, 1.0]])
    cam = cam_maniskill2gs(torch.tensor(ext[:3], dtype=torch.float32), K, 128, 96, torch.tensor(rigid, dtype=torch.float32), s)
    sim_centre = np.linalg.inv(ext)[:3, 3]
    c = cam.camera_center.double().numpy()
    assert np.abs(A[:, :3] @ c + A[:, 3] - sim_centre).max() < 1e-5


# ---- the library's symbols and checks ---------------------------------------------------------------------------------
def test_render_pointcloud_is_exported_and_checks_its_struct_size():
    from gsworld_amd import _lib

    L = _lib.lib()
    for name in ("gsr_render_pointcloud", "gsr_pointcloud_workspace"):
        assert hasattr(L, name) and name in _lib.exported_symbols()
    s = _lib.GsrCloudSpec()
    s.struct_size = C.sizeof(_lib.GsrCloudSpec) + 8
    assert L.gsr_render_pointcloud(C.byref(s), None) == _lib.GSR_E_INVALID
    assert b"struct_size" in L.gsr_last_error()
    n = C.c_int64(-1)
    assert L.gsr_pointcloud_workspace(C.byref(s), C.byref(n)) == _lib.GSR_E_INVALID and n.value == -1
    # the ctypes mirror has the library's size: the next check (no views) is what refuses the spec now
    s.struct_size = C.sizeof(_lib.GsrCloudSpec)
    assert L.gsr_render_pointcloud(C.byref(s), None) == _lib.GSR_E_INVALID
    assert b"view array" in L.gsr_last_error()


def test_workspace_and_limits():
    from gsworld_amd import _lib

    L = _lib.lib()

    def spec(E, Cn, W=64, H=48, mode=_lib.PC_FPS, K=1024, M=8192):
        views = (_lib.GsrCloudView * (E * Cn))(*[_lib.GsrCloudView(W, H) for _ in range(E * Cn)])
        s = _lib.GsrCloudSpec()
        s.struct_size = C.sizeof(_lib.GsrCloudSpec)
        s.E, s.C, s.views, s.mode, s.K, s.fps_candidates = E, Cn, views, mode, K, M
        return s, views

    n = C.c_int64(0)
    s, keep = spec(2, 2)
    assert L.gsr_pointcloud_workspace(C.byref(s), C.byref(n)) == _lib.GSR_OK
    assert n.value >= 2 * 2 * 12 * 4 + 2 * 8192 * 18  # (per-workgroup counts + the FPS candidates)
    for bad in (dict(E=0, Cn=1), dict(E=33, Cn=2), dict(E=1, Cn=1, K=0), dict(E=1, Cn=1, K=8193),
                dict(E=1, Cn=1, M=16385), dict(E=1, Cn=1, mode=3), dict(E=1, Cn=1, W=0)):
        s, keep = spec(**bad)
        assert L.gsr_pointcloud_workspace(C.byref(s), C.byref(n)) == _lib.GSR_E_INVALID, bad
    s, keep = spec(1, 1, mode=_lib.PC_DENSE, K=0, M=0)  # (K and fps_candidates mean nothing to a dense cloud)
    assert L.gsr_pointcloud_workspace(C.byref(s), C.byref(n)) == _lib.GSR_OK


def test_bad_specs_raise_value_error():
    from gsworld_amd.pointcloud import PointCloudSpec

    PointCloudSpec().validated()
    PointCloudSpec(num_points=1024, sample="stride", crop=((0, 0, 0), (1, 1, 1)), exclude_labels=(-1, 3),
                   out_from_scene=np.eye(4)).validated()
    for bad in (dict(num_points=0), dict(num_points=8193), dict(num_points=1.5), dict(num_points=64, sample="random"),
                dict(num_points=64, fps_candidates=0), dict(num_points=64, fps_candidates=16385),
                dict(crop=((0, 0), (1, 1))), dict(crop=((0, 0, 0),)), dict(crop=((0, 0, float("nan")), (1, 1, 1))),
                dict(exclude_labels=(40000,)), dict(exclude_labels=(1.5,)), dict(out_from_scene=np.eye(3)),
                dict(out_from_scene=np.full((3, 4), np.inf))):
        with pytest.raises(ValueError):
            PointCloudSpec(**bad).validated()
    bits = PointCloudSpec(exclude_labels=(0, 33, -1)).exclusion_bitmap()
    assert bits[0] == 1 and bits[1] == 2 and bits[2047] == 1 << 31 and int(np.count_nonzero(bits)) == 3


def test_loops_refuse_bad_point_cloud_arguments():
    from gsworld_amd.closed_loop import ClosedLoopRenderer, PipelinedClosedLoop
    from gsworld_amd.pointcloud import PointCloudSpec

    with pytest.raises(ValueError, match="ClosedLoopRenderer"):
        PipelinedClosedLoop(None, {}, {}, pointcloud=PointCloudSpec())
    with pytest.raises(ValueError):
        ClosedLoopRenderer(None, {}, {}, pointcloud=PointCloudSpec(num_points=0))
    with pytest.raises(ValueError):
        ClosedLoopRenderer(None, {}, {}, pointcloud="fps")
    with pytest.raises(ValueError):
        ClosedLoopRenderer(None, {}, {"a": None, "b": None}, num_envs=33, pointcloud=PointCloudSpec())
