"""Real2sim on the device: from a trained scan to the per-Gaussian labels ``merger.assign_semantic_labels`` reads.

Two steps of GSWorld's real2sim sit between training and a loadable scene, and both rest on the nearest point of one cloud
for every point of another (``gsr_nn_query``, csrc/nnquery.hip; include/gsr.h is the definition):

* alignment -- ``registration_icp``: point-to-point ICP with scaling (real2sim/scripts/icp.py:46-55, Open3D there);
* segmentation -- ``transfer_labels`` / ``transfer_labels_with_bbox`` / ``validate_labels`` / ``semantic_bounding_boxes``
  (real2sim_utils/segment_utils.py, bbox_utils.py; scipy's cKDTree and a Python loop over the points there).

All tensors are device float32 / int32; there is no CPU path.  Bindings are plain ctypes, bound on first use."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from ._lib import check, lib

LABEL_MAX_BOXES = 1024  # include/gsr.h GSR_LABEL_MAX_BOXES
ICP_WORKSPACE_BYTES = 256 * 18 * 8  # include/gsr.h GSR_ICP_WORKSPACE_BYTES


class GsrNnQuery(C.Structure):
    """The arguments of ``gsr_nn_query`` (include/gsr.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_ref", C.c_int32), ("index_mem", C.c_void_p), ("index_bytes", C.c_int64),
                ("n_query", C.c_int32), ("use_transform", C.c_int32), ("query", C.c_void_p),
                ("query_transform", C.c_float * 12), ("max_dist2", C.c_float), ("reserved", C.c_int32),
                ("index", C.c_void_p), ("dist2", C.c_void_p), ("query_out", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


class GsrLabelTransfer(C.Structure):
    """The arguments of ``gsr_label_transfer`` (include/gsr.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n", C.c_int32), ("index", C.c_void_p), ("points", C.c_void_p),
                ("ref_labels", C.c_void_p), ("n_ref", C.c_int32), ("n_boxes", C.c_int32), ("box_labels", C.c_void_p),
                ("box_bounds", C.c_void_p), ("threshold", C.c_float), ("reserved", C.c_int32), ("labels", C.c_void_p)]


class GsrIcpMoments(C.Structure):
    """The arguments of ``gsr_icp_moments`` (include/gsr.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n", C.c_int32), ("source", C.c_void_p), ("transform", C.c_float * 12),
                ("use_transform", C.c_int32), ("n_ref", C.c_int32), ("index_mem", C.c_void_p), ("index_bytes", C.c_int64),
                ("index", C.c_void_p), ("dist2", C.c_void_p), ("sums", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


def _bind():
    L = lib()
    if not getattr(L, "_real2sim_bound", False):
        L.gsr_nn_index_bytes.restype = C.c_size_t
        L.gsr_nn_index_bytes.argtypes = [C.c_int32]
        L.gsr_nn_build.restype = C.c_int
        L.gsr_nn_build.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.gsr_nn_query_workspace_bytes.restype = C.c_size_t
        L.gsr_nn_query_workspace_bytes.argtypes = [C.c_int32]
        L.gsr_nn_query.restype = C.c_int
        L.gsr_nn_query.argtypes = [C.POINTER(GsrNnQuery), C.c_void_p]
        L.gsr_label_transfer.restype = C.c_int
        L.gsr_label_transfer.argtypes = [C.POINTER(GsrLabelTransfer), C.c_void_p]
        L.gsr_icp_moments.restype = C.c_int
        L.gsr_icp_moments.argtypes = [C.POINTER(GsrIcpMoments), C.c_void_p]
        L._real2sim_bound = True
    return L


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _points(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor is required")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}; the MI355X op has no CPU path")
    if t.ndim != 2 or t.size(1) != 3:
        raise RuntimeError(f"{name} must have dimensions (num_points, 3)")
    return t.detach().to(torch.float32).contiguous()


def _transform34(transform):
    """(4,4) or (3,4), any array-like -> 12 float32 (row-major 3 x 4), rounded once from float64; None -> None."""
    if transform is None or isinstance(transform, C.c_float * 12):  # (already converted: an ICP iteration converts once)
        return transform
    if isinstance(transform, torch.Tensor):
        transform = transform.detach().cpu().numpy()
    m = np.asarray(transform, dtype=np.float64)
    if m.shape not in ((4, 4), (3, 4)):
        raise ValueError("transform must be a (4, 4) or (3, 4) matrix")
    return (C.c_float * 12)(*m[:3].astype(np.float32).reshape(-1).tolist())


class NearestIndex:
    """The search structure of a reference cloud ``points`` (n, 3), built once; ``query`` answers against it."""

    def __init__(self, points: torch.Tensor):
        pts = _points("NearestIndex: points", points)
        if pts.numel() and not bool(torch.isfinite(pts).all()):  # (the one host read of the build)
            raise ValueError("NearestIndex: points hold a non-finite value")
        L = _bind()
        self.device, self.n = pts.device, int(pts.size(0))
        self.index_bytes = int(L.gsr_nn_index_bytes(self.n))
        self.mem = torch.empty(self.index_bytes, dtype=torch.uint8, device=pts.device)
        self._ws = self._icp = None
        with torch.cuda.device(pts.device):
            check(L.gsr_nn_build(self.n, C.c_void_p(pts.data_ptr()), C.c_void_p(self.mem.data_ptr()), self.index_bytes,
                                 _stream(pts.device)))

    def _workspace(self, L, m):
        nbytes = int(L.gsr_nn_query_workspace_bytes(m))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def query_raw(self, q: torch.Tensor, transform=None, max_dist: float | None = None, out=None):
        """-> (index int32 (m), dist2 float32 (m), transformed queries float32 (m, 3)).  ``out``: optional preallocated triple."""
        qs = _points("NearestIndex.query: q", q)
        if qs.device != self.device:
            raise RuntimeError("NearestIndex.query: q is on another device than the index")
        L = _bind()
        m = int(qs.size(0))
        if out is None:
            out = (torch.empty(m, dtype=torch.int32, device=self.device), torch.empty(m, dtype=torch.float32, device=self.device),
                   torch.empty((m, 3), dtype=torch.float32, device=self.device))
        index, dist2, moved = out
        if m == 0:
            return index, dist2, moved
        ws = self._workspace(L, m)
        a = GsrNnQuery(struct_size=C.sizeof(GsrNnQuery), n_ref=self.n, index_mem=self.mem.data_ptr(),
                       index_bytes=self.index_bytes, n_query=m, query=qs.data_ptr(), index=index.data_ptr(),
                       dist2=dist2.data_ptr(), query_out=moved.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        t = _transform34(transform)
        if t is not None:
            a.use_transform, a.query_transform = 1, t
        a.max_dist2 = -1.0 if max_dist is None else float(np.float32(max_dist) * np.float32(max_dist))
        with torch.cuda.device(self.device):
            check(L.gsr_nn_query(C.byref(a), _stream(self.device)))
        return index, dist2, moved

    def query(self, q: torch.Tensor, transform=None, max_dist: float | None = None):
        """-> (index int64 (m): the nearest reference point, the lowest index on ties, or -1; dist float32 (m), inf with -1)."""
        index, dist2, _ = self.query_raw(q, transform, max_dist)
        return index.to(torch.int64), torch.sqrt(dist2)

    def moments(self, source: torch.Tensor, transform, index: torch.Tensor, dist2: torch.Tensor) -> np.ndarray:
        """The 18 binary64 sums of ``gsr_icp_moments`` over the inliers of a query of ``source`` under ``transform`` -> host."""
        src = _points("NearestIndex.moments: source", source)
        L = _bind()
        if self._icp is None:  # (the sums and the partials' workspace: allocated once, an ICP loop calls this per iteration)
            self._icp = (torch.empty(18, dtype=torch.float64, device=self.device),
                         torch.empty(ICP_WORKSPACE_BYTES, dtype=torch.uint8, device=self.device))
        sums, ws = self._icp
        a = GsrIcpMoments(struct_size=C.sizeof(GsrIcpMoments), n=int(src.size(0)), source=src.data_ptr(), n_ref=self.n,
                          index_mem=self.mem.data_ptr(), index_bytes=self.index_bytes, index=index.data_ptr(),
                          dist2=dist2.data_ptr(), sums=sums.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        t = _transform34(transform)
        if t is not None:
            a.use_transform, a.transform = 1, t
        with torch.cuda.device(self.device):
            check(L.gsr_icp_moments(C.byref(a), _stream(self.device)))
        return sums.cpu().numpy()


def _labels32(name, labels, n, dev):
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor; the MI355X op has no CPU path")
    if labels.numel() != n:
        raise RuntimeError(f"{name} must hold one label per source point")
    return labels.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()


def _nearest_in_source_frame(source_points, target_points, transformation_matrix):
    inv = np.linalg.inv(np.asarray(transformation_matrix.detach().cpu().numpy() if isinstance(transformation_matrix, torch.Tensor)
                                   else transformation_matrix, dtype=np.float64))
    nn = NearestIndex(source_points)
    return nn, nn.query_raw(target_points, transform=inv)


def transfer_labels(source_points, source_labels, target_points, transformation_matrix):
    """Every target point, brought into the source frame by ``inv(transformation_matrix)`` (float64 on the host, handed over
    as 3 x 4 float32), takes the label of its nearest source point -> (labels int32 (M), distances float32 (M))."""
    nn, (index, dist2, _) = _nearest_in_source_frame(source_points, target_points, transformation_matrix)
    lab = _labels32("transfer_labels: source_labels", source_labels, nn.n, nn.device)
    if nn.n == 0:
        return torch.full_like(index, -1), torch.sqrt(dist2)
    # (index -1 -- a non-finite target -- must not wrap to the last source label)
    return torch.where(index >= 0, lab[index.clamp_min(0).to(torch.int64)], torch.full_like(index, -1)), torch.sqrt(dist2)


def transfer_labels_with_bbox(source_points, source_labels, target_points, transformation_matrix, semantic_bboxes,
                              bbox_distance_threshold=0.1):
    """``transfer_labels`` followed by the validation against per-label boxes (``gsr_label_transfer``): ``semantic_bboxes`` is
    ``{label: (min xyz, max xyz)}``, its insertion order the row order -> (labels int32 (M), -1 = invalid; distances (M))."""
    if len(semantic_bboxes) > LABEL_MAX_BOXES:
        raise ValueError(f"transfer_labels_with_bbox: at most {LABEL_MAX_BOXES} boxes")
    nn, (index, dist2, moved) = _nearest_in_source_frame(source_points, target_points, transformation_matrix)
    dev = nn.device
    lab = _labels32("transfer_labels_with_bbox: source_labels", source_labels, nn.n, dev)
    rows = [(int(k), np.asarray(torch.as_tensor(lo).cpu(), np.float64).reshape(3), np.asarray(torch.as_tensor(hi).cpu(), np.float64).reshape(3))
            for k, (lo, hi) in semantic_bboxes.items()]
    box_labels = torch.tensor([r[0] for r in rows], dtype=torch.int32, device=dev)
    box_bounds = torch.tensor(np.array([np.concatenate(r[1:]) for r in rows], np.float64).reshape(-1, 6), dtype=torch.float32,
                              device=dev)
    out = torch.empty_like(index)
    a = GsrLabelTransfer(struct_size=C.sizeof(GsrLabelTransfer), n=int(index.numel()), index=index.data_ptr(),
                         points=moved.data_ptr(), ref_labels=lab.data_ptr(), n_ref=nn.n, n_boxes=len(rows),
                         box_labels=box_labels.data_ptr(), box_bounds=box_bounds.data_ptr(),
                         threshold=float(bbox_distance_threshold), labels=out.data_ptr())
    with torch.cuda.device(dev):
        check(_bind().gsr_label_transfer(C.byref(a), _stream(dev)))
    return out, torch.sqrt(dist2)


def validate_labels(distances, threshold=0.1):
    """Boolean mask of the reliable labels: nearest-neighbour distance within ``threshold``."""
    return distances <= threshold


def semantic_bounding_boxes(vertices: torch.Tensor, labels: torch.Tensor) -> dict:
    """Per-label AABBs of labelled vertices -> ``{label: (min (3,) float32 tensor, max (3,))}``, labels ascending (the order
    ``np.unique`` gives the reference's ``get_semantic_bounding_boxes``)."""
    v = _points("semantic_bounding_boxes: vertices", vertices)
    lab = labels.detach().reshape(-1).to(device=v.device, dtype=torch.int64)
    if lab.numel() != v.size(0):
        raise RuntimeError("semantic_bounding_boxes: one label per vertex")
    uniq, inv = torch.unique(lab, return_inverse=True)
    idx = inv[:, None].expand(-1, 3)
    lo = torch.full((uniq.numel(), 3), float("inf"), device=v.device).scatter_reduce(0, idx, v, "amin")
    hi = torch.full((uniq.numel(), 3), float("-inf"), device=v.device).scatter_reduce(0, idx, v, "amax")
    return {int(k): (lo[i], hi[i]) for i, k in enumerate(uniq.tolist())}


IcpResult = namedtuple("IcpResult", "transformation fitness inlier_rmse num_correspondences iterations")


def umeyama_from_moments(s: np.ndarray, with_scaling: bool = True) -> np.ndarray:
    """The similarity (4, 4) float64 that maps the p' onto the q in the least-squares sense, from the 18 sums of
    ``gsr_icp_moments`` (Umeyama 1991: SVD of the cross-covariance, reflection guard, scale = tr(D S) / var(p'))."""
    n = s[0]
    mp, mq = s[1:4] / n, s[4:7] / n
    cov = (s[7:16].reshape(3, 3) / n - np.outer(mp, mq)).T  # E[(q - mq)(p - mp)^T]
    var_p = s[16] / n - mp @ mp
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    scale = float((D * S).sum() / var_p) if with_scaling and var_p > 0 else 1.0
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = mq - scale * R @ mp
    return T


def registration_icp(source, target, max_correspondence_distance, init=None, with_scaling=True, max_iteration=30,
                     relative_fitness=1e-6, relative_rmse=1e-6) -> IcpResult:
    """Point-to-point ICP of ``source`` (m, 3) onto ``target`` (n, 3), optionally with scaling.  Per iteration: one query of
    the sources under the current transform within ``max_correspondence_distance``, one ``gsr_icp_moments``, one 18-double
    host read, the Umeyama solve in float64, T <- dT T.  Stops when fitness and RMSE both change by less than their
    thresholds, at ``max_iteration``, or with fewer than three inliers (the transform so far is returned)."""
    src = _points("registration_icp: source", source)
    nn = NearestIndex(target)
    if src.device != nn.device:
        raise RuntimeError("registration_icp: source and target are on different devices")
    m = int(src.size(0))
    T = np.eye(4) if init is None else np.array(init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else init,
                                                dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("registration_icp: init must be a (4, 4) matrix")
    out = None
    fitness = rmse = 0.0
    count = iterations = 0
    prev = None
    for it in range(int(max_iteration) + 1):
        t34 = _transform34(T)
        out = nn.query_raw(src, transform=t34, max_dist=max_correspondence_distance, out=out)
        s = nn.moments(src, t34, out[0], out[1])
        count = int(s[0])
        fitness = count / m if m else 0.0
        rmse = float(np.sqrt(s[17] / count)) if count else 0.0
        if count < 3 or it == int(max_iteration):
            break
        if prev is not None and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
        prev = (fitness, rmse)
        T = umeyama_from_moments(s, with_scaling) @ T
        iterations += 1
    return IcpResult(T, fitness, rmse, count, iterations)
