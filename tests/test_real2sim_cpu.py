"""Real2sim without a device: known answers for the float64 restatement (tests/ref_real2sim.py), the conditions the GPU tests
rely on -- asserted on exactly the inputs those tests use --, and the argument checks of the new C ABI entries."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gsworld_amd import _lib, real2sim
from tests import ref_real2sim as rr


# ---- the restatement itself ------------------------------------------------------------------------------------------------
def test_box_distance_known_answers():
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 2.0, 3.0])
    d = rr.point_to_bbox_distance
    assert d(np.array([0.5, 1.0, 1.5]), lo, hi) == 0.0                       # inside
    assert d(np.array([1.0, 2.0, 3.0]), lo, hi) == 0.0                       # on a corner
    assert d(np.array([1.25, 1.0, 1.0]), lo, hi) == 0.25                     # off a face
    assert d(np.array([-3.0, -4.0, 1.0]), lo, hi) == 5.0                     # off an edge
    assert d(np.array([3.0, 5.0, 9.0]), lo, hi) == 7.0                       # off a corner: (2, 3, 6)
    pts = np.array([[0.5, 1.0, 1.5], [1.25, 1.0, 1.0], [-3.0, -4.0, 1.0], [3.0, 5.0, 9.0]])
    assert rr.box_distances(pts, {4: (lo, hi)})[:, 0].tolist() == [0.0, 0.25, 5.0, 7.0]


def test_label_outcomes_on_a_hand_made_case():
    boxes = {3: (np.zeros(3), np.ones(3)), 5: (np.array([2.0, 0, 0]), np.array([3.0, 1, 1])),
             8: (np.array([2.0, 0, 0]), np.array([3.0, 1, 1]))}
    pts = np.array([[0.5, 0.5, 0.5],    # label 3, inside its box: kept
                    [1.05, 0.5, 0.5],   # label 3, 0.05 off its box: kept (within the threshold)
                    [2.5, 0.5, 0.5],    # label 3, far from its box, inside 5 and 8: the FIRST row wins the tie
                    [1.5, 0.5, 0.5],    # label 3, 0.5 from every box: invalid
                    [0.5, 0.5, 0.5],    # source unlabelled
                    [0.5, 0.5, 0.5],    # label 9 has no box
                    [1.92, 0.5, 0.5]])  # label 3, 0.92 off its own box, 0.08 off box 5: relabelled
    labels, outcome = rr.validate_with_bbox(pts, [3, 3, 3, 3, -1, 9, 3], boxes, 0.1)
    assert labels.tolist() == [3, 3, 5, -1, -1, -1, 5]
    assert outcome.tolist() == [rr.KEPT, rr.KEPT, rr.RELABELLED, rr.INVALIDATED, rr.SOURCE_UNLABELLED, rr.NO_BOX, rr.RELABELLED]


def test_umeyama_recovers_a_similarity_from_exact_correspondences():
    rng = np.random.default_rng(3)
    p = rng.normal(0, 1, (50, 3))
    for with_scaling, scale in ((True, 1.7), (False, 1.0)):
        T = rr.similarity(scale, 0.9, (0.3, -2.0, 0.7))
        T[:3, :3] = T[:3, :3] @ np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
        assert np.abs(rr.umeyama(p, rr.apply_transform(T, p), with_scaling) - T).max() < 1e-12
        # the device route solves from the 18 sums: the same answer
        q = rr.apply_transform(T, p)
        s = np.concatenate([[len(p)], p.sum(0), q.sum(0), (p[:, :, None] * q[:, None, :]).sum(0).reshape(-1),
                            [(p * p).sum()], [0.0]])
        assert np.abs(real2sim.umeyama_from_moments(s, with_scaling) - T).max() < 1e-12


def test_umeyama_reflection_guard():
    rng = np.random.default_rng(4)
    p = rng.normal(0, 1, (40, 3))
    q = p * np.array([1.0, 1.0, -1.0])  # a mirror image: the best PROPER rotation is asked for
    T = rr.umeyama(p, q)
    assert np.linalg.det(T[:3, :3]) > 0


# ---- the conditions the GPU tests rely on, on their own inputs -----------------------------------------------------------
def test_lattice_case_holds_ties_and_duplicates_and_is_exact_in_float32():
    ref, q = rr.lattice_case()
    assert ref.shape == (3000, 3) and q.shape == (1000, 3)
    assert (ref[::97] == ref[0]).all()
    assert (ref * 8 == np.round(ref * 8)).all() and np.abs(ref).max() <= 2 and np.abs(q).max() <= 2
    _, d1, second = rr.nearest(q, ref)
    assert (second == d1).mean() >= 0.10 and (d1 == 0).mean() >= 0.01
    # multiples of 1/64 below 48: exact in float32, so the device's chain must reproduce them bit for bit
    assert (d1 * 64 == np.round(d1 * 64)).all() and d1.max() < 48
    assert (d1.astype(np.float32).astype(np.float64) == d1).all()


def test_lattice_label_case_covers_every_outcome_exactly():
    ref, labels, q, boxes, thr = rr.lattice_label_case()
    for lo, hi in boxes.values():
        assert (lo * 8 == np.round(lo * 8)).all() and (hi * 8 == np.round(hi * 8)).all()
    assert thr * thr == np.float32(thr) * np.float32(thr)
    _, _, outcome = rr.transfer_labels_with_bbox(ref, labels, q, np.eye(4), boxes, thr)
    assert np.bincount(outcome, minlength=5).min() >= 10


@functools.lru_cache(maxsize=None)
def undecided_count(n, m, transformed):
    ref, _, q = rr.clustered_case(n, m)
    qq = rr.moved_queries(q, transformed)
    _, d1, second = rr.nearest(qq, ref)
    ok, _ = rr.decided(np.sqrt(d1), np.sqrt(second), max(np.abs(qq).max(), np.abs(ref).max()), transformed)
    return int((~ok).sum())


@pytest.mark.parametrize("n,m", rr.SIZES)
def test_general_cases_are_decided_but_for_one_percent(n, m):
    for transformed in (False, True):
        assert undecided_count(n, m, transformed) <= 0.01 * m


def test_clustered_case_has_far_queries_and_clusters():
    ref, rid, q = rr.clustered_case(5000, 3000)
    assert len(np.unique(rid)) == rr.NUM_CLUSTERS
    assert (np.abs(q).max(1) > 1.5).mean() > 0.05  # queries far outside the reference bounds
    assert np.abs(ref).max() < 1.5


def test_label_case_covers_every_outcome_and_is_decided_but_for_one_percent():
    case = rr.label_case()
    _, _, outcome = rr.transfer_labels_with_bbox(*case)
    assert np.bincount(outcome, minlength=5).min() >= 10, np.bincount(outcome, minlength=5)
    assert rr.label_undecided(*case).mean() <= 0.01


@pytest.mark.parametrize("which,with_scaling", [(0, True), (1, True), (2, False)])
def test_icp_restatement_converges_to_the_truth(which, with_scaling):
    src, tgt, T_true = rr.icp_case(which)
    assert src.shape == (1056, 3) and tgt.shape == (1456, 3)
    T, fitness, rmse, count, updates = rr.icp(src, tgt, 0.03, with_scaling=with_scaling)
    assert np.abs(T - T_true).max() < 1e-7 and fitness == 1.0 and count == 1056 and rmse < 1e-6
    if which == 1:
        assert updates > 1
        # (one update from the identity is not enough: the first correspondences hold wrong pairs)
        T1 = rr.icp(src, tgt, 0.03, max_iteration=1)[0]
        assert np.abs(T1 - T_true).max() > 1e-4


# ---- the library's argument checks (no device) ----------------------------------------------------------------------------
def test_symbols_exported_and_declared():
    names = {"gsr_nn_index_bytes", "gsr_nn_build", "gsr_nn_query_workspace_bytes", "gsr_nn_query", "gsr_label_transfer",
             "gsr_icp_moments"}
    assert names <= set(_lib.exported_symbols())
    lib = real2sim._bind()
    assert all(hasattr(lib, n) for n in names)
    assert lib.gsr_nn_query.argtypes[0]._type_ is real2sim.GsrNnQuery


def test_workspace_sizes_monotone_and_aligned():
    lib = real2sim._bind()
    for f in (lib.gsr_nn_index_bytes, lib.gsr_nn_query_workspace_bytes):
        sizes = [f(n) for n in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 65536, 1 << 20, 1468850, 1 << 28)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.gsr_nn_index_bytes(1 << 20) >= (1 << 20) * (12 + 4 + 4 + 4)  # sorted points, codes, both permutations
    assert lib.gsr_nn_query_workspace_bytes(1 << 20) >= (1 << 20) * 12
    assert real2sim.ICP_WORKSPACE_BYTES == 256 * 18 * 8 and real2sim.LABEL_MAX_BOXES == 1024


P = 0x10000  # a 256-aligned non-null address the library must never touch on a rejected call


def _query(**kw):
    lib = real2sim._bind()
    a = real2sim.GsrNnQuery(struct_size=C.sizeof(real2sim.GsrNnQuery), n_ref=100, index_mem=P,
                            index_bytes=lib.gsr_nn_index_bytes(100), n_query=10, query=P, max_dist2=-1.0, index=P, dist2=P,
                            workspace=P, workspace_bytes=lib.gsr_nn_query_workspace_bytes(10))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rc(fn, a):
    return getattr(real2sim._bind(), fn)(C.byref(a), None)


def _last():
    return _lib.lib().gsr_last_error()


def test_nn_build_rejects_invalid_arguments():
    lib, E = real2sim._bind(), _lib.GSR_E_INVALID
    nb = lib.gsr_nn_index_bytes(100)
    assert lib.gsr_nn_build(-1, P, P, nb, None) == E and b"gsr_nn_build" in _last()
    assert lib.gsr_nn_build(100, None, P, nb, None) == E
    assert lib.gsr_nn_build(100, P, None, nb, None) == E
    assert lib.gsr_nn_build(100, P, P, nb - 1, None) == E and b"gsr_nn_build" in _last()
    assert lib.gsr_nn_build(100, P, P + 4, nb, None) == E
    assert lib.gsr_nn_build(0, None, None, 0, None) == _lib.GSR_OK  # an empty reference is legal: nothing is launched


def test_nn_query_rejects_invalid_arguments():
    E = _lib.GSR_E_INVALID
    assert real2sim._bind().gsr_nn_query(None, None) == E
    assert _rc("gsr_nn_query", _query(struct_size=8)) == E and b"gsr_nn_query" in _last()
    assert _rc("gsr_nn_query", _query(n_ref=-1)) == E
    assert _rc("gsr_nn_query", _query(n_query=-1)) == E
    assert _rc("gsr_nn_query", _query(max_dist2=float("nan"))) == E
    for field in ("query", "index", "dist2", "workspace", "index_mem"):
        assert _rc("gsr_nn_query", _query(**{field: None})) == E, field
    assert _rc("gsr_nn_query", _query(workspace_bytes=_query().workspace_bytes - 1)) == E
    assert _rc("gsr_nn_query", _query(index_bytes=_query().index_bytes - 1)) == E
    assert _rc("gsr_nn_query", _query(workspace=P + 8)) == E
    assert _rc("gsr_nn_query", _query(n_query=0, query=None, index=None, dist2=None, workspace=None)) == _lib.GSR_OK


def _transfer(**kw):
    a = real2sim.GsrLabelTransfer(struct_size=C.sizeof(real2sim.GsrLabelTransfer), n=10, index=P, points=P, ref_labels=P,
                                  n_ref=100, n_boxes=3, box_labels=P, box_bounds=P, threshold=0.1, labels=P)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_label_transfer_rejects_invalid_arguments():
    E = _lib.GSR_E_INVALID
    assert real2sim._bind().gsr_label_transfer(None, None) == E
    assert _rc("gsr_label_transfer", _transfer(struct_size=0)) == E and b"gsr_label_transfer" in _last()
    assert _rc("gsr_label_transfer", _transfer(n=-1)) == E
    assert _rc("gsr_label_transfer", _transfer(n_boxes=-1)) == E
    assert _rc("gsr_label_transfer", _transfer(n_boxes=real2sim.LABEL_MAX_BOXES + 1)) == E
    for field in ("index", "points", "ref_labels", "box_labels", "box_bounds", "labels"):
        assert _rc("gsr_label_transfer", _transfer(**{field: None})) == E, field
    assert _rc("gsr_label_transfer", _transfer(n=0, index=None, points=None, labels=None)) == _lib.GSR_OK


def _moments(**kw):
    lib = real2sim._bind()
    a = real2sim.GsrIcpMoments(struct_size=C.sizeof(real2sim.GsrIcpMoments), n=10, source=P, n_ref=100, index_mem=P,
                               index_bytes=lib.gsr_nn_index_bytes(100), index=P, dist2=P, sums=P, workspace=P,
                               workspace_bytes=real2sim.ICP_WORKSPACE_BYTES)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_icp_moments_rejects_invalid_arguments():
    E = _lib.GSR_E_INVALID
    assert real2sim._bind().gsr_icp_moments(None, None) == E
    assert _rc("gsr_icp_moments", _moments(struct_size=4)) == E and b"gsr_icp_moments" in _last()
    assert _rc("gsr_icp_moments", _moments(n=-1)) == E
    assert _rc("gsr_icp_moments", _moments(n_ref=-1)) == E
    for field in ("source", "index", "dist2", "sums", "workspace", "index_mem"):
        assert _rc("gsr_icp_moments", _moments(**{field: None})) == E, field
    assert _rc("gsr_icp_moments", _moments(workspace_bytes=real2sim.ICP_WORKSPACE_BYTES - 1)) == E
    assert _rc("gsr_icp_moments", _moments(workspace=P + 4)) == E
    assert _rc("gsr_icp_moments", _moments(index_bytes=_moments().index_bytes - 1)) == E


# ---- the Python layer --------------------------------------------------------------------------------------------------------
def test_no_cpu_path():
    pts = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        real2sim.NearestIndex(pts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        real2sim.transfer_labels(pts, torch.zeros(4, dtype=torch.int32), pts, np.eye(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        real2sim.transfer_labels_with_bbox(pts, torch.zeros(4, dtype=torch.int32), pts, np.eye(4), {})
    with pytest.raises(RuntimeError, match="no CPU path"):
        real2sim.registration_icp(pts, pts, 0.03)
    with pytest.raises(RuntimeError, match="no CPU path"):
        real2sim.semantic_bounding_boxes(pts, torch.zeros(4))


def test_validate_labels_and_transform_rounding():
    d = torch.tensor([0.0, 0.1, 0.1000001, float("inf")])
    assert real2sim.validate_labels(d, 0.1).tolist() == [True, True, False, False]
    T = rr.similarity(1.1, 0.35, (0.2, -0.1, 0.3))
    m = real2sim._transform34(T)
    assert list(m) == T[:3].astype(np.float32).reshape(-1).tolist()
    assert real2sim._transform34(None) is None
    with pytest.raises(ValueError):
        real2sim._transform34(np.eye(3))


def test_segment_cli_reads_its_inputs_without_a_device(tmp_path):
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location(
        "segment_gs", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "segment_gs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pts = np.arange(12, dtype=np.float32).reshape(4, 3)
    np.savez(tmp_path / "src.npz", points=pts, labels=np.array([0, 1, -1, 1]))
    p, lab = mod.read_labelled_cloud(str(tmp_path / "src.npz"))
    assert (p == pts).all() and lab.tolist() == [0, 1, -1, 1]
    np.savez(tmp_path / "boxes.npz", labels=np.array([1, 0]), min=np.zeros((2, 3)), max=np.ones((2, 3)))
    boxes = mod.read_boxes(str(tmp_path / "boxes.npz"))
    assert list(boxes) == [1, 0]  # the file's row order is kept
    assert mod.output_path("/a/b/scan.ply", None) == "/a/b/scan_semantics_gs.npy"
