"""Real2sim on the device against the float64 restatement (tests/ref_real2sim.py): the nearest-point query exactly on lattice
inputs and within stated margins on general floats, its edges, label transfer, the ICP sums, ICP end to end, and the chain
into ``GaussianModelMerger.assign_semantic_labels``.  tests/test_real2sim_cpu.py asserts, on the same inputs, the conditions
the caps here rely on."""
import functools
import types

import numpy as np
import pytest
import torch

from gsworld_amd import real2sim
from tests import ref_real2sim as rr

pytestmark = pytest.mark.gpu


def dev_t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(n, m, transformed):
    """The float64 answer of a clustered case, computed once: (ref, q, moved queries, index, distance, second distance, s)."""
    ref, _, q = rr.clustered_case(n, m)
    moved = rr.moved_queries(q, transformed)  # (under the transform rounded to float32, as the device receives it)
    idx, d1, second = rr.nearest(moved, ref)
    return ref, q, moved, idx, np.sqrt(d1), np.sqrt(second), max(np.abs(moved).max(), np.abs(ref).max())


# ---- (a) exact lattice inputs ------------------------------------------------------------------------------------------------
def test_lattice_index_and_distance_are_exact(cuda_device):
    ref, q = rr.lattice_case()
    idx, d1, _ = rr.nearest(q, ref)
    nn = real2sim.NearestIndex(dev_t(ref, cuda_device))
    index, dist2, moved = nn.query_raw(dev_t(q, cuda_device))
    assert index.dtype == torch.int32 and dist2.dtype == torch.float32
    assert (index.cpu().numpy() == idx).all()  # the first index on every tie and duplicate
    assert (dist2.cpu().numpy().astype(np.float64) == d1).all()
    assert (moved.cpu().numpy() == q).all()
    index64, dist = nn.query(dev_t(q, cuda_device))
    assert index64.dtype == torch.int64 and (index64.cpu().numpy() == idx).all()
    assert (dist.cpu().numpy() == np.sqrt(d1.astype(np.float32))).all()


def test_lattice_label_transfer_is_exact(cuda_device):
    ref, labels, q, boxes, thr = rr.lattice_label_case()
    want, want_dist, _ = rr.transfer_labels_with_bbox(ref, labels, q, np.eye(4), boxes, thr)
    got, dist = real2sim.transfer_labels_with_bbox(dev_t(ref, cuda_device), dev_t(labels, cuda_device), dev_t(q, cuda_device),
                                                   np.eye(4), boxes, thr)
    assert got.dtype == torch.int32 and (got.cpu().numpy() == want).all()
    assert (dist.cpu().numpy() == want_dist.astype(np.float32)).all()


# ---- (b) general floats ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transformed", [False, True])
@pytest.mark.parametrize("n,m", rr.SIZES)
def test_general_floats(cuda_device, n, m, transformed):
    ref, q, moved, idx, d1, second, s = reference(n, m, transformed)
    nn = real2sim.NearestIndex(dev_t(ref, cuda_device))
    index, dist = nn.query(dev_t(q, cuda_device), transform=rr.QUERY_SIMILARITY if transformed else None)
    index, dist = index.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    ok, margin = rr.decided(d1, second, s, transformed)
    print(f"n {n} m {m} transformed {transformed}: undecided {int((~ok).sum())}, wrong among decided "
          f"{int((index[ok] != idx[ok]).sum())}, max dist error over margin {np.max(np.abs(dist - d1) / np.maximum(margin, 1e-300)):.3f}")
    assert (~ok).sum() <= 0.01 * m
    assert (index >= 0).all() and (index < n).all()
    assert (index[ok] == idx[ok]).all()
    # an undecided query may take another point, but one whose float64 distance is within the margin of the minimum
    taken = np.sqrt(((moved - ref.astype(np.float64)[index]) ** 2).sum(1))
    assert (taken - d1 <= margin).all()
    assert (np.abs(dist - d1) <= margin).all()


# ---- (c) edges --------------------------------------------------------------------------------------------------------------------
def brute(q, ref):
    idx, d1, _ = rr.nearest(q, ref)
    return idx, d1


def test_far_queries_and_queries_on_reference_points(cuda_device):
    ref, _, _ = rr.clustered_case(2049, 1000)
    rng = np.random.default_rng(5)
    far = (rng.uniform(50.0, 60.0, (130, 3)) * rng.choice([-1.0, 1.0], (130, 3))).astype(np.float32)
    on = ref[rng.integers(0, len(ref), 200)]
    q = np.concatenate([far, on])
    idx, d1 = brute(q, ref)
    index, dist2, _ = real2sim.NearestIndex(dev_t(ref, cuda_device)).query_raw(dev_t(q, cuda_device))
    index, dist2 = index.cpu().numpy(), dist2.cpu().numpy()
    assert (dist2[130:] == 0).all() and (index[130:] == idx[130:]).all()  # (a duplicated point: the first index)
    taken = ((q.astype(np.float64) - ref.astype(np.float64)[index]) ** 2).sum(1)
    assert (taken[:130] <= d1[:130] * (1 + 1e-6)).all()
    assert np.allclose(dist2[:130], d1[:130], rtol=1e-6, atol=0)


@pytest.mark.parametrize("shape", ["line", "plane", "point"])
def test_degenerate_reference_extents(cuda_device, shape):
    rng = np.random.default_rng(9)
    ref = (rng.integers(-64, 64, (1500, 3)) / 16).astype(np.float32)
    if shape == "line":
        ref[:, 1:] = 0.25
    elif shape == "plane":
        ref[:, 2] = -1.0
    else:
        ref[:] = ref[0]
    q = (rng.integers(-80, 80, (300, 3)) / 16).astype(np.float32)  # exact arithmetic: equality is asked for
    idx, d1 = brute(q, ref)
    index, dist2, _ = real2sim.NearestIndex(dev_t(ref, cuda_device)).query_raw(dev_t(q, cuda_device))
    assert (index.cpu().numpy() == idx).all() and (dist2.cpu().numpy().astype(np.float64) == d1).all()


def test_empty_reference_and_empty_query(cuda_device):
    q = torch.randn(70, 3, device=cuda_device)
    nn = real2sim.NearestIndex(torch.zeros(0, 3, device=cuda_device))
    index, dist2, moved = nn.query_raw(q, transform=rr.QUERY_SIMILARITY)
    assert (index == -1).all() and torch.isinf(dist2).all() and (dist2 > 0).all()
    want = rr.apply_transform(rr.QUERY_SIMILARITY, q.cpu().numpy())
    assert np.abs(moved.cpu().numpy() - want).max() < 1e-5  # the transformed queries are still delivered
    labels, dist = real2sim.transfer_labels(torch.zeros(0, 3, device=cuda_device),
                                            torch.zeros(0, dtype=torch.int32, device=cuda_device), q, np.eye(4))
    assert (labels == -1).all() and torch.isinf(dist).all()
    nn = real2sim.NearestIndex(torch.randn(100, 3, device=cuda_device))
    index, dist = nn.query(torch.zeros(0, 3, device=cuda_device))
    assert index.shape == (0,) and dist.shape == (0,)


def test_max_dist_cuts_some_and_all(cuda_device):
    ref, q, _, idx, d1, _, _ = reference(2049, 1000, False)
    nn = real2sim.NearestIndex(dev_t(ref, cuda_device))
    full_index, full_dist2, _ = nn.query_raw(dev_t(q, cuda_device))
    limit = float(np.median(d1))
    index, dist2, _ = nn.query_raw(dev_t(q, cuda_device), max_dist=limit)
    keep = full_dist2 <= float(np.float32(limit) * np.float32(limit))  # the definition: d2 > max_dist2 is cut
    assert 300 < int(keep.sum()) < 700
    assert (index[keep] == full_index[keep]).all() and (dist2[keep] == full_dist2[keep]).all()
    assert (index[~keep] == -1).all() and torch.isinf(dist2[~keep]).all()
    index, dist2, _ = nn.query_raw(dev_t(q, cuda_device), max_dist=1e-9)
    assert (index == -1).all() and torch.isinf(dist2).all()
    # a limit equal to a distance still matches: queries on reference points under max_dist = 0
    index, dist2, _ = nn.query_raw(dev_t(ref[:100], cuda_device), max_dist=0.0)
    assert (dist2 == 0).all() and (index.cpu().numpy() == brute(ref[:100], ref)[0]).all()
    # through the C ABI a limit of -0.0 is the limit 0, not "no limit": only the queries on reference points match
    import ctypes as C

    mixed = dev_t(np.concatenate([ref[:50], q[:50]]), cuda_device)
    out_i = torch.empty(100, dtype=torch.int32, device=cuda_device)
    out_d = torch.empty(100, device=cuda_device)
    ws = nn._workspace(real2sim._bind(), 100)
    a = real2sim.GsrNnQuery(struct_size=C.sizeof(real2sim.GsrNnQuery), n_ref=nn.n, index_mem=nn.mem.data_ptr(),
                            index_bytes=nn.index_bytes, n_query=100, query=mixed.data_ptr(), max_dist2=-0.0,
                            index=out_i.data_ptr(), dist2=out_d.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    assert np.signbit(np.float32(a.max_dist2))
    real2sim.check(real2sim._bind().gsr_nn_query(C.byref(a), C.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream)))
    assert (out_d[:50] == 0).all() and (out_i[:50].cpu().numpy() == brute(ref[:50], ref)[0]).all()
    assert (full_dist2[:50] > 0).all() and (out_i[50:] == -1).all() and torch.isinf(out_d[50:]).all()


def test_non_finite_queries_leave_their_neighbours_alone(cuda_device):
    ref, q, _, _, _, _, _ = reference(1025, 257, False)
    nn = real2sim.NearestIndex(dev_t(ref, cuda_device))
    clean_index, clean_dist2, _ = nn.query_raw(dev_t(q, cuda_device))
    bad = q.copy()
    rows = np.array([0, 1, 63, 64, 65, 128, 200, 256])
    bad[rows, [0, 1, 2, 0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.nan]
    index, dist2, _ = nn.query_raw(dev_t(bad, cuda_device))
    mask = np.zeros(len(q), bool)
    mask[rows] = True
    mask = torch.from_numpy(mask).to(cuda_device)
    assert (index[mask] == -1).all() and torch.isinf(dist2[mask]).all() and (dist2[mask] > 0).all()
    assert (index[~mask] == clean_index[~mask]).all() and (dist2[~mask] == clean_dist2[~mask]).all()
    with pytest.raises(ValueError, match="non-finite"):
        real2sim.NearestIndex(dev_t(bad, cuda_device))


def test_outputs_land_between_guards_in_poisoned_buffers(cuda_device):
    ref, q, _, idx, _, _, _ = reference(1023, 257, False)
    m, g = len(q), 64
    nn = real2sim.NearestIndex(dev_t(ref, cuda_device))
    want = nn.query_raw(dev_t(q, cuda_device), transform=rr.QUERY_SIMILARITY)
    index = torch.full((m + 2 * g,), -7, dtype=torch.int32, device=cuda_device)
    dist2 = torch.full((m + 2 * g,), float("nan"), device=cuda_device)
    moved = torch.full((m + 2 * g, 3), float("nan"), device=cuda_device)
    got = nn.query_raw(dev_t(q, cuda_device), transform=rr.QUERY_SIMILARITY, out=(index[g:g + m], dist2[g:g + m], moved[g:g + m]))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert (index[:g] == -7).all() and (index[g + m:] == -7).all()
    assert torch.isnan(dist2[:g]).all() and torch.isnan(dist2[g + m:]).all()
    assert torch.isnan(moved[:g]).all() and torch.isnan(moved[g + m:]).all()


def test_query_order_and_reuse_do_not_change_the_answer(cuda_device):
    ref, q, _, _, _, _, _ = reference(5000, 3000, True)
    nn = real2sim.NearestIndex(dev_t(ref, cuda_device))
    a = nn.query_raw(dev_t(q, cuda_device), transform=rr.QUERY_SIMILARITY)
    a = tuple(t.clone() for t in a)
    perm = np.random.default_rng(2).permutation(len(q))
    b = nn.query_raw(dev_t(q[perm], cuda_device), transform=rr.QUERY_SIMILARITY)
    p = torch.from_numpy(perm).to(cuda_device)
    for x, y in zip(a, b):
        assert torch.equal(x[p], y)  # per query: the same bytes in another launch position
    junk = torch.full((1 << 20,), float("nan"), device=cuda_device)  # an unrelated allocation in between
    c = nn.query_raw(dev_t(q, cuda_device), transform=rr.QUERY_SIMILARITY)
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    del junk


# ---- (d) label transfer, general --------------------------------------------------------------------------------------------
def test_label_transfer_general(cuda_device):
    case = rr.label_case()
    ref, labels, targets, T, boxes, thr = case
    want, want_dist, outcome = rr.transfer_labels_with_bbox(*case)
    undecided = rr.label_undecided(*case)
    src, lab, tgt = dev_t(ref, cuda_device), dev_t(labels, cuda_device), dev_t(targets, cuda_device)
    got, dist = real2sim.transfer_labels_with_bbox(src, lab, tgt, T, boxes, thr)
    got, dist = got.cpu().numpy(), dist.cpu().numpy()
    print(f"outcomes {np.bincount(outcome, minlength=5).tolist()}, undecided {int(undecided.sum())}, "
          f"differing among undecided {int((got != want)[undecided].sum())}, among decided {int((got != want)[~undecided].sum())}")
    assert undecided.mean() <= 0.01
    assert (got[~undecided] == want[~undecided]).all()
    s = max(np.abs(ref).max(), np.abs(rr.apply_transform(np.linalg.inv(T), targets)).max())
    assert (np.abs(dist - want_dist) <= 1e-6 * want_dist + 1e-5 * s).all()
    # the plain transfer and the distance validation on the same data
    plain, plain_dist = real2sim.transfer_labels(src, lab, tgt, T)
    moved = rr.apply_transform(np.linalg.inv(T), targets)
    idx, d1, second = rr.nearest(moved, ref)
    ok, _ = rr.decided(np.sqrt(d1), np.sqrt(second), s, True)
    assert (plain.cpu().numpy()[ok] == labels[idx][ok]).all()
    assert torch.equal(plain_dist, torch.from_numpy(dist).to(cuda_device))
    # a target with a non-finite coordinate has no neighbour: -1 from both transfers (not the LAST source's label), distance inf
    bad = targets[:200].copy()
    bad[[3, 150], [0, 2]] = [np.nan, np.inf]
    keep = np.ones(200, bool)
    keep[[3, 150]] = False
    assert labels[-1] != -1
    for (labs, dists), clean in ((real2sim.transfer_labels(src, lab, dev_t(bad, cuda_device), T), plain.cpu().numpy()),
                                 (real2sim.transfer_labels_with_bbox(src, lab, dev_t(bad, cuda_device), T, boxes, thr), got)):
        assert labs[[3, 150]].tolist() == [-1, -1] and torch.isinf(dists[[3, 150]]).all()
        assert (labs.cpu().numpy()[keep] == clean[:200][keep]).all()  # (the rows around them are answered as before)
    valid = real2sim.validate_labels(plain_dist, 0.1).cpu().numpy()
    clear = np.abs(np.sqrt(d1) - 0.1) > 1e-5 * s
    assert (valid[clear] == (np.sqrt(d1) <= 0.1)[clear]).all() and 0 < valid.sum() < len(valid)


def test_semantic_bounding_boxes(cuda_device):
    ref, rid, _ = rr.clustered_case(2049, 1000)
    got = real2sim.semantic_bounding_boxes(dev_t(ref, cuda_device), dev_t(rid, cuda_device))
    want = rr.semantic_bounding_boxes(ref, rid)
    assert list(got) == list(want)
    for k in want:
        assert (got[k][0].cpu().numpy() == want[k][0].astype(np.float32)).all()
        assert (got[k][1].cpu().numpy() == want[k][1].astype(np.float32)).all()


# ---- (e) ICP moments --------------------------------------------------------------------------------------------------------------
def test_icp_moments_against_float64_sums(cuda_device):
    ref, q, _, _, d1, _, _ = reference(2049, 1000, True)
    nn = real2sim.NearestIndex(dev_t(ref, cuda_device))
    src = dev_t(q, cuda_device)
    index, dist2, moved = nn.query_raw(src, transform=rr.QUERY_SIMILARITY, max_dist=float(np.median(d1)))
    got = nn.moments(src, rr.QUERY_SIMILARITY, index, dist2)
    again = nn.moments(src, rr.QUERY_SIMILARITY, index, dist2)
    assert got.tobytes() == again.tobytes()
    idx = index.cpu().numpy()
    inl = idx >= 0
    assert 300 < inl.sum() < 700 and got[0] == inl.sum()
    p = moved.cpu().numpy().astype(np.float64)[inl]  # the device's own transformed sources, widened
    qq = ref.astype(np.float64)[idx[inl]]
    terms = [np.ones((len(p), 1)), p, qq, (p[:, :, None] * qq[:, None, :]).reshape(len(p), 9), (p * p).sum(1, keepdims=True),
             dist2.cpu().numpy().astype(np.float64)[inl][:, None]]
    terms = np.concatenate(terms, 1)
    want, scale = terms.sum(0), np.abs(terms).sum(0)
    print("max |sum error| / sum |terms|:", np.max(np.abs(got - want) / scale))
    assert (np.abs(got - want) <= 1e-6 * scale).all()
    # p' is what the query delivered: the float32 transform of the sources, within its rounding of the float64 product
    assert np.abs(p - rr.moved_queries(q, True)[inl]).max() <= 1e-5 * np.abs(p).max()


def test_icp_moments_of_nothing_are_zero(cuda_device):
    nn = real2sim.NearestIndex(torch.randn(50, 3, device=cuda_device))
    src = torch.randn(30, 3, device=cuda_device) + 100.0
    index, dist2, _ = nn.query_raw(src, max_dist=0.5)
    assert (index == -1).all()
    assert (nn.moments(src, None, index, dist2) == 0).all()


# ---- (f) ICP end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,with_scaling", [(0, True), (1, True), (2, False)])
def test_icp_converges_to_the_truth(cuda_device, which, with_scaling):
    src, tgt, T_true = rr.icp_case(which)
    r = real2sim.registration_icp(dev_t(src, cuda_device), dev_t(tgt, cuda_device), 0.03, with_scaling=with_scaling)
    print(f"case {which}: max |T - T_true| {np.abs(r.transformation - T_true).max():.3e}, fitness {r.fitness}, rmse "
          f"{r.inlier_rmse:.3e}, iterations {r.iterations}")
    assert r.transformation.dtype == np.float64 and r.transformation.shape == (4, 4)
    assert np.abs(r.transformation - T_true).max() <= 1e-5
    assert r.fitness == 1.0 and r.num_correspondences == len(src)
    assert r.inlier_rmse <= 1e-5
    assert 1 <= r.iterations < 30


def test_icp_with_fewer_than_three_inliers_returns_the_start(cuda_device):
    src, tgt, _ = rr.icp_case(0)
    init = rr.similarity(1.0, 0.0, (50.0, 0.0, 0.0))
    r = real2sim.registration_icp(dev_t(src, cuda_device), dev_t(tgt, cuda_device), 0.03, init=init)
    assert (r.transformation == init).all() and r.fitness == 0.0 and r.num_correspondences == 0 and r.iterations == 0
    assert r.inlier_rmse == 0.0


# ---- (g) the chain ----------------------------------------------------------------------------------------------------------------
def test_labels_reach_the_merger(cuda_device, tmp_path):
    from gsworld_amd.merger import GaussianModelMerger

    ref, labels, targets, T, boxes, thr = rr.label_case()
    got, _ = real2sim.transfer_labels_with_bbox(dev_t(ref, cuda_device), dev_t(labels, cuda_device),
                                                dev_t(targets, cuda_device), T, boxes, thr)
    path = str(tmp_path / "scan_semantics_gs.npy")
    np.save(path, got.cpu().numpy().astype(np.int64))
    merger = GaussianModelMerger.__new__(GaussianModelMerger)
    merger.device = cuda_device
    model = types.SimpleNamespace(_xyz=dev_t(targets, cuda_device))
    model = merger.assign_semantic_labels(model, path)
    assert model._semantics.shape == (len(targets), 1) and model._semantics.device.type == "cuda"
    assert torch.equal(model._semantics[:, 0].to(torch.int32), got)
    assert set(np.unique(got.cpu().numpy())) >= {-1, 4, 5}
