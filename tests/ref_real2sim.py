"""Independent float64 numpy restatement of the real2sim steps (the checker of tests/test_real2sim_*.py): brute-force
all-pairs nearest point, the label rules of GSWorld's segment_utils.transfer_labels_with_bbox:85-112 line for line, and
point-to-point ICP with Umeyama's solve.  Also the seeded inputs both test files use, so that the conditions the GPU tests
rely on are asserted (test_real2sim_cpu.py) on exactly the data those tests run."""
import numpy as np

SIZES = [(1, 65), (2, 1), (63, 64), (64, 63), (1023, 257), (1025, 257), (2049, 1000), (5000, 3000)]
NUM_CLUSTERS = 12


# ---- nearest point ------------------------------------------------------------------------------------------------------------
def all_pairs_d2(q, ref, chunk=512):
    """(m, n) float64 squared distances, chunked over the queries."""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    out = np.empty((len(q), len(ref)))
    for a in range(0, len(q), chunk):
        d = q[a:a + chunk, None, :] - ref[None, :, :]
        out[a:a + chunk] = (d * d).sum(-1)
    return out


def nearest(q, ref, chunk=512):
    """-> (index of the first minimum, its squared distance, the second-smallest squared distance (inf when n == 1))."""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    idx, d1, second = np.empty(len(q), np.int64), np.empty(len(q)), np.full(len(q), np.inf)
    for a in range(0, len(q), chunk):
        d2 = all_pairs_d2(q[a:a + chunk], ref)
        rows = np.arange(len(d2))
        idx[a:a + chunk] = d2.argmin(1)
        d1[a:a + chunk] = d2[rows, idx[a:a + chunk]]
        if d2.shape[1] > 1:
            d2[rows, idx[a:a + chunk]] = np.inf
            second[a:a + chunk] = d2.min(1)
    return idx, d1, second


def apply_transform(T, pts):
    T, pts = np.asarray(T, np.float64), np.asarray(pts, np.float64)
    return pts @ T[:3, :3].T + T[:3, 3]


def similarity(scale, angle_z, translation):
    c, s = np.cos(angle_z), np.sin(angle_z)
    T = np.eye(4)
    T[:3, :3] = scale * np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = translation
    return T


# ---- the label rules --------------------------------------------------------------------------------------------------------------
def point_to_bbox_distance(point, min_bound, max_bound):
    dx = max(min_bound[0] - point[0], 0, point[0] - max_bound[0])
    dy = max(min_bound[1] - point[1], 0, point[1] - max_bound[1])
    dz = max(min_bound[2] - point[2], 0, point[2] - max_bound[2])
    return np.sqrt(dx * dx + dy * dy + dz * dz)


KEPT, RELABELLED, INVALIDATED, SOURCE_UNLABELLED, NO_BOX = range(5)


def validate_with_bbox(points, transferred_labels, semantic_bboxes, threshold):
    """segment_utils.py:85-112 on points already in the source frame -> (labels, outcome per point)."""
    labels = np.array(transferred_labels, dtype=np.int64)
    outcome = np.empty(len(labels), np.int64)
    for i in range(len(points)):
        point = points[i]
        current_label = int(labels[i])
        if current_label == -1:
            outcome[i] = SOURCE_UNLABELLED
            continue
        if current_label in semantic_bboxes:
            min_bound, max_bound = semantic_bboxes[current_label]
            outcome[i] = KEPT
            if point_to_bbox_distance(point, min_bound, max_bound) > threshold:
                min_distance = float("inf")
                best_label = -1
                for sem_idx, (min_b, max_b) in semantic_bboxes.items():
                    dist = point_to_bbox_distance(point, min_b, max_b)
                    if dist < min_distance and dist <= threshold:
                        min_distance = dist
                        best_label = sem_idx
                labels[i] = best_label
                outcome[i] = RELABELLED if best_label != -1 else INVALIDATED
        else:
            labels[i] = -1
            outcome[i] = NO_BOX
    return labels, outcome


def box_distances(points, semantic_bboxes):
    """(M, rows) float64 distances of every point to every box, rows in the dict's order."""
    p = np.asarray(points, np.float64)
    cols = []
    for lo, hi in semantic_bboxes.values():
        e = np.maximum(np.maximum(np.asarray(lo, np.float64) - p, 0.0), p - np.asarray(hi, np.float64))
        cols.append(np.sqrt((e * e).sum(1)))
    return np.stack(cols, 1) if cols else np.zeros((len(p), 0))


def transfer_labels_with_bbox(source_points, source_labels, target_points, transformation_matrix, semantic_bboxes,
                              bbox_distance_threshold=0.1):
    moved = apply_transform(np.linalg.inv(np.asarray(transformation_matrix, np.float64)), target_points)
    idx, d1, _ = nearest(moved, source_points)
    labels, outcome = validate_with_bbox(moved, np.asarray(source_labels)[idx], semantic_bboxes, bbox_distance_threshold)
    return labels, np.sqrt(d1), outcome


def semantic_bounding_boxes(vertices, labels):
    v, lab = np.asarray(vertices, np.float64), np.asarray(labels)
    return {int(k): (v[lab == k].min(0), v[lab == k].max(0)) for k in np.unique(lab)}


# ---- ICP --------------------------------------------------------------------------------------------------------------------------
def umeyama(p, q, with_scaling=True):
    """The similarity (4, 4) minimising sum |s R p + t - q|^2 over exact correspondences p[i] <-> q[i] (Umeyama 1991)."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    mp, mq = p.mean(0), q.mean(0)
    cov = (q - mq).T @ (p - mp) / len(p)
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    scale = (D * S).sum() / ((p - mp) ** 2).sum(1).mean() if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = mq - scale * R @ mp
    return T


def icp(source, target, max_dist, init=None, with_scaling=True, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> (T, fitness, rmse, correspondences, updates): evaluate under T; stop on < 3 inliers, on the iteration limit, or
    when fitness and RMSE both moved by less than their thresholds; else T <- umeyama(inliers) T."""
    T = np.eye(4) if init is None else np.array(init, np.float64)
    prev, updates = None, 0
    for it in range(max_iteration + 1):
        moved = apply_transform(T, source)
        idx, d1, _ = nearest(moved, target)
        inl = d1 <= max_dist * max_dist
        count = int(inl.sum())
        fitness = count / len(source)
        rmse = float(np.sqrt(d1[inl].sum() / count)) if count else 0.0
        if count < 3 or it == max_iteration:
            break
        if prev is not None and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
        prev = (fitness, rmse)
        T = umeyama(moved[inl], np.asarray(target, np.float64)[idx[inl]], with_scaling) @ T
        updates += 1
    return T, fitness, rmse, count, updates


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------
def lattice_case(n_ref=3000, n_query=1000):
    """Integer multiples of 1/8 in [-2, 2): every difference, square and sum is exact in float32; duplicates and ties abound."""
    rng = np.random.default_rng(7)
    ref = (rng.integers(-16, 16, (n_ref, 3)) / 8).astype(np.float32)
    ref[::97] = ref[0]
    q = (rng.integers(-16, 16, (n_query, 3)) / 8).astype(np.float32)
    return ref, q


def lattice_label_case():
    """Labels and boxes on the lattice (threshold 0.125): every box distance and the comparison are exact in float32."""
    ref, q = lattice_case()
    labels = (np.floor((ref[:, 0] + 2.0)).astype(np.int64) + 4 * (ref[:, 1] >= 0)).astype(np.int32)  # 8 slabs
    labels[::50] = -1
    boxes = semantic_bounding_boxes(ref[labels >= 0], labels[labels >= 0])
    del boxes[7]  # a label without a box row
    lo, hi = boxes[2]
    boxes[2] = (lo + np.array([0.25, 0.5, 0.0]), hi - np.array([0.25, 0.0, 0.5]))  # shrunk: own-box validation fails
    lo, hi = boxes[5]
    boxes[5] = (lo - 0.5, hi + 0.5)  # grown: captures neighbours
    return ref, labels, q, boxes, 0.125


def centres():
    return np.random.default_rng(11).uniform(-1.0, 1.0, (NUM_CLUSTERS, 3))


def clustered_case(n_ref, n_query):
    """References: 12 clusters (sigma 0.05); queries: 90 % around the centres (sigma 0.08), 10 % uniform in [-3, 3]^3.
    -> (ref float32, cluster id per reference, queries float32)."""
    rng = np.random.default_rng(1000 * n_ref + n_query)
    c = centres()
    rid = rng.integers(0, NUM_CLUSTERS, n_ref)
    ref = (c[rid] + rng.normal(0.0, 0.05, (n_ref, 3))).astype(np.float32)
    qid = rng.integers(0, NUM_CLUSTERS, n_query)
    q = c[qid] + rng.normal(0.0, 0.08, (n_query, 3))
    far = rng.random(n_query) < 0.1
    q[far] = rng.uniform(-3.0, 3.0, (int(far.sum()), 3))
    return ref, rid.astype(np.int32), q.astype(np.float32)


QUERY_SIMILARITY = similarity(1.1, 0.35, (0.2, -0.1, 0.3))
QUERY_SIMILARITY32 = QUERY_SIMILARITY.astype(np.float32).astype(np.float64)  # as the device receives it


def moved_queries(q, transformed):
    """The queries of a general case as the reference sees them: float64, under the float32-rounded similarity or plain."""
    return apply_transform(QUERY_SIMILARITY32, q) if transformed else np.asarray(q, np.float64)


def decided(dist1, dist2nd, s, transformed):
    """The margin of a decided query, on DISTANCES: the float64 gap between best and second best exceeds 1e-6 dist1 (+ 1e-5 s
    under a transform, s the largest absolute coordinate) -- about 8x the float32 rounding of the chain and of the 3 x 4
    product.  -> (decided mask, margin)."""
    margin = 1e-6 * dist1 + (1e-5 * s if transformed else 0.0)
    return (dist2nd - dist1) > margin, margin


def label_case():
    """The (5000, 3000) clustered case with labels = cluster ids, every 50th source unlabelled, one label without a box,
    four boxes shrunk toward their centres and one grown.  -> (ref, labels, q, T (source -> target), boxes, threshold)."""
    ref, rid, q = clustered_case(5000, 3000)
    labels = rid.copy()
    labels[::50] = -1
    boxes = semantic_bounding_boxes(ref[labels >= 0], labels[labels >= 0])
    del boxes[11]
    for k in (0, 1, 2, 3):
        lo, hi = boxes[k]
        mid, half = (lo + hi) / 2, (hi - lo) / 2
        boxes[k] = (mid - 0.15 * half, mid + 0.15 * half)
    lo, hi = boxes[4]
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    boxes[4] = (mid - 4.0 * half, mid + 4.0 * half)
    # the targets live in the scan's frame: T maps the source frame onto it, the transfer applies inv(T)
    T = QUERY_SIMILARITY
    targets = apply_transform(T, q).astype(np.float32)
    return ref, labels, targets, T, boxes, 0.1


def label_undecided(ref, labels, targets, T, boxes, threshold):
    """Points whose label may legitimately differ in float32: an undecided neighbour, a box distance within 1e-5 s of the
    threshold, or -- where the own box does not clearly hold the point, so that the search for a closer box can run -- the
    two smallest qualifying box distances within 1e-5 s of each other."""
    moved = apply_transform(np.linalg.inv(T), targets)
    s = max(np.abs(moved).max(), np.abs(ref).max())
    idx, d1, second = nearest(moved, ref)
    ok, _ = decided(np.sqrt(d1), np.sqrt(second), s, True)
    bd = box_distances(moved, boxes)
    near_thr = (np.abs(bd - threshold) <= 1e-5 * s).any(1)
    rows = {k: r for r, k in enumerate(boxes)}
    own = np.array([bd[i, rows[l]] if l in rows else np.inf for i, l in enumerate(np.asarray(labels)[idx])])
    qual = np.where(bd <= threshold + 1e-5 * s, bd, np.inf)
    qual.sort(1)
    with np.errstate(invalid="ignore"):
        close = np.isfinite(qual[:, 1]) & ((qual[:, 1] - qual[:, 0]) <= 1e-5 * s) & np.isfinite(own) & (own > threshold - 1e-5 * s)
    return ~ok | near_thr | close


def icp_case(which):
    """Source: a 12^3 grid of spacing 0.05 with 60 % occupancy and +-0.005 jitter (1 056 points by this seed's draw);
    target: its exact similarity image rounded to float32 plus 400 uniform distractors, shuffled.
    which 0: 0.5 deg, scale 1.01, 5 mm; 1: 4 deg, scale 1.04, 15-20 mm; 2: rigid (scale 1), 2 deg, 10 mm."""
    rng = np.random.default_rng(23)
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.05
    keep = np.argsort(rng.random(len(g)))[:1056]
    src = (g[np.sort(keep)] + rng.uniform(-0.005, 0.005, (1056, 3))).astype(np.float32)
    scale, deg, t = [(1.01, 0.5, (0.005, 0.0, 0.0)), (1.04, 4.0, (0.015, -0.02, 0.018)), (1.0, 2.0, (0.01, 0.0, -0.01))][which]
    a = np.deg2rad(deg)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    c = src.astype(np.float64).mean(0)
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = c - scale * R @ c + np.array(t)  # (rotation and scaling about the cloud's centre)
    lo, hi = src.min(0) - 0.1, src.max(0) + 0.1
    tgt = np.concatenate([apply_transform(T, src), rng.uniform(lo, hi, (400, 3))]).astype(np.float32)
    rng.shuffle(tgt)
    return src, tgt, T
