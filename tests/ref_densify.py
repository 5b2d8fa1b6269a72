"""NumPy restatement of include/gsr.h ``gsr_densify_plan`` / ``gsr_densify_apply`` (the definition is that header comment):
decisions and copies in float32, operation by operation in the written order; the computed child values (scaling,
position) also in binary64 from the float32 inputs.  Test infrastructure: nothing in the product imports it.

NumPy's float32 exp / log and the device's need not round alike, so the tests draw inputs whose decisions do not depend on
the last bit (``margins``) and hold the computed child values to the binary64 evaluation within stated bounds."""
import numpy as np

F = np.float32
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
MODEL_M = (3, 3, 45, 1, 3, 4)
U = 2.0 ** -23


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def plan(accum, denom, scaling, opacity, grad_threshold, min_opacity, dense_limit, world_limit, world_on):
    """-> dict: keep / clone / split (bool, N), counts (kept, clones, split, N_out), parent (N_out,), child_s (N,3) float32."""
    accum, denom, opacity = (np.asarray(a, F).reshape(-1) for a in (accum, denom, opacity))
    s = np.asarray(scaling, F).reshape(-1, 3)
    thr, mop, dl, wl = F(grad_threshold), F(min_opacity), F(dense_limit), F(world_limit)
    with np.errstate(all="ignore"):
        g = accum / denom
        g[np.isnan(g)] = F(0)
        hot_clone = np.abs(g) >= thr
        hot_split = g >= thr
        e = np.exp(s)
        assert e.dtype == F
        smax = np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2])  # np.maximum propagates NaN
        small = smax <= dl
        clone_sel = hot_clone & small
        split_sel = hot_split & ~small
        op = F(1) / (F(1) + np.exp(-opacity))
        prune_op = op < mop
        big_self = bool(world_on) & (smax > wl)
        child_s = np.log(e / F(1.6))
        ce = np.exp(child_s)
        big_child = bool(world_on) & (np.maximum(np.maximum(ce[:, 0], ce[:, 1]), ce[:, 2]) > wl)
    keep = ~split_sel & ~prune_op & ~big_self
    clone = clone_sel & ~prune_op & ~big_self
    split = split_sel & ~prune_op & ~big_child
    i = np.arange(accum.size, dtype=np.int32)
    parent = np.concatenate((i[keep], i[clone], i[split], i[split])).astype(np.int32)
    counts = (int(keep.sum()), int(clone.sum()), int(split.sum()), int(parent.size))
    return {"keep": keep, "clone": clone, "split": split, "counts": counts, "parent": parent, "child_s": child_s.astype(F)}


def margins(accum, denom, scaling, opacity, grad_threshold, min_opacity, dense_limit, world_limit):
    """-> (N,) float64: the smallest relative distance of a compared quantity (|g|, g, smax, op, the child's smax) from its
    threshold, evaluated in binary64 from the float32 inputs; a NaN quantity compares false on every side (inf distance)."""
    accum, denom, opacity = (np.asarray(a, F).reshape(-1).astype(np.float64) for a in (accum, denom, opacity))
    s = np.asarray(scaling, F).reshape(-1, 3).astype(np.float64)
    thr, mop, dl, wl = (float(F(x)) for x in (grad_threshold, min_opacity, dense_limit, world_limit))
    with np.errstate(all="ignore"):
        g = accum / denom
        g[np.isnan(g)] = 0.0
        smax = np.exp(s).max(axis=1)  # (ndarray.max propagates NaN)
        op = 1.0 / (1.0 + np.exp(-opacity))
        pairs = ((np.abs(g), thr), (g, thr), (smax, dl), (smax, wl), (smax / float(F(1.6)), wl), (op, mop))
        out = np.full(accum.size, np.inf)
        for q, t in pairs:
            d = np.abs(q - t) / t
            out = np.minimum(out, np.where(np.isnan(d), np.inf, d))
    return out


def rotation_rows(q, dtype):
    """build_rotation of raw quaternions (n, 4) in ``dtype``, the header's order of operations -> (n, 3, 3)."""
    q = q.astype(dtype)
    one, two = dtype(1), dtype(2)
    with np.errstate(all="ignore"):
        rw, rx, ry, rz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        n = np.sqrt(((rw * rw + rx * rx) + ry * ry) + rz * rz)
        w, x, y, z = rw / n, rx / n, ry / n, rz / n
        R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                      two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                      two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], 1)
    assert R.dtype == dtype
    return R.reshape(-1, 3, 3)


def children(xyz, scaling, rotation, noise, parents, c, dtype):
    """Child ``c`` of the rows ``parents`` -> (position (n,3), scaling (n,3), sum_j |v_j| (n,)) evaluated in ``dtype``."""
    s = np.asarray(scaling, F).reshape(-1, 3)[parents].astype(dtype)
    x = np.asarray(xyz, F).reshape(-1, 3)[parents].astype(dtype)
    nz = np.asarray(noise, F).reshape(-1, 2, 3)[parents, c].astype(dtype)
    with np.errstate(all="ignore"):
        e = np.exp(s)
        v = e * nz
        R = rotation_rows(np.asarray(rotation, F).reshape(-1, 4)[parents], dtype)
        t = (R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2]) + R[:, :, 2] * v[:, 2:3]
        pos = t + x
        child_s = np.log(e / dtype(F(1.6)))
    assert pos.dtype == dtype and child_s.dtype == dtype
    return pos, child_s, np.abs(v).sum(axis=1)


def apply(pl, groups, noise):
    """``groups``: name -> (param, exp_avg | None, exp_avg_sq | None), (N, M) float32 each.  -> name -> (param, m, v) of
    N_out rows: copies bit for bit, zero moments on new rows, computed children in float32."""
    K, Cn, S, n_out = pl["counts"]
    parent = pl["parent"]
    out = {}
    for name, (p, m, v) in groups.items():
        q = np.asarray(p, F)[parent].copy()
        if name in ("xyz", "scaling") and S:
            for c in (0, 1):
                rows = slice(K + Cn + c * S, K + Cn + (c + 1) * S)
                pos, cs, _ = children(groups["xyz"][0], groups["scaling"][0], groups["rotation"][0], noise, parent[rows], c, F)
                q[rows] = pos if name == "xyz" else cs
        if m is None:
            out[name] = (q, None, None)
            continue
        mq, vq = np.asarray(m, F)[parent].copy(), np.asarray(v, F)[parent].copy()
        mq[K:] = 0
        vq[K:] = 0
        out[name] = (q, mq, vq)
    return out


def child_bounds(pl, groups, noise):
    """The binary64 child values and their bounds: -> list over c of (rows, pos64, pos_bound, s64, s_bound).
    scaling: 4 * 2^-23 * max(1, |value|) (expf, one division, logf, each <= 1 ulp, doubled); position component k:
    16 * 2^-23 * (|xyz_k| + sum_j |v_j|) (the normalisation, nine entries of <= 6 roundings, three products, three sums)."""
    K, Cn, S, _ = pl["counts"]
    out = []
    for c in (0, 1):
        rows = slice(K + Cn + c * S, K + Cn + (c + 1) * S)
        par = pl["parent"][rows]
        pos, cs, va = children(groups["xyz"][0], groups["scaling"][0], groups["rotation"][0], noise, par, c, np.float64)
        x = np.abs(np.asarray(groups["xyz"][0], F).reshape(-1, 3)[par].astype(np.float64))
        out.append((rows, pos, 16 * U * (x + va[:, None]), cs, 4 * U * np.maximum(1.0, np.abs(cs))))
    return out


# ---- inputs whose decisions do not hang on the last bit -----------------------------------------------------------------
THRESHOLDS = dict(grad_threshold=2e-4, min_opacity=5e-3, extent=2.0, percent_dense=0.01)
KEEP, PRUNE, CLONE, SPLIT, BIG, MID, CLONE_NEG = range(7)
MARGIN = 1e-4


def limits(extent=THRESHOLDS["extent"], percent_dense=THRESHOLDS["percent_dense"]):
    """(dense_limit, world_limit) as the caller forms them, in binary32."""
    return F(percent_dense) * F(extent), F(0.1) * F(extent)


def _rows(rng, action):
    """accum, denom, scaling, opacity of rows with the given intent (what the row becomes also depends on the world flag):
    KEEP cold, small or large, opaque | PRUNE transparent, anything else | CLONE hot and small | CLONE_NEG a negative
    quotient: hot by norm, not by value -- cloned when small, else kept | SPLIT hot and large | BIG larger than 1.6 x the world
    limit, hot or not (with the flag: self and children pruned) | MID hot, between the world limit and 1.6 x it (with the flag:
    the self is gone either way, the children stay)."""
    n = action.size
    thr = THRESHOLDS["grad_threshold"]
    dl, wl = (float(x) for x in limits())
    denom = rng.integers(1, 40, n).astype(F)
    hot = np.isin(action, (CLONE, SPLIT, MID, CLONE_NEG)) | (np.isin(action, (PRUNE, BIG)) & (rng.random(n) < 0.5))
    g = np.where(hot, thr * rng.uniform(1.05, 30.0, n), thr * rng.uniform(0.0, 0.9, n))
    g = np.where(action == CLONE_NEG, -g, g)
    accum = (g * denom).astype(F)
    lo = np.full(n, dl * 0.05)
    hi = np.full(n, dl * 0.95)
    large = np.isin(action, (SPLIT,)) | (np.isin(action, (KEEP, PRUNE, CLONE_NEG)) & (rng.random(n) < 0.5))
    lo[large], hi[large] = dl * 1.05, wl * 0.95
    lo[action == BIG], hi[action == BIG] = wl * 1.7, wl * 20
    lo[action == MID], hi[action == MID] = wl * 1.05, wl * 1.5
    smax = np.exp(rng.uniform(np.log(lo), np.log(hi)))
    sc = smax[:, None] * rng.uniform(0.1, 1.0, (n, 3))
    sc[np.arange(n), rng.integers(0, 3, n)] = smax
    scaling = np.log(sc).astype(F)
    mop = THRESHOLDS["min_opacity"]
    op = np.where(action == PRUNE, mop * rng.uniform(0.05, 0.9, n), rng.uniform(mop * 1.2, 0.99, n))
    opacity = np.log(op / (1 - op)).astype(F)
    return accum, denom, scaling, opacity


def make_inputs(rng, action):
    """-> dict accum (N,1), denom (N,1), scaling (N,3), opacity (N,1): rows of ``_rows``, redrawn until every compared quantity
    sits at least MARGIN relative from its threshold (checked in binary64 by ``margins``)."""
    action = np.asarray(action)
    accum, denom, scaling, opacity = _rows(rng, action)
    dl, wl = limits()
    for _ in range(20):
        bad = margins(accum, denom, scaling, opacity, THRESHOLDS["grad_threshold"], THRESHOLDS["min_opacity"], dl, wl) < MARGIN
        if not bad.any():
            break
        a, d, s, o = _rows(rng, action[bad])
        accum[bad], denom[bad], scaling[bad], opacity[bad] = a, d, s, o
    return {"accum": accum[:, None], "denom": denom[:, None], "scaling": scaling, "opacity": opacity[:, None]}


def make_model(rng, N, scaling, opacity, moments=True):
    """name -> (param, exp_avg, exp_avg_sq) (N, M) float32; f_dc's first column carries the row index (the order of the
    output shows in the data itself), moments non-zero everywhere."""
    groups = {}
    for name, M in zip(NAMES, MODEL_M):
        p = rng.normal(0.0, 1.0, (N, M)).astype(F)
        if name == "scaling":
            p = np.asarray(scaling, F).reshape(N, 3).copy()
        elif name == "opacity":
            p = np.asarray(opacity, F).reshape(N, 1).copy()
        elif name == "f_dc":
            p[:, 0] = np.arange(N, dtype=F)
        m = (rng.normal(0.0, 1.0, (N, M)).astype(F) + F(3)) if moments else None
        v = (rng.uniform(0.5, 2.0, (N, M)).astype(F)) if moments else None
        groups[name] = (p, m, v)
    return groups
