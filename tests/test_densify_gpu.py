"""Densify-and-prune on the MI355X (csrc/densify.hip; include/gsr.h is the definition) against the NumPy restatement
(tests/ref_densify.py).

EQUAL, no tolerance: counts, parent, the segment order, every copied parameter bit, every moment bit of kept rows, zeros on
new rows, guard floats, the sources, and the bytes the ctypes and the compiled binding produce.  The decisions rest on expf,
which NumPy and the device need not round alike, so the inputs are drawn with every compared quantity (|g|, smax, op, the
child's smax) at least 1e-4 relative from its threshold -- asserted in binary64 for every row of every case: the share of
rows left out of a comparison is zero.

Within a bound of the binary64 evaluation: the computed child values.  Scaling: 4 * 2^-23 * max(1, |value|) (expf, one
division, logf, each <= 1 ulp; doubled).  Position component k: 16 * 2^-23 * (|xyz_k| + sum_j |v_j|) (the normalisation,
nine entries of <= 6 roundings each, three products, three sums; about twice the count).  The worst observed ratios to
these bounds are printed by test_worst_child_ratios.  Should a bound ever be exceeded, the finding is which operation
differs; the bound is not to be widened without that.

Buffers are carved from larger tensors with 64 guard floats on each side, as tests/test_optim_gpu.py carves them."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import ref_densify as rd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL = -777.25
NAMES = rd.NAMES
MS = dict(zip(NAMES, rd.MODEL_M))
SHAPES = dict(zip(NAMES, ((3,), (1, 3), (15, 3), (1,), (3,), (4,))))
ROLES = {"xyz": "xyz", "scaling": "scaling"}
T = rd.THRESHOLDS
SCAN_THREADS, BLOCK = 256, 256  # densify.hip: the block-total scan's workgroup, Gaussians per workgroup
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1025, SCAN_THREADS * BLOCK + 257]
WORST = {"scaling": 0.0, "position": 0.0}


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def carve(a, dev, misalign=0):
    """-> (view, buffer): ``a`` on the device as a contiguous view ``misalign`` floats past the 64-float front guard."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((GUARD + misalign + a.size + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[GUARD + misalign:GUARD + misalign + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view, buf


def carve_out(shape, dev, misalign=0):
    return carve(np.full(shape, 12345.0, np.float32), dev, misalign)


def guards_intact(buf, n, misalign=0):
    b = buf.cpu().numpy()
    return bool((b[:GUARD + misalign] == np.float32(SENTINEL)).all() and (b[GUARD + misalign + n:] == np.float32(SENTINEL)).all())


def patterns(rng, N):
    i = np.arange(N)
    first = np.full(N, rd.PRUNE)
    first[0] = rd.SPLIT
    last = np.full(N, rd.KEEP)
    last[-1] = rd.CLONE
    last_only = np.full(N, rd.PRUNE)
    last_only[-1] = rd.KEEP
    return {"kept": np.full(N, rd.KEEP), "pruned": np.full(N, rd.PRUNE), "cloned": np.full(N, rd.CLONE),
            "split": np.full(N, rd.SPLIT), "alternating": np.where(i % 2 == 0, np.where(i % 4 == 0, rd.SPLIT, rd.CLONE), rd.KEEP),
            "runs64": np.array([rd.SPLIT, rd.KEEP, rd.CLONE, rd.PRUNE])[((i + 3) // 64) % 4], "random": rng.integers(0, 7, N),
            "first": first, "last": last, "last_only": last_only}


def draw(rng, action):
    """Inputs of a case, the margin condition asserted for every row, model groups and noise."""
    N = action.size
    inp = rd.make_inputs(rng, action)
    groups = rd.make_model(rng, N, inp["scaling"], inp["opacity"])
    noise = rng.normal(0.0, 1.0, (N, 2, 3)).astype(np.float32)
    return inp, groups, noise


def assert_margins(inp):
    dl, wl = rd.limits()
    m = rd.margins(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], T["grad_threshold"], T["min_opacity"], dl, wl)
    assert (m >= rd.MARGIN).all(), "an input row sits on a threshold: the share of rows left out must be zero"


def within(got, want64, bound, what):
    """NaN exactly where the binary64 evaluation has NaN; elsewhere inside the bound.  -> the worst ratio to the bound."""
    nan = np.isnan(want64)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN placement")
    if nan.all():
        return 0.0
    ratio = np.abs(got.astype(np.float64) - want64)[~nan] / bound[~nan]
    assert (ratio <= 1.0).all(), f"{what}: {ratio.max():.3f} x the bound"
    return float(ratio.max())


def run_case(dev, inp, groups, noise, world_on, binding="auto", moments=True, misalign=None):
    """plan -> read counts -> apply on carved buffers.  -> (counts, parent, {name: (param, m, v)}) as numpy, with guards, the
    sources and the workspace's surroundings checked."""
    from gsworld_amd import _C

    N = noise.shape[0]
    misalign = misalign or {}
    dl, wl = rd.limits()
    src, bufs = {}, []

    def put(key, a, mis=0):
        v, b = carve(a, dev, mis)
        src[key] = (v, np.ascontiguousarray(a, dtype=np.float32))
        bufs.append((b, a.size, mis))
        return v

    accum, denom = put("accum", inp["accum"]), put("denom", inp["denom"])
    nz = put("noise", noise)
    g = {}
    for n in NAMES:
        mis = misalign.get(n, 0)
        p, m, v = groups[n]
        g[n] = (put(n, p, mis), put(n + ".m", m, mis) if moments else None, put(n + ".v", v, mis) if moments else None)
    nbytes = _C.densify_workspace_bytes(N)
    wsbuf = torch.full((nbytes + 512,), 0xAB, dtype=torch.uint8, device=dev)
    ws = wsbuf[256:256 + nbytes]
    cbuf = torch.full((12,), -5, dtype=torch.int32, device=dev)
    counts_dev, _ = _C.densify_plan(accum, denom, g["scaling"][0], g["opacity"][0], grad_threshold=T["grad_threshold"],
                                    min_opacity=T["min_opacity"], dense_limit=dl, world_limit=wl, prune_world_size=world_on,
                                    counts=cbuf[4:8], workspace=ws, binding=binding)
    counts = tuple(int(c) for c in counts_dev.tolist())
    assert (cbuf[:4] == -5).all() and (cbuf[8:] == -5).all()
    n_out = counts[3]
    dst, call = {}, []
    for n in NAMES:
        mis = misalign.get(n, 0)
        outs = [carve_out((n_out, MS[n]), dev, mis) for _ in range(3 if moments else 1)]
        dst[n] = outs
        call.append({"src": g[n], "dst": tuple(o[0] for o in outs) + ((None, None) if not moments else ()), "M": MS[n],
                     "role": ROLES.get(n, "copy")})
    parent = torch.full((n_out + 2 * GUARD,), -9, dtype=torch.int32, device=dev)
    _C.densify_apply(N, n_out, ws, g["xyz"][0], g["scaling"][0], g["rotation"][0], nz, call, parent[GUARD:GUARD + n_out],
                     binding=binding)
    torch.cuda.synchronize()
    assert (parent[:GUARD] == -9).all() and (parent[GUARD + n_out:] == -9).all()
    assert (wsbuf[:256] == 0xAB).all() and (wsbuf[256 + nbytes:] == 0xAB).all()
    for b, size, mis in bufs:
        assert guards_intact(b, size, mis)
    for key, (v, a) in src.items():
        np.testing.assert_array_equal(rd.bits(v.cpu().numpy()), rd.bits(a), err_msg=f"source {key} was modified")
    out = {}
    for n in NAMES:
        for _, b in dst[n]:
            assert guards_intact(b, n_out * MS[n], misalign.get(n, 0)), f"guards of {n}"
        arrs = [o[0].cpu().numpy() for o in dst[n]]
        out[n] = tuple(arrs) if moments else (arrs[0], None, None)
    return counts, parent[GUARD:GUARD + n_out].cpu().numpy(), out


def check_case(got, inp, groups, noise, world_on, moments=True, what=""):
    counts, parent, out = got
    dl, wl = rd.limits()
    pl = rd.plan(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], T["grad_threshold"], T["min_opacity"], dl, wl, world_on)
    assert counts == pl["counts"], f"{what}: counts"
    K, Cn, S, n_out = counts
    np.testing.assert_array_equal(parent, pl["parent"], err_msg=f"{what}: parent")
    for a, b in ((0, K), (K, K + Cn), (K + Cn, K + Cn + S), (K + Cn + S, n_out)):  # four segments, each ascending
        assert (np.diff(parent[a:b]) > 0).all()
    src = {n: (groups[n][0], groups[n][1] if moments else None, groups[n][2] if moments else None) for n in NAMES}
    want = rd.apply(pl, src, noise)
    computed = np.zeros(n_out, bool)
    computed[K + Cn:] = True
    for n in NAMES:
        skip = computed if n in ROLES else np.zeros(n_out, bool)
        np.testing.assert_array_equal(rd.bits(out[n][0])[~skip], rd.bits(want[n][0])[~skip], err_msg=f"{what}: {n}")
        if moments:
            for j, key in ((1, "exp_avg"), (2, "exp_avg_sq")):
                np.testing.assert_array_equal(rd.bits(out[n][j]), rd.bits(want[n][j]), err_msg=f"{what}: {n} {key}")
                assert not rd.bits(out[n][j])[K:].any(), "new rows start with zero moments (+0.0)"
    for rows, pos, pb, cs, sb in rd.child_bounds(pl, src, noise):
        WORST["position"] = max(WORST["position"], within(out["xyz"][0][rows], pos, pb, f"{what}: child position"))
        WORST["scaling"] = max(WORST["scaling"], within(out["scaling"][0][rows], cs, sb, f"{what}: child scaling"))
    return pl


# ---- the kernels against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_every_pattern_world_prune_on_and_off(cuda_device, N):
    """Ten patterns x world-size prune on / off, the six model groups, with moments (and, for every other pattern, without)."""
    rng = np.random.default_rng(4000 + N)
    big = N > 2000
    for k, (pname, action) in enumerate(patterns(rng, N).items()):
        if big and pname != "random":
            continue  # (the large size is about the carry of the block-total scan; the small sizes cover every pattern)
        inp, groups, noise = draw(rng, action)
        assert_margins(inp)
        for world_on in (True, False):
            moments = not (k % 2 == 1 and world_on)
            got = run_case(cuda_device, inp, groups, noise, world_on, moments=moments)
            pl = check_case(got, inp, groups, noise, world_on, moments=moments, what=f"N={N} {pname} world={world_on}")
            K, Cn, S, n_out = pl["counts"]
            if pname == "kept":
                assert (K, Cn, S) == (N, 0, 0)
            if pname == "pruned":
                assert n_out == 0 and all(got[2][n][0].shape == (0, MS[n]) for n in NAMES)
            if pname == "cloned":
                assert (K, Cn, S) == (N, N, 0)
            if pname == "split":
                assert (K, Cn, S) == (0, 0, N)
            if pname == "first":
                assert (K, Cn, S) == (0, 0, 1)
            if pname == "last":
                assert (K, Cn, S) == (N, 1, 0) and got[1][-1] == N - 1
            if pname == "last_only":
                assert (K, Cn, S) == (1, 0, 0) and got[1][0] == N - 1


def test_random_pattern_takes_every_branch(cuda_device):
    """The random pattern at N = 1025 with the world-size prune on: kept, pruned by opacity, cloned, cloned by norm only (a
    negative quotient), split, too large (self and children), between (children only) all occur."""
    N = 1025
    rng = np.random.default_rng(4000 + N)
    action = patterns(rng, N)["random"]
    assert set(action.tolist()) == set(range(7))
    inp, groups, noise = draw(rng, action)
    dl, wl = rd.limits()
    on = rd.plan(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], T["grad_threshold"], T["min_opacity"], dl, wl, True)
    off = rd.plan(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], T["grad_threshold"], T["min_opacity"], dl, wl, False)
    assert off["counts"][0] > on["counts"][0] and off["counts"][2] > on["counts"][2] > 0 and on["counts"][1] > 0
    assert (on["clone"] & (inp["accum"][:, 0] < 0)).any() and (on["split"] & ~off["keep"] & (action == rd.MID)).any()


def test_nan_scale_nan_opacity_and_zero_denominator(cuda_device):
    """Rows with a NaN scale (the max propagates it: neither small nor too large -- split when hot, else kept), a NaN opacity
    (never below min_opacity: not pruned by it) and denom = 0 (0 / 0 -> NaN -> 0: cold; x / 0 -> inf: hot)."""
    N = 257
    rng = np.random.default_rng(77)
    action = rng.integers(0, 7, N)
    inp, groups, noise = draw(rng, action)
    nan = np.float32(np.nan)
    inp["scaling"][[3, 64, 200], [0, 2, 1]] = nan
    inp["scaling"][100] = nan
    inp["accum"][[3, 100]] = 1.0  # hot
    inp["accum"][[64, 200]] = 0.0
    inp["opacity"][[5, 3, 129, 256]] = nan
    inp["opacity"][[100, 64, 200, 8]] = 2.0
    inp["denom"][[7, 8, 255, 64]] = 0.0
    inp["accum"][[7, 255]] = 0.0
    inp["accum"][8] = 0.5
    inp["scaling"][8] = np.log(0.01)
    groups["scaling"] = (inp["scaling"].copy(),) + groups["scaling"][1:]
    groups["opacity"] = (inp["opacity"].copy(),) + groups["opacity"][1:]
    assert_margins(inp)
    for world_on in (True, False):
        got = run_case(cuda_device, inp, groups, noise, world_on)
        pl = check_case(got, inp, groups, noise, world_on, what=f"special values world={world_on}")
        assert pl["split"][[3, 100]].all() and pl["keep"][[64, 200]].all() and not pl["split"][[64, 200]].any()
        assert not (pl["clone"][7] or pl["split"][7]) and pl["clone"][8] and pl["keep"][8]


def test_without_moments_and_misaligned_groups(cuda_device):
    """Groups that never stepped (NULL moments), and groups carved one / two / three floats off 16-byte alignment (walked
    element by element) next to aligned ones: the same rows."""
    N = 333
    rng = np.random.default_rng(91)
    inp, groups, noise = draw(rng, rng.integers(0, 7, N))
    assert_margins(inp)
    base = run_case(cuda_device, inp, groups, noise, True)
    check_case(base, inp, groups, noise, True, what="aligned")
    for misalign in ({"f_rest": 1}, {"xyz": 3, "scaling": 2, "opacity": 1}, dict.fromkeys(NAMES, 1)):
        for moments in (True, False):
            got = run_case(cuda_device, inp, groups, noise, True, moments=moments, misalign=misalign)
            check_case(got, inp, groups, noise, True, moments=moments, what=f"misaligned {misalign} moments={moments}")
            for n in NAMES:  # the vector and the element path compute the same bytes, children included
                np.testing.assert_array_equal(rd.bits(got[2][n][0]), rd.bits(base[2][n][0]))


@pytest.mark.parametrize("N", [65, 1025])
def test_ctypes_and_compiled_binding_give_the_same_bytes(cuda_device, N):
    rng = np.random.default_rng(300 + N)
    inp, groups, noise = draw(rng, rng.integers(0, 7, N))
    assert_margins(inp)
    a = run_case(cuda_device, inp, groups, noise, True, binding="ext")
    b = run_case(cuda_device, inp, groups, noise, True, binding="ctypes")
    check_case(a, inp, groups, noise, True, what="ext")
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for n in NAMES:
        for x, y in zip(a[2][n], b[2][n]):
            np.testing.assert_array_equal(rd.bits(x), rd.bits(y), err_msg=n)


def test_neither_call_synchronises(cuda_device):
    """plan and apply each under torch.cuda.set_sync_debug_mode("error"); the single read of counts sits between them."""
    from gsworld_amd import _C

    dev = cuda_device
    N = 1025
    rng = np.random.default_rng(55)
    inp, groups, noise = draw(rng, rng.integers(0, 7, N))
    t = {n: tuple(torch.from_numpy(a).to(dev) for a in groups[n]) for n in NAMES}
    accum, denom, nz = (torch.from_numpy(a).to(dev) for a in (inp["accum"], inp["denom"], noise))
    dl, wl = rd.limits()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        counts_dev, ws = _C.densify_plan(accum, denom, t["scaling"][0], t["opacity"][0], grad_threshold=T["grad_threshold"],
                                         min_opacity=T["min_opacity"], dense_limit=dl, world_limit=wl, prune_world_size=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    counts = counts_dev.tolist()
    n_out = counts[3]
    dst = {n: tuple(torch.empty((n_out, MS[n]), device=dev) for _ in range(3)) for n in NAMES}
    parent = torch.empty((n_out,), dtype=torch.int32, device=dev)
    call = [{"src": t[n], "dst": dst[n], "M": MS[n], "role": ROLES.get(n, "copy")} for n in NAMES]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _C.densify_apply(N, n_out, ws, t["xyz"][0], t["scaling"][0], t["rotation"][0], nz, call, parent)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = (tuple(counts), parent.cpu().numpy(), {n: tuple(x.cpu().numpy() for x in dst[n]) for n in NAMES})
    check_case(got, inp, groups, noise, True, what="sync debug mode")


# ---- the public interface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "sparse_adam", "fresh", "none"])
def test_optim_densify_and_prune(cuda_device, kind):
    """gsworld_amd.optim.densify_and_prune with torch.optim.Adam, SparseGaussianAdam, an optimizer that never stepped and no
    optimizer: fresh nn.Parameters of N_out rows, state re-keyed, ``step`` kept, moments only where there were any."""
    from gsworld_amd.optim import SparseGaussianAdam, densify_and_prune

    dev = cuda_device
    N = 700
    rng = np.random.default_rng(123)
    inp, groups, noise = draw(rng, rng.integers(0, 7, N))
    assert_margins(inp)
    params = {n: torch.nn.Parameter(torch.from_numpy(groups[n][0]).to(dev).view((N,) + SHAPES[n]).contiguous()) for n in NAMES}
    opt = None
    if kind != "none":
        pg = [{"params": [params[n]], "lr": 1e-3, "name": n} for n in NAMES]
        opt = SparseGaussianAdam(pg, lr=0.0, eps=1e-15) if kind == "sparse_adam" else torch.optim.Adam(pg, lr=0.0, eps=1e-15)
    stepped = kind in ("adam", "sparse_adam")
    if stepped:
        for n in NAMES:
            opt.state[params[n]] = {"step": torch.tensor(7.0),
                                    "exp_avg": torch.from_numpy(groups[n][1]).to(dev).view(params[n].shape).clone(),
                                    "exp_avg_sq": torch.from_numpy(groups[n][2]).to(dev).view(params[n].shape).clone()}
    old = dict(params)
    new, counts, parent = densify_and_prune(params, opt, torch.from_numpy(inp["accum"]).to(dev),
                                            torch.from_numpy(inp["denom"]).to(dev), grad_threshold=T["grad_threshold"],
                                            min_opacity=T["min_opacity"], extent=T["extent"], percent_dense=T["percent_dense"],
                                            prune_world_size=True, noise=torch.from_numpy(noise).to(dev))
    assert all(isinstance(c, int) for c in counts) and parent.dtype == torch.int32 and parent.shape == (counts[3],)
    out = {}
    for k, n in enumerate(NAMES):
        prm = new[n]
        assert isinstance(prm, torch.nn.Parameter) and prm.requires_grad and prm.shape == (counts[3],) + SHAPES[n]
        m = v = None
        if opt is not None:
            assert opt.param_groups[k]["params"][0] is prm and old[n] not in opt.state
            st = opt.state.get(prm)
            if stepped:
                assert float(st["step"]) == 7.0
                m, v = st["exp_avg"], st["exp_avg_sq"]
                assert m.shape == prm.shape and v.shape == prm.shape
            else:
                assert not st
        host = lambda x: None if x is None else x.detach().cpu().numpy().reshape(counts[3], MS[n])  # noqa: E731
        out[n] = (host(prm), host(m), host(v))
    check_case((counts, parent.cpu().numpy(), out), inp, groups, noise, True, moments=stepped, what=kind)
    # a side array carried along by parent
    labels = torch.arange(N, device=dev)
    assert torch.equal(labels[parent.long()].float(), new["f_dc"].detach()[:, 0, 0])
    if kind == "none":  # noise drawn inside: the same decisions, other children
        again, counts2, parent2 = densify_and_prune(old, None, torch.from_numpy(inp["accum"]).to(dev),
                                                    torch.from_numpy(inp["denom"]).to(dev), grad_threshold=T["grad_threshold"],
                                                    min_opacity=T["min_opacity"], extent=T["extent"],
                                                    percent_dense=T["percent_dense"], prune_world_size=True,
                                                    generator=torch.Generator(device=dev).manual_seed(3))
        assert counts2 == counts and torch.equal(parent2, parent)
        K, Cn, S, _ = counts
        assert torch.equal(again["xyz"][:K + Cn], new["xyz"][:K + Cn]) and not torch.equal(again["xyz"][K + Cn:], new["xyz"][K + Cn:])


# ---- GaussianModel ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gs_paths():
    added = [os.path.join(ROOT, "gsworld_amd", "dropin"), os.path.join(ROOT, "gsworld_amd", "gs_compat")]
    for p in added:
        sys.path.insert(0, p)
    yield
    for p in added:
        sys.path.remove(p)
    for m in [k for k in sys.modules if k.split(".")[0] in ("scene", "gaussian_renderer", "arguments", "utils",
                                                            "diff_gaussian_rasterization", "simple_knn", "fused_ssim")]:
        del sys.modules[m]


PERCENT_DENSE = 0.08
TRAIN_ARGS = types.SimpleNamespace(percent_dense=PERCENT_DENSE, position_lr_init=1.6e-4, feature_lr=2.5e-3, opacity_lr=2.5e-2,
                                   scaling_lr=5e-3, rotation_lr=1e-3)


def model_from(cls, raw, dev):
    pc = cls(3, "sparse_adam")
    P = torch.nn.Parameter
    pc._xyz, pc._features_dc, pc._features_rest = P(raw.xyz.to(dev)), P(raw.features_dc.to(dev).contiguous()), \
        P(raw.features_rest.to(dev).contiguous())
    pc._opacity, pc._scaling, pc._rotation = P(raw.opacity.to(dev)), P(raw.scaling.to(dev)), P(raw.rotation.to(dev))
    pc.active_sh_degree = 3
    pc.spatial_lr_scale = 1.0
    pc.training_setup(TRAIN_ARGS)
    return pc


def between(values, q):
    """A threshold inside a gap of at least 1e-3 relative between two neighbours of the sorted positive ``values``, at or
    after quantile ``q``: no value sits within 1e-4 of it."""
    v = np.sort(np.asarray(values, np.float64))
    v = v[v > 0]
    for i in range(int(q * v.size), v.size - 1):
        if v[i + 1] - v[i] > 2e-3 * v[i]:
            return float(np.float32(0.5 * (v[i] + v[i + 1])))
    raise AssertionError("no gap")


def pick_extent(smax, q=0.5):
    """An extent whose dense limit (PERCENT_DENSE x extent) splits the sorted ``smax`` at or after quantile ``q`` inside a gap,
    and whose world limit (0.1 x extent) is no closer than 2e-4 relative to any smax or child smax (smax / 1.6) either."""
    v = np.sort(np.asarray(smax, np.float64))
    one6 = float(np.float32(1.6))
    for i in range(int(q * v.size), v.size - 1):
        if v[i + 1] - v[i] <= 2e-3 * v[i]:
            continue
        extent = float(np.float32(0.5 * (v[i] + v[i + 1]) / PERCENT_DENSE))
        dl = float(np.float32(PERCENT_DENSE) * np.float32(extent))
        wl = float(np.float32(0.1) * np.float32(extent))
        if min(np.abs(v - dl).min() / dl, np.abs(v - wl).min() / wl, np.abs(v / one6 - wl).min() / wl) >= 2e-4:
            return extent
    raise AssertionError("no extent")


def test_model_densify_and_prune_between_training_iterations(cuda_device, gs_paths):
    """GaussianModel(3, "sparse_adam"), 2 000 Gaussians, a 64 x 64 view: three iterations, densify_and_prune, three more.
    The fused route is taken; parameters, moments and side arrays have N_out rows; ``step`` survives; new rows' moments are
    zero before the next step and move with it where a row is visible; a subclass overriding the hooks, started from the
    same state, gives the same counts and order through the literal sequence."""
    from gaussian_renderer import render
    from scene.gaussian_model import GaussianModel

    from gsworld_amd import scenes
    from gsworld_amd.ssim import photometric_loss

    class Hooked(GaussianModel):
        hooks = 0

        def prune_points(self, mask):
            self.hooks += 1
            super().prune_points(mask)

        def densification_postfix(self, *args):
            self.hooks += 1
            super().densification_postfix(*args)

    dev = cuda_device
    N, S = 2000, 64
    raw = scenes.random_scene_camera_frame(N, seed=6)
    pc = model_from(GaussianModel, raw, dev)
    cam = scenes.identity_camera(S, S, 60.0).to(dev)
    pipe = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, antialiasing=False)
    bg = torch.zeros(3, device=dev)
    gt = torch.rand(3, S, S, generator=torch.Generator().manual_seed(8)).to(dev)

    def iterate(model, n):
        for _ in range(n):
            out = render(cam, model, pipe, bg)
            photometric_loss(out["render"], gt, 0.2).backward()
            model.add_densification_stats(out["viewspace_points"], out["radii"])
            model.optimizer.step(out["radii"], model.get_xyz.shape[0])
            model.optimizer.zero_grad(set_to_none=True)
        return out["radii"]

    radii = iterate(pc, 3)
    # thresholds from the state itself, each inside a gap of the values it is compared with
    accum, denom = pc.xyz_gradient_accum.cpu().numpy(), pc.denom.cpu().numpy()
    scaling, opacity = pc._scaling.detach().cpu().numpy(), pc._opacity.detach().cpu().numpy()
    seen = denom[:, 0] > 0
    assert 100 < seen.sum() < N
    max_grad = between((accum[seen] / denom[seen]).reshape(-1), 0.5)
    smax = np.exp(scaling.astype(np.float64)).max(axis=1)
    extent = pick_extent(smax)
    min_opacity = between(1.0 / (1.0 + np.exp(-opacity.astype(np.float64))).reshape(-1), 0.1)
    dl, wl = np.float32(PERCENT_DENSE) * np.float32(extent), np.float32(0.1) * np.float32(extent)
    assert (rd.margins(accum, denom, scaling, opacity, max_grad, min_opacity, dl, wl) >= rd.MARGIN).all()
    pl = rd.plan(accum, denom, scaling, opacity, max_grad, min_opacity, dl, wl, True)
    K, Cn, Sp, n_out = pl["counts"]
    assert 0 < K < N and Cn > 20 and Sp > 20 and n_out != N
    assert (smax > float(wl)).any(), "the world-size prune must act"

    # the same state in a model whose class overrides the hooks
    hooked = model_from(Hooked, raw, dev)
    for n in NAMES:
        a, b = pc._current()[n], hooked._current()[n]
        b.data.copy_(a.data)
        hooked.optimizer.state[b] = {k: v.clone() for k, v in pc.optimizer.state[a].items()}
    hooked.xyz_gradient_accum, hooked.denom = pc.xyz_gradient_accum.clone(), pc.denom.clone()
    hooked.max_radii2D = pc.max_radii2D.clone()
    noise = torch.randn(N, 2, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    before = {n: (t.detach().cpu().numpy().reshape(N, -1), pc.optimizer.state[t]["exp_avg"].cpu().numpy().reshape(N, -1),
                  pc.optimizer.state[t]["exp_avg_sq"].cpu().numpy().reshape(N, -1)) for n, t in pc._current().items()}
    steps = {n: float(pc.optimizer.state[t]["step"]) for n, t in pc._current().items()}

    pc.densify_and_prune(max_grad, min_opacity, extent, 20, radii, noise=noise)
    hooked.densify_and_prune(max_grad, min_opacity, extent, 20, radii, noise=noise)
    assert pc.last_densify_route == "fused" and hooked.last_densify_route == "literal" and hooked.hooks == 4
    want = rd.apply(pl, before, noise.cpu().numpy())
    bounds = rd.child_bounds(pl, before, noise.cpu().numpy())
    new = np.zeros(n_out, bool)
    new[K + Cn:] = True
    for model in (pc, hooked):
        assert model.get_xyz.shape[0] == n_out
        assert model.xyz_gradient_accum.shape == (n_out, 1) and not model.xyz_gradient_accum.any()
        assert model.denom.shape == (n_out, 1) and not model.denom.any()
        assert model.max_radii2D.shape == (n_out,) and not model.max_radii2D.any() and model.tmp_radii is None
        for k, n in enumerate(NAMES):
            prm = model._current()[n]
            assert prm.shape == (n_out,) + SHAPES[n] and model.optimizer.param_groups[k]["params"][0] is prm
            st = model.optimizer.state[prm]
            assert float(st["step"]) == steps[n]
            skip = new if n in ROLES else np.zeros(n_out, bool)
            got = prm.detach().cpu().numpy().reshape(n_out, -1)
            np.testing.assert_array_equal(rd.bits(got)[~skip], rd.bits(want[n][0])[~skip], err_msg=n)
            for j, key in ((1, "exp_avg"), (2, "exp_avg_sq")):
                assert st[key].shape == prm.shape
                np.testing.assert_array_equal(rd.bits(st[key].cpu().numpy().reshape(n_out, -1)), rd.bits(want[n][j]))
        for rows, pos, pb, cs, sb in bounds:
            within(model._xyz.detach().cpu().numpy()[rows], pos, pb, "child position")
            within(model._scaling.detach().cpu().numpy()[rows], cs, sb, "child scaling")

    # training goes on at the new size; new rows' moments move where the rows are seen
    radii2 = iterate(pc, 1).cpu().numpy()
    fresh_seen = (radii2 > 0)[K:]
    m = pc.optimizer.state[pc._xyz]["exp_avg_sq"].cpu().numpy()[K:]
    assert fresh_seen.any() and (m[fresh_seen] != 0).any() and not m[~fresh_seen].any()
    iterate(pc, 2)
    assert pc.get_xyz.shape[0] == n_out and float(pc.denom.max()) == 3.0


def test_reset_opacity_on_the_device(cuda_device, gs_paths):
    """opacity = inverse_sigmoid(min(sigmoid(o), 0.01)) within the logf bound 4 * 2^-23 * max(1, |value|) of the binary64
    evaluation (a sigmoid, a subtraction, a division and a log: ~3e-7 relative in the log's argument, half an ulp of the
    result); the opacity moments are zero, every other group keeps its tensors."""
    from scene.gaussian_model import GaussianModel

    from gsworld_amd import scenes

    dev = cuda_device
    N = 3000
    pc = model_from(GaussianModel, scenes.random_scene_camera_frame(N, seed=9), dev)
    with torch.no_grad():
        pc._opacity[::3] -= 6.0  # a third below 0.01
    for t in pc._current().values():
        pc.optimizer.state[t] = {"step": torch.tensor(5.0), "exp_avg": torch.ones_like(t), "exp_avg_sq": torch.ones_like(t)}
    others = {n: t for n, t in pc._current().items() if n != "opacity"}
    o = pc._opacity.detach().cpu().numpy().astype(np.float64)
    pc.reset_opacity()
    x = np.minimum(1.0 / (1.0 + np.exp(-o)), float(np.float32(0.01)))
    want = np.log(x / (1.0 - x))
    got = pc._opacity.detach().cpu().numpy()
    assert got.shape == (N, 1) and (x < 0.0099).sum() > 100 and (x == float(np.float32(0.01))).sum() > 100
    ratio = np.abs(got - want) / (4 * rd.U * np.maximum(1.0, np.abs(want)))
    print(f"reset_opacity: worst ratio to the bound {ratio.max():.3f}")
    assert (ratio <= 1.0).all()
    st = pc.optimizer.state[pc._opacity]
    assert pc.optimizer.param_groups[3]["params"][0] is pc._opacity and float(st["step"]) == 5.0
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    for n, t in others.items():
        assert pc._current()[n] is t and pc.optimizer.state[t]["exp_avg"].all()


def test_worst_child_ratios():
    """(Runs last: prints what the cases above observed.)"""
    print(f"worst ratio to the bound: child scaling {WORST['scaling']:.3f}, child position {WORST['position']:.3f}")
    assert WORST["scaling"] <= 1.0 and WORST["position"] <= 1.0
