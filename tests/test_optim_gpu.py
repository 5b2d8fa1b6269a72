"""The optimizer step and the densification statistics on the MI355X (csrc/optim.hip; include/gsr.h is the definition),
held BIT FOR BIT to the float32 restatement (tests/ref_optim.py): the operations are IEEE binary32 add / mul / div / sqrt,
correctly rounded on both sides, contraction off, denormals kept -- no tolerance anywhere in this file.

Buffers are carved from larger tensors with 64 guard floats on each side; the guards must come back unchanged.

On the MI355X the equality holds for every case below.  Should one ever fail, the finding is which operation differs, with
its operands; the comparison is not to be loosened."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import ref_optim as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL = -777.25
MODEL_M = (3, 3, 45, 1, 3, 4)  # xyz, f_dc, f_rest, opacity, scaling, rotation
MODEL_SHAPES = ((3,), (1, 3), (15, 3), (1,), (3,), (4,))
MODEL_LR = (1.6e-4, 2.5e-3, 1.25e-4, 2.5e-2, 5e-3, 1e-3)
EPS = 1e-15


# ---- helpers ----------------------------------------------------------------------------------------------------------
def carve(a: np.ndarray, dev, misalign: int = 0):
    """-> (view, buffer): ``a`` on the device as a contiguous view ``misalign`` floats past the 64-float front guard."""
    a = np.ascontiguousarray(a)
    buf = torch.full((GUARD + misalign + a.size + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[GUARD + misalign:GUARD + misalign + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (misalign % 4 == 0)
    return view, buf


def guards_intact(buf, n: int, misalign: int = 0) -> bool:
    b = buf.cpu().numpy()
    return bool((b[:GUARD + misalign] == np.float32(SENTINEL)).all() and (b[GUARD + misalign + n:] == np.float32(SENTINEL)).all())


def make_group(rng, N: int, M: int):
    """p, g, m, v (N, M) float32: |g| log-uniform over 1e-8 .. 1e2 with zeros, moments of matching size, m = v = 0 on every
    fifth element (a Gaussian's first sight)."""
    n = N * M
    g = (10.0 ** rng.uniform(-8, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0.0
    m = (g * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    v = (g.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    m[::5] = 0.0
    v[::5] = 0.0
    p = rng.normal(0.0, 1.0, n).astype(np.float32)
    return tuple(a.reshape(N, M) for a in (p, g, m, v))


def patterns(rng, N: int) -> dict:
    i = np.arange(N)
    first, last = np.zeros(N, bool), np.zeros(N, bool)
    first[0], last[-1] = True, True
    return {"all": np.ones(N, bool), "none": np.zeros(N, bool), "first": first, "last": last, "alternating": i % 2 == 0,
            "runs64": ((i + 3) // 64) % 2 == 0, "random": rng.random(N) < 0.3}


def forms(rng, vis: np.ndarray, dev) -> dict:
    """The same visibility as a bool mask, a uint8 mask (any nonzero byte), int32 radii (zeros and negatives invisible) and,
    when everything is visible, None."""
    N = vis.size
    u8 = np.where(vis, rng.choice(np.array([1, 2, 7, 128, 255], np.uint8), N), 0).astype(np.uint8)
    radii = np.where(vis, rng.integers(1, 500, N), rng.choice(np.array([0, 0, -1, -2_000_000_000]), N)).astype(np.int32)
    out = {"bool": torch.from_numpy(vis.copy()).to(dev), "uint8": torch.from_numpy(u8).to(dev),
           "radii": torch.from_numpy(radii).to(dev)}
    if vis.all():
        out["none"] = None
    return out


def run_group(dev, arrays, visible, lr=1e-3, eps=EPS, misalign=0, binding="auto", call=None):
    """One single-group update of carved copies of ``arrays``; -> (p, m, v) as numpy, guards checked."""
    from gsworld_amd import _C

    (p, pb), (g, gb), (m, mb), (v, vb) = (carve(a, dev, misalign) for a in arrays)
    N, M = arrays[0].shape
    if call is not None:
        call(p, g, m, v)
    else:
        _C.adam_update_groups([{"param": p, "grad": g, "exp_avg": m, "exp_avg_sq": v, "lr": lr, "eps": eps}], visible, N,
                              binding=binding)
    for b in (pb, gb, mb, vb):
        assert guards_intact(b, N * M, misalign)
    assert np.array_equal(ro.bits(g.cpu().numpy()), ro.bits(arrays[1])), "grad is read-only"
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def assert_bits(got, want, what=""):
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
        np.testing.assert_array_equal(ro.bits(a), ro.bits(b), err_msg=f"{what} {name}")


# ---- single groups ----------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 3), (5, 3), (63, 4), (64, 4), (65, 4), (257, 3), (333, 1), (70, 7), (129, 48), (100, 45), (1000, 45)]


@pytest.mark.parametrize("N,M", SHAPES)
def test_single_group_every_visibility_and_form(cuda_device, N, M):
    """Every visibility pattern in every form (bool, uint8, int32 radii, None) equals the restatement -- and so each other."""
    rng = np.random.default_rng(1000 * N + M)
    arrays = make_group(rng, N, M)
    for pname, vis in patterns(rng, N).items():
        want = ro.adam_f32(*arrays, vis, 1e-3, EPS)
        for fname, visible in forms(rng, vis, cuda_device).items():
            got = run_group(cuda_device, arrays, visible)
            assert_bits(got, want, f"({N},{M}) {pname}/{fname}")
            if not vis.any():  # nothing visible: nothing moved
                assert_bits(got, (arrays[0], arrays[2], arrays[3]), f"({N},{M}) {pname}/{fname} untouched")


@pytest.mark.parametrize("M", [3, 45])
@pytest.mark.parametrize("parity", [0, 1])
def test_vectors_straddling_gaussians_of_different_visibility(cuda_device, M, parity):
    """M no multiple of 4: 16-byte vectors span a visible and an invisible Gaussian.  Invisible rows hold NaN gradients; their
    param / moments keep their bits, visible rows equal the restatement (no NaN may appear anywhere in the outputs)."""
    N = 131
    rng = np.random.default_rng(7 + M + parity)
    p, g, m, v = make_group(rng, N, M)
    vis = (np.arange(N) + parity) % 2 == 0
    g = g.copy()
    g[~vis] = np.nan
    want = ro.adam_f32(p, g, m, v, vis, 1e-3, EPS)
    for fname, visible in forms(rng, vis, cuda_device).items():
        got = run_group(cuda_device, (p, g, m, v), visible)
        assert not any(np.isnan(a).any() for a in got)
        assert_bits(got, want, f"straddle M={M} parity={parity} {fname}")
        assert_bits([a[~vis] for a in got], [a[~vis] for a in (p, m, v)], "invisible rows")


@pytest.mark.parametrize("N,M", [(1000, 45), (257, 3)])
def test_misaligned_base(cuda_device, N, M):
    """The four arrays start one float into their buffers (4-byte aligned only): the element path, same bits."""
    rng = np.random.default_rng(N + M)
    arrays = make_group(rng, N, M)
    for pname in ("random", "alternating", "all"):
        vis = patterns(rng, N)[pname]
        want = ro.adam_f32(*arrays, vis, 1e-3, EPS)
        got = run_group(cuda_device, arrays, forms(rng, vis, cuda_device)["radii"], misalign=1)
        assert_bits(got, want, f"misaligned ({N},{M}) {pname}")
    # ... and a call whose arrays disagree in alignment (only the gradient is off)
    from gsworld_amd import _C

    vis = patterns(rng, N)["random"]
    want = ro.adam_f32(*arrays, vis, 1e-3, EPS)
    (p, pb), (m, mb), (v, vb) = (carve(arrays[k], cuda_device) for k in (0, 2, 3))
    g, gb = carve(arrays[1], cuda_device, misalign=3)
    _C.adam_update_groups([{"param": p, "grad": g, "exp_avg": m, "exp_avg_sq": v, "lr": 1e-3, "eps": EPS}],
                          torch.from_numpy(vis).to(cuda_device), N)
    assert_bits((p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()), want, "mixed alignment")
    assert all(guards_intact(b, N * M) for b in (pb, mb, vb)) and guards_intact(gb, N * M, 3)


def test_nonfinite_gradients_of_visible_gaussians_propagate(cuda_device):
    """The one test that feeds NaN / inf to VISIBLE rows: they propagate as the arithmetic says (NaN compared as NaN)."""
    rng = np.random.default_rng(3)
    p, g, m, v = make_group(rng, 50, 7)
    g = g.copy()
    g[3, 2], g[10, :], g[20, 0], g[21, 1] = np.nan, np.nan, np.inf, -np.inf
    vis = np.ones(50, bool)
    vis[10] = False
    want = ro.adam_f32(p, g, m, v, vis, 1e-3, EPS)
    got = run_group(cuda_device, (p, g, m, v), torch.from_numpy(vis).to(cuda_device))
    for a, b in zip(got, want):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_array_equal(ro.bits(a)[~np.isnan(b)], ro.bits(b)[~np.isnan(b)])
    assert np.isnan(got[0][3, 2]) and not np.isnan(got[0][10]).any()


# ---- the model's six groups ----------------------------------------------------------------------------------------------
def model_arrays(rng, N):
    return [make_group(rng, N, M) for M in MODEL_M]


@pytest.mark.parametrize("N", [1000, 200_003])
def test_six_groups_in_one_call(cuda_device, N):
    """One six-group call == six single-group calls == the restatement; each group its own lr, eps 1e-15, random visibility 0.3."""
    from gsworld_amd import _C

    rng = np.random.default_rng(N)
    groups = model_arrays(rng, N)
    vis = rng.random(N) < 0.3
    radii = forms(rng, vis, cuda_device)["radii"]
    want = [ro.adam_f32(*a, vis, lr, EPS) for a, lr in zip(groups, MODEL_LR)]
    carved = [[carve(x, cuda_device) for x in a] for a in groups]
    _C.adam_update_groups([{"param": c[0][0], "grad": c[1][0], "exp_avg": c[2][0], "exp_avg_sq": c[3][0], "lr": lr, "eps": EPS}
                           for c, lr in zip(carved, MODEL_LR)], radii, N)
    for k, (c, a, lr) in enumerate(zip(carved, groups, MODEL_LR)):
        got = tuple(c[i][0].cpu().numpy() for i in (0, 2, 3))
        assert_bits(got, want[k], f"group {k} of six")
        assert all(guards_intact(c[i][1], a[0].size) for i in range(4))
        assert_bits(run_group(cuda_device, a, radii, lr=lr), got, f"group {k} alone")


def make_optimizer(dev, arrays_per_group, with_grad=None):
    """SparseGaussianAdam over parameters of the model's shapes, gradients set from the arrays (``with_grad``: which groups)."""
    from gsworld_amd.optim import SparseGaussianAdam

    params = []
    for k, (a, shape) in enumerate(zip(arrays_per_group, MODEL_SHAPES)):
        prm = torch.nn.Parameter(torch.from_numpy(a[0].copy()).to(dev).view(-1, *shape))
        if with_grad is None or k in with_grad:
            prm.grad = torch.from_numpy(a[1].copy()).to(dev).view(-1, *shape)
        params.append(prm)
    opt = SparseGaussianAdam([{"params": [prm], "lr": lr, "name": str(k)} for k, (prm, lr) in enumerate(zip(params, MODEL_LR))],
                             lr=0.0, eps=EPS)
    return opt, params


def test_optimizer_skips_groups_without_gradient(cuda_device):
    N = 1000
    rng = np.random.default_rng(5)
    groups = model_arrays(rng, N)
    vis = rng.random(N) < 0.3
    opt, params = make_optimizer(cuda_device, groups, with_grad={0, 1, 3, 4, 5})  # f_rest has no gradient
    opt.step(torch.from_numpy(vis).to(cuda_device), N)
    for k, (a, lr) in enumerate(zip(groups, MODEL_LR)):
        got_p = params[k].detach().cpu().numpy().reshape(N, -1)
        if k == 2:
            np.testing.assert_array_equal(ro.bits(got_p), ro.bits(a[0]))
            assert len(opt.state[params[k]]) == 0
            continue
        z = np.zeros_like(a[0])
        want = ro.adam_f32(a[0], a[1], z, z, vis, lr, EPS)  # (state is created as zeros on first use)
        st = opt.state[params[k]]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        got = (got_p, st["exp_avg"].cpu().numpy().reshape(N, -1), st["exp_avg_sq"].cpu().numpy().reshape(N, -1))
        assert_bits(got, want, f"optimizer group {k}")


def test_three_steps_with_changing_visibility(cuda_device):
    """State and parameters match the restatement after every one of three steps; None / mask / radii in turn."""
    N = 777
    rng = np.random.default_rng(11)
    groups = model_arrays(rng, N)
    opt, params = make_optimizer(cuda_device, groups)
    ref = [(a[0], np.zeros_like(a[0]), np.zeros_like(a[0])) for a in groups]
    for step in range(3):
        vis = np.ones(N, bool) if step == 0 else rng.random(N) < (0.5 if step == 1 else 0.1)
        visible = [None, torch.from_numpy(vis).to(cuda_device), forms(rng, vis, cuda_device)["radii"]][step]
        grads = [make_group(rng, N, M)[1] for M in MODEL_M]
        for prm, g in zip(params, grads):
            prm.grad = torch.from_numpy(g).to(cuda_device).view(prm.shape)
        opt.step(visible, N)
        ref = [ro.adam_f32(r[0], g, r[1], r[2], vis, lr, EPS) for r, g, lr in zip(ref, grads, MODEL_LR)]
        for k, prm in enumerate(params):
            st = opt.state[prm]
            got = tuple(t.detach().cpu().numpy().reshape(N, -1) for t in (prm, st["exp_avg"], st["exp_avg_sq"]))
            assert_bits(got, ref[k], f"step {step} group {k}")


def test_noncontiguous_gradient_is_made_contiguous(cuda_device):
    N, rng = 300, np.random.default_rng(13)
    p, g, m, v = make_group(rng, N, 3)
    from gsworld_amd.optim import SparseGaussianAdam

    prm = torch.nn.Parameter(torch.from_numpy(p.copy()).to(cuda_device))
    wide = torch.zeros(N, 16, 3, device=cuda_device)
    wide[:, 0] = torch.from_numpy(g).to(cuda_device)
    prm.grad = wide[:, 0]
    assert not prm.grad.is_contiguous()
    opt = SparseGaussianAdam([{"params": [prm], "lr": 1e-3, "name": "x"}], lr=0.0, eps=EPS)
    opt.step(None, N)
    z = np.zeros_like(p)
    assert_bits((prm.detach().cpu().numpy(), opt.state[prm]["exp_avg"].cpu().numpy(), opt.state[prm]["exp_avg_sq"].cpu().numpy()),
                ro.adam_f32(p, g, z, z, None, 1e-3, EPS))
    with pytest.raises(RuntimeError):  # a non-contiguous parameter is refused, not copied
        bad = torch.nn.Parameter(wide[:, 1])
        bad.grad = torch.zeros_like(bad)
        SparseGaussianAdam([{"params": [bad], "lr": 1e-3}], lr=0.0, eps=EPS).step(None, N)


# ---- bindings ----------------------------------------------------------------------------------------------------------
def test_compiled_and_ctypes_bindings_give_the_same_bytes(cuda_device):
    rng = np.random.default_rng(17)
    arrays = make_group(rng, 1000, 45)
    vis = rng.random(1000) < 0.3
    radii = forms(rng, vis, cuda_device)["radii"]
    a = run_group(cuda_device, arrays, radii, lr=2.5e-3, binding="ext")
    b = run_group(cuda_device, arrays, radii, lr=2.5e-3, binding="ctypes")
    assert_bits(a, b, "ext vs ctypes")
    assert_bits(a, ro.adam_f32(*arrays, vis, 2.5e-3, EPS), "ext vs restatement")


def test_upstream_adamUpdate_signature(cuda_device):
    from gsworld_amd import _C

    rng = np.random.default_rng(19)
    N, M = 257, 3
    arrays = make_group(rng, N, M)
    vis = rng.random(N) < 0.5
    visible = torch.from_numpy(vis).to(cuda_device)
    got = run_group(cuda_device, arrays, None,
                    call=lambda p, g, m, v: _C.adamUpdate(p, g, m, v, visible, 1e-2, 0.9, 0.999, 1e-15, N, M))
    assert_bits(got, ro.adam_f32(*arrays, vis, 1e-2, 1e-15), "adamUpdate")
    # other betas travel too
    got = run_group(cuda_device, arrays, None,
                    call=lambda p, g, m, v: _C.adamUpdate(p, g, m, v, visible, 1e-2, 0.8, 0.99, 1e-8, N, M))
    assert_bits(got, ro.adam_f32(*arrays, vis, 1e-2, 1e-8, 0.8, 0.99), "adamUpdate betas")


# ---- densification statistics ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 64, 65, 1000, 100_003])
def test_densification_stats(cuda_device, N):
    from gsworld_amd import _C
    from gsworld_amd.optim import densification_stats

    rng = np.random.default_rng(N)
    radii = np.where(rng.random(N) < 0.4, rng.integers(1, 900, N), rng.choice(np.array([0, 0, -3]), N)).astype(np.int32)
    if N >= 64:
        radii[0], radii[-1] = 17, 0
    grad = (10.0 ** rng.uniform(-9, 1, (N, 3)) * rng.choice([-1.0, 1.0], (N, 3))).astype(np.float32)
    grad[:, 2] = np.nan  # the third column is never read
    grad[rng.random(N) < 0.1, :2] = 0.0
    accum = rng.uniform(0, 1, (N, 1)).astype(np.float32)
    denom = rng.integers(0, 50, (N, 1)).astype(np.float32)
    maxr = rng.integers(0, 600, N).astype(np.float32)
    want = ro.stats_f32(radii, grad, accum, denom, maxr)
    r = torch.from_numpy(radii).to(cuda_device)
    outs = {}
    for binding in ("ext", "ctypes", "api", "no_max"):
        (g, gb), (a, ab), (d, db), (mx, mb) = (carve(x, cuda_device) for x in (grad, accum, denom, maxr))
        if binding == "api":
            densification_stats(r, g, a, d, mx)
        elif binding == "no_max":
            densification_stats(r, g, a, d)  # max_radii2D=None is accepted
        else:
            _C.densification_stats(r, g, a, d, mx, binding=binding)
        assert all(guards_intact(b, x.size) for b, x in ((gb, grad), (ab, accum), (db, denom), (mb, maxr)))
        outs[binding] = got = (a.cpu().numpy(), d.cpu().numpy(), mx.cpu().numpy())
        np.testing.assert_array_equal(ro.bits(got[0]), ro.bits(want[0]), err_msg=f"grad_accum {binding}")
        np.testing.assert_array_equal(ro.bits(got[1]), ro.bits(want[1]), err_msg=f"denom {binding}")
        np.testing.assert_array_equal(ro.bits(got[2]), ro.bits(maxr if binding == "no_max" else want[2]),
                                      err_msg=f"max_radii2D {binding}")
        inv = radii <= 0
        for x, x0 in zip(got, (accum, denom, maxr)):
            np.testing.assert_array_equal(ro.bits(x).reshape(N)[inv], ro.bits(x0).reshape(N)[inv])
    assert not np.isnan(outs["ext"][0]).any()


# ---- optimizer state: checkpoints, prune, densify ------------------------------------------------------------------------
def test_state_dict_round_trip(cuda_device):
    """state_dict() -> fresh optimizer -> load_state_dict(): the next step is bit-identical."""
    N = 500
    rng = np.random.default_rng(23)
    groups = model_arrays(rng, N)
    opt, params = make_optimizer(cuda_device, groups)
    vis1 = torch.from_numpy(rng.random(N) < 0.6).to(cuda_device)
    opt.step(vis1, N)
    sd = copy.deepcopy(opt.state_dict())  # (as a checkpoint holds it: load_state_dict itself does not copy the tensors)
    snap = [(p.detach().cpu().numpy().reshape(N, -1), None) for p in params]
    opt2, params2 = make_optimizer(cuda_device, [(s[0],) + tuple(a[1:]) for s, a in zip(snap, groups)])
    opt2.load_state_dict(sd)
    grads = [make_group(rng, N, M)[1] for M in MODEL_M]
    vis2 = forms(rng, rng.random(N) < 0.4, cuda_device)["radii"]
    for o, ps in ((opt, params), (opt2, params2)):
        for prm, g in zip(ps, grads):
            prm.grad = torch.from_numpy(g).to(cuda_device).view(prm.shape)
        o.step(vis2, N)
    for a, b in zip(params, params2):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[a][key].view(torch.int32), opt2.state[b][key].view(torch.int32))
            assert opt.state[a][key].abs().sum().item() > 0


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


TRAIN_ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, feature_lr=2.5e-3, opacity_lr=2.5e-2,
                                   scaling_lr=5e-3, rotation_lr=1e-3)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
NAME_LR = dict(zip(NAMES, (1.6e-4, 2.5e-3, 2.5e-3 / 20.0, 2.5e-2, 5e-3, 1e-3)))


def model_from(raw, dev):
    from scene.gaussian_model import GaussianModel

    pc = GaussianModel(3, "sparse_adam")
    P = torch.nn.Parameter
    pc._xyz, pc._features_dc, pc._features_rest = P(raw.xyz.to(dev)), P(raw.features_dc.to(dev).contiguous()), \
        P(raw.features_rest.to(dev).contiguous())
    pc._opacity, pc._scaling, pc._rotation = P(raw.opacity.to(dev)), P(raw.scaling.to(dev)), P(raw.rotation.to(dev))
    pc.active_sh_degree = 3
    pc.spatial_lr_scale = 1.0
    pc.training_setup(TRAIN_ARGS)
    return pc


def host(t, N):
    return t.detach().cpu().numpy().reshape(N, -1)


def test_model_prune_and_densify_keep_the_moments(cuda_device, gs_paths):
    """GaussianModel(3, "sparse_adam"): step, prune_points, densification_postfix, step -- surviving rows keep their moments,
    new rows start at zero, and the second step matches the restatement."""
    from gsworld_amd import scenes
    from gsworld_amd.optim import SparseGaussianAdam

    dev = cuda_device
    N = 600
    rng = np.random.default_rng(29)
    pc = model_from(scenes.random_scene_camera_frame(N, seed=2), dev)
    assert isinstance(pc.optimizer, SparseGaussianAdam)
    assert [g["name"] for g in pc.optimizer.param_groups] == list(NAMES)
    cur = pc._current()
    ref = {n: (host(cur[n], N), np.zeros((N, cur[n][0].numel()), np.float32), np.zeros((N, cur[n][0].numel()), np.float32))
           for n in NAMES}

    def step(N, vis):
        cur = pc._current()
        for n in NAMES:
            g = make_group(rng, N, cur[n][0].numel())[1]
            cur[n].grad = torch.from_numpy(g).to(dev).view(cur[n].shape)
            ref[n] = ro.adam_f32(ref[n][0], g, ref[n][1], ref[n][2], vis, NAME_LR[n], EPS)
        pc.optimizer.step(torch.from_numpy(vis).to(dev), N)
        for n, group in zip(NAMES, pc.optimizer.param_groups):
            prm = group["params"][0]
            assert prm is pc._current()[n]
            st = pc.optimizer.state[prm]
            assert_bits((host(prm, N), host(st["exp_avg"], N), host(st["exp_avg_sq"], N)), ref[n], n)

    step(N, rng.random(N) < 0.7)
    prune = rng.random(N) < 0.2
    pc.prune_points(torch.from_numpy(prune).to(dev))
    extra = 50
    new = scenes.random_scene_camera_frame(extra, seed=3)
    pc.densification_postfix(new.xyz.to(dev), new.features_dc.to(dev), new.features_rest.to(dev), new.opacity.to(dev),
                             new.scaling.to(dev), new.rotation.to(dev), None)
    N2 = int((~prune).sum()) + extra
    new_np = dict(zip(NAMES, (new.xyz, new.features_dc, new.features_rest, new.opacity, new.scaling, new.rotation)))
    for n in NAMES:
        add = new_np[n].numpy().reshape(extra, -1)
        ref[n] = (np.concatenate((ref[n][0][~prune], add)), np.concatenate((ref[n][1][~prune], np.zeros_like(add))),
                  np.concatenate((ref[n][2][~prune], np.zeros_like(add))))
    assert pc.get_xyz.shape[0] == N2
    step(N2, rng.random(N2) < 0.5)


# ---- a training loop -------------------------------------------------------------------------------------------------------
def test_training_iterations_end_to_end(cuda_device, gs_paths):
    """3 000 Gaussians, 64 x 64, five iterations: render (gs_compat) -> photometric_loss -> backward ->
    add_densification_stats(..., radii) -> optimizer.step(radii, N).  After every iteration the six parameters, both moments,
    xyz_gradient_accum, denom and max_radii2D equal the restatement applied on the host to that iteration's own gradients and
    radii, bit for bit.  The loop runs under torch.cuda.set_sync_debug_mode("error"): nothing in it reads the device."""
    from gaussian_renderer import render

    from gsworld_amd import scenes
    from gsworld_amd.ssim import photometric_loss

    dev = cuda_device
    N, S, ITERS = 3000, 64, 5
    pc = model_from(scenes.random_scene_camera_frame(N, seed=4), dev)
    cam = scenes.identity_camera(S, S, 60.0).to(dev)
    pipe = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, antialiasing=False)
    bg = torch.zeros(3, device=dev)
    gt = torch.rand(3, S, S, generator=torch.Generator().manual_seed(8)).to(dev)
    start = {n: host(t, N) for n, t in pc._current().items()}
    log = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in range(ITERS):
            out = render(cam, pc, pipe, bg)
            loss = photometric_loss(out["render"], gt, 0.2)
            loss.backward()
            radii = out["radii"]
            pc.add_densification_stats(out["viewspace_points"], radii)
            pc.optimizer.step(radii, N)
            cur = pc._current()
            log.append({
                "radii": radii.clone(), "vgrad": out["viewspace_points"].grad.clone(),
                "grads": {n: cur[n].grad.clone() for n in NAMES}, "params": {n: cur[n].detach().clone() for n in NAMES},
                "m": {n: pc.optimizer.state[cur[n]]["exp_avg"].clone() for n in NAMES},
                "v": {n: pc.optimizer.state[cur[n]]["exp_avg_sq"].clone() for n in NAMES},
                "accum": pc.xyz_gradient_accum.clone(), "denom": pc.denom.clone(), "maxr": pc.max_radii2D.clone()})
            pc.optimizer.zero_grad(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = {n: (start[n], np.zeros_like(start[n]), np.zeros_like(start[n])) for n in NAMES}
    accum, denom, maxr = np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32), np.zeros(N, np.float32)
    seen = np.zeros(N, bool)
    for it, rec in enumerate(log):
        radii = rec["radii"].cpu().numpy()
        assert 0 < (radii > 0).sum() < N, "the view must see some Gaussians and miss some"
        seen |= radii > 0
        accum, denom, maxr = ro.stats_f32(radii, rec["vgrad"].cpu().numpy(), accum, denom, maxr)
        for name, got, want in (("xyz_gradient_accum", rec["accum"], accum), ("denom", rec["denom"], denom),
                                ("max_radii2D", rec["maxr"], maxr)):
            np.testing.assert_array_equal(ro.bits(got.cpu().numpy()), ro.bits(want), err_msg=f"iteration {it} {name}")
        for n in NAMES:
            g = host(rec["grads"][n], N)
            assert np.isfinite(g).all()
            ref[n] = ro.adam_f32(ref[n][0], g, ref[n][1], ref[n][2], radii, NAME_LR[n], EPS)
            assert_bits((host(rec["params"][n], N), host(rec["m"][n], N), host(rec["v"][n], N)), ref[n], f"iteration {it} {n}")
    # the loop trained: parameters of seen Gaussians moved, the others kept their bits
    assert (ro.bits(ref["xyz"][0])[seen] != ro.bits(start["xyz"])[seen]).any()
    np.testing.assert_array_equal(ro.bits(ref["xyz"][0])[~seen], ro.bits(start["xyz"])[~seen])
    assert float(denom.max()) == ITERS  # (a Gaussian in front of the camera is counted in every iteration)
