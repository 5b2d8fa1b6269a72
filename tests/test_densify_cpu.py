"""Densify-and-prune (include/gsr.h ``gsr_densify_plan`` / ``gsr_densify_apply``) on the CPU: exported symbols, argument
checks (they return before any device work), the workspace size, and ``GaussianModel``'s literal torch sequence -- upstream's
densify_and_clone / densify_and_split / prune_points on the model's hooks -- against the NumPy restatement
(tests/ref_densify.py): counts, order, copied bits, zero moments on new rows, side arrays reset."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from gsworld_amd import _lib
from tests import ref_densify as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = rd.NAMES
SHAPES = dict(zip(NAMES, ((3,), (1, 3), (15, 3), (1,), (3,), (4,))))
MS = dict(zip(NAMES, rd.MODEL_M))
TRAIN_ARGS = types.SimpleNamespace(percent_dense=rd.THRESHOLDS["percent_dense"], position_lr_init=1.6e-4, feature_lr=2.5e-3,
                                   opacity_lr=2.5e-2, scaling_lr=5e-3, rotation_lr=1e-3)


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


# ---- the library's argument checks -----------------------------------------------------------------------------------------
def test_symbols_exported_and_declared():
    names = {"gsr_densify_plan", "gsr_densify_apply", "gsr_densify_workspace_bytes"}
    assert names <= set(_lib.exported_symbols())
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names)
    assert lib.gsr_densify_plan.argtypes[0]._type_ is _lib.GsrDensifyPlan
    assert lib.gsr_densify_apply.argtypes[0]._type_ is _lib.GsrDensifyApply
    assert (_lib.DENSIFY_COPY, _lib.DENSIFY_XYZ, _lib.DENSIFY_SCALING) == (0, 1, 2)
    from gsworld_amd import _C, optim

    assert callable(_C.densify_plan) and callable(_C.densify_apply) and callable(optim.densify_and_prune)


def test_workspace_bytes_monotone_and_aligned():
    f = _lib.lib().gsr_densify_workspace_bytes
    sizes = [f(n) for n in (0, 1, 2, 255, 256, 257, 1025, 65536, 65793, 1 << 20, 1 << 30)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert sizes[-1] >= (1 << 30) * 8  # (two row-map entries per Gaussian: every Gaussian may come out twice)


def _plan(N=4, ptr=0x1000, ws=0x10000):
    """A GsrDensifyPlan whose pointers are never dereferenced: the checks under test return first."""
    s = _lib.GsrDensifyPlan()
    s.struct_size, s.N = C.sizeof(_lib.GsrDensifyPlan), N
    s.grad_accum = s.denom = s.scaling = s.opacity = s.counts = ptr
    s.workspace, s.workspace_bytes = ws, 1 << 40
    return s


def _apply(N=4, N_out=4, num_groups=1, M=3, role=0, moments=True):
    s = _lib.GsrDensifyApply()
    s.struct_size, s.N, s.N_out, s.num_groups = C.sizeof(_lib.GsrDensifyApply), N, N_out, num_groups
    s.workspace, s.workspace_bytes = 0x10000, 1 << 40  # (far from every other range below)
    s.xyz, s.scaling, s.rotation, s.noise, s.parent = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    for k in range(min(max(num_groups, 0), _lib.ADAM_MAX_GROUPS)):
        base = 0x1000000 * (k + 1)
        ptrs = [base + 0x100000 * j for j in range(6)]
        if not moments:
            ptrs[1] = ptrs[2] = ptrs[4] = ptrs[5] = None
        s.groups[k] = _lib.GsrDensifyGroup(*ptrs, M, role)
    return s


def _rc_plan(s):
    return _lib.lib().gsr_densify_plan(C.byref(s), None)


def _rc_apply(s):
    return _lib.lib().gsr_densify_apply(C.byref(s), None)


def _last():
    return _lib.lib().gsr_last_error()


def test_plan_rejects_invalid_arguments():
    E = _lib.GSR_E_INVALID
    s = _plan()
    s.struct_size -= 4
    assert _rc_plan(s) == E and b"gsr_densify_plan" in _last()
    assert _rc_plan(_plan(N=-1)) == E
    assert _rc_plan(_plan(N=(1 << 30) + 1)) == E and b"gsr_densify_plan" in _last()
    for field in ("grad_accum", "denom", "scaling", "opacity", "counts", "workspace"):
        s = _plan()
        setattr(s, field, None)
        assert _rc_plan(s) == E, field
    s = _plan(N=1000)
    s.workspace_bytes = _lib.lib().gsr_densify_workspace_bytes(1000) - 1
    assert _rc_plan(s) == E and b"gsr_densify_plan" in _last()
    assert _rc_plan(_plan(ws=0x10004)) == E
    assert _lib.lib().gsr_densify_plan(None, None) == E


def test_apply_rejects_invalid_arguments():
    E = _lib.GSR_E_INVALID
    s = _apply()
    s.struct_size += 8
    assert _rc_apply(s) == E and b"gsr_densify_apply" in _last()
    assert _rc_apply(_apply(N=-1)) == E
    assert _rc_apply(_apply(N=(1 << 30) + 1)) == E
    assert _rc_apply(_apply(N=4, N_out=9)) == E and b"gsr_densify_apply" in _last()
    assert _rc_apply(_apply(N_out=-1)) == E
    assert _rc_apply(_apply(num_groups=9)) == E
    assert _rc_apply(_apply(M=0)) == E
    assert _rc_apply(_apply(M=4097)) == E and b"gsr_densify_apply" in _last()
    assert _rc_apply(_apply(role=3)) == E
    assert _rc_apply(_apply(M=4, role=_lib.DENSIFY_XYZ)) == E  # (the computed roles are three floats wide)
    for field in ("workspace", "xyz", "scaling", "rotation", "noise", "parent"):
        s = _apply()
        setattr(s, field, None)
        assert _rc_apply(s) == E, field
    for field in ("param", "out_param", "exp_avg", "out_exp_avg_sq"):  # a null tensor; moments given in part
        s = _apply()
        setattr(s.groups[0], field, None)
        assert _rc_apply(s) == E, field
    assert _lib.lib().gsr_densify_apply(None, None) == E


def test_apply_rejects_overlap():
    E = _lib.GSR_E_INVALID
    s = _apply()
    s.groups[0].out_param = s.groups[0].param  # in place
    assert _rc_apply(s) == E and b"gsr_densify_apply" in _last() and b"overlap" in _last()
    s = _apply()
    s.groups[0].out_exp_avg = s.groups[0].exp_avg + 4 * 3 * 4 - 4  # the last float of the source
    assert _rc_apply(s) == E
    s = _apply(num_groups=2)
    s.groups[1].out_exp_avg_sq = s.groups[0].out_param + 8  # two outputs
    assert _rc_apply(s) == E and b"overlap" in _last()
    s = _apply()
    s.parent = s.noise + 16
    assert _rc_apply(s) == E
    s = _apply()
    s.groups[0].out_param = s.workspace + 64
    assert _rc_apply(s) == E


def test_empty_model_returns_ok_without_device():
    s = _plan(N=0)
    s.grad_accum = s.denom = s.scaling = s.opacity = s.counts = s.workspace = None
    assert _rc_plan(s) == _lib.GSR_OK
    s = _apply(N=0, N_out=0, num_groups=6)
    s.workspace = s.xyz = s.scaling = s.rotation = s.noise = s.parent = None
    assert _rc_apply(s) == _lib.GSR_OK
    # everything pruned: nothing to write, nothing launched (the checks still run)
    assert _rc_apply(_apply(N=7, N_out=0, num_groups=6, moments=False)) == _lib.GSR_OK
    assert _rc_apply(_apply(N=7, N_out=0, M=0)) == _lib.GSR_E_INVALID


def test_fused_route_has_no_cpu_path():
    from gsworld_amd.optim import densify_and_prune

    params = {n: torch.nn.Parameter(torch.zeros((4,) + SHAPES[n])) for n in NAMES}
    with pytest.raises(RuntimeError, match="no CPU path"):
        densify_and_prune(params, None, torch.zeros(4, 1), torch.ones(4, 1), grad_threshold=2e-4, min_opacity=5e-3,
                          extent=2.0, percent_dense=0.01, prune_world_size=True)


# ---- the restatement itself ----------------------------------------------------------------------------------------------
def test_restatement_children_float32_against_binary64():
    """The float32 child values of the restatement sit inside the bounds the device is held to."""
    rng = np.random.default_rng(5)
    N = 4000
    inp = rd.make_inputs(rng, np.full(N, rd.SPLIT))
    groups = rd.make_model(rng, N, inp["scaling"], inp["opacity"])
    noise = rng.normal(0, 1, (N, 2, 3)).astype(np.float32)
    dl, wl = rd.limits()
    pl = rd.plan(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], 2e-4, 5e-3, dl, wl, True)
    assert pl["counts"] == (0, 0, N, 2 * N)
    out = rd.apply(pl, groups, noise)
    for rows, pos, pb, cs, sb in rd.child_bounds(pl, groups, noise):
        assert (np.abs(out["xyz"][0][rows] - pos) <= pb).all()
        assert (np.abs(out["scaling"][0][rows] - cs) <= sb).all()


# ---- GaussianModel: the literal sequence ---------------------------------------------------------------------------------
def build_model(cls, groups, inp, optimizer_type="default", dev="cpu", stepped=True):
    pc = cls(3, optimizer_type)
    P = torch.nn.Parameter
    t = {n: torch.from_numpy(groups[n][0]).to(dev).view((-1,) + SHAPES[n]).contiguous() for n in NAMES}
    pc._xyz, pc._features_dc, pc._features_rest = P(t["xyz"]), P(t["f_dc"]), P(t["f_rest"])
    pc._opacity, pc._scaling, pc._rotation = P(t["opacity"]), P(t["scaling"]), P(t["rotation"])
    pc.spatial_lr_scale = 1.0
    pc.training_setup(TRAIN_ARGS)
    if stepped:
        for n, prm in pc._current().items():
            pc.optimizer.state[prm] = {"step": torch.tensor(7.0),
                                       "exp_avg": torch.from_numpy(groups[n][1]).to(dev).view(prm.shape).clone(),
                                       "exp_avg_sq": torch.from_numpy(groups[n][2]).to(dev).view(prm.shape).clone()}
    pc.xyz_gradient_accum = torch.from_numpy(inp["accum"]).to(dev).clone()
    pc.denom = torch.from_numpy(inp["denom"]).to(dev).clone()
    pc.max_radii2D = torch.full((groups["xyz"][0].shape[0],), 500.0, device=dev)
    return pc


def host(t, n_out, name):
    return t.detach().cpu().numpy().reshape(n_out, MS[name])


def check_model(pc, pl, want, groups, noise, stepped=True):
    """The model after densify_and_prune against the restatement: everything copied is equal bit for bit, the computed
    children sit within their bounds of the binary64 evaluation."""
    K, Cn, S, n_out = pl["counts"]
    cur = pc._current()
    new_rows = np.zeros(n_out, bool)
    new_rows[K + Cn:] = True
    for n in NAMES:
        prm = cur[n]
        assert isinstance(prm, torch.nn.Parameter) and prm.requires_grad and prm.shape == (n_out,) + SHAPES[n]
        assert pc.optimizer.param_groups[NAMES.index(n)]["params"][0] is prm
        got = host(prm, n_out, n)
        computed = new_rows if n in ("xyz", "scaling") else np.zeros(n_out, bool)
        np.testing.assert_array_equal(rd.bits(got[~computed]), rd.bits(want[n][0][~computed]), err_msg=n)
        st = pc.optimizer.state.get(prm)
        if not stepped:
            assert st is None or "exp_avg" not in st
            continue
        assert float(st["step"]) == 7.0
        for key, w in (("exp_avg", want[n][1]), ("exp_avg_sq", want[n][2])):
            g = host(st[key], n_out, n)
            np.testing.assert_array_equal(rd.bits(g), rd.bits(w), err_msg=f"{n} {key}")
            assert (g[K:] == 0).all() and (K == 0 or (g[:K] != 0).all())
    # order and parent: f_dc's first column carries the input row
    np.testing.assert_array_equal(host(cur["f_dc"], n_out, "f_dc")[:, 0].astype(np.int32), pl["parent"])
    for rows, pos, pb, cs, sb in rd.child_bounds(pl, groups, noise):
        assert (np.abs(cur["xyz"].detach().cpu().numpy()[rows] - pos) <= pb).all()
        assert (np.abs(cur["scaling"].detach().cpu().numpy()[rows] - cs) <= sb).all()
    assert pc.xyz_gradient_accum.shape == (n_out, 1) and not pc.xyz_gradient_accum.any()
    assert pc.denom.shape == (n_out, 1) and not pc.denom.any()
    assert pc.max_radii2D.shape == (n_out,) and not pc.max_radii2D.any()
    assert pc.tmp_radii is None


def case(seed, N, actions=None):
    rng = np.random.default_rng(seed)
    action = rng.integers(0, 7, N) if actions is None else np.asarray(actions)
    inp = rd.make_inputs(rng, action)
    dl, wl = rd.limits()
    m = rd.margins(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], 2e-4, 5e-3, dl, wl)
    assert (m >= rd.MARGIN).all()  # no row is left out of any comparison below
    groups = rd.make_model(rng, N, inp["scaling"], inp["opacity"])
    noise = rng.normal(0, 1, (N, 2, 3)).astype(np.float32)
    return inp, groups, noise


@pytest.mark.parametrize("world_on", [True, False])
@pytest.mark.parametrize("stepped", [True, False])
def test_literal_sequence_equals_restatement(gs_paths, world_on, stepped):
    from scene.gaussian_model import GaussianModel

    N = 700
    inp, groups, noise = case(11, N)
    dl, wl = rd.limits()
    pl = rd.plan(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], 2e-4, 5e-3, dl, wl, world_on)
    K, Cn, S, n_out = pl["counts"]
    assert 0 < K < N and Cn > 0 and S > 0, "the case must keep, prune, clone and split"
    want = rd.apply(pl, groups, noise)
    pc = build_model(GaussianModel, groups, inp, stepped=stepped)
    assert not pc._fused_densify()
    radii = torch.arange(N, dtype=torch.int32)
    pc.densify_and_prune(2e-4, 5e-3, rd.THRESHOLDS["extent"], 20 if world_on else None, radii,
                         noise=torch.from_numpy(noise))
    assert pc.last_densify_route == "literal"
    check_model(pc, pl, want, groups, noise, stepped=stepped)


@pytest.mark.parametrize("actions", ["keep", "prune", "clone", "split", "first", "last"])
def test_literal_sequence_edge_patterns(gs_paths, actions):
    from scene.gaussian_model import GaussianModel

    N = 130
    a = np.full(N, {"keep": rd.KEEP, "prune": rd.PRUNE, "clone": rd.CLONE, "split": rd.SPLIT}.get(actions, rd.KEEP))
    if actions == "first":
        a[0] = rd.SPLIT
    if actions == "last":
        a[-1] = rd.CLONE
    inp, groups, noise = case(13, N, a)
    dl, wl = rd.limits()
    pl = rd.plan(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], 2e-4, 5e-3, dl, wl, True)
    expect = {"keep": (N, 0, 0, N), "prune": (0, 0, 0, 0), "clone": (N, N, 0, 2 * N), "split": (0, 0, N, 2 * N),
              "first": (N - 1, 0, 1, N + 1), "last": (N, 1, 0, N + 1)}[actions]
    assert pl["counts"] == expect
    want = rd.apply(pl, groups, noise)
    pc = build_model(GaussianModel, groups, inp)
    pc.densify_and_prune(2e-4, 5e-3, rd.THRESHOLDS["extent"], 20, None, noise=torch.from_numpy(noise))
    check_model(pc, pl, want, groups, noise)


def test_subclass_overriding_the_hooks_is_routed_through_them(gs_paths):
    from scene.gaussian_model import GaussianModel

    calls = []

    class Hooked(GaussianModel):
        def prune_points(self, mask):
            calls.append(("prune", int(mask.sum())))
            super().prune_points(mask)

        def densification_postfix(self, *args):
            calls.append(("postfix", args[0].shape[0]))
            super().densification_postfix(*args)

    class OnlyPrune(GaussianModel):
        def prune_points(self, mask):
            super().prune_points(mask)

    N = 300
    inp, groups, noise = case(17, N)
    dl, wl = rd.limits()
    pl = rd.plan(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], 2e-4, 5e-3, dl, wl, True)
    pc = build_model(Hooked, groups, inp)
    assert not pc._fused_densify() and not build_model(OnlyPrune, groups, inp)._fused_densify()
    # (the route does not depend on the device for such a class: the test of it on a HIP device is in test_densify_gpu.py)
    pc.densify_and_prune(2e-4, 5e-3, rd.THRESHOLDS["extent"], 20, torch.zeros(N, dtype=torch.int32),
                         noise=torch.from_numpy(noise))
    assert [c[0] for c in calls] == ["postfix", "postfix", "prune", "prune"]
    assert calls[0][1] + calls[1][1] > 0
    check_model(pc, pl, rd.apply(pl, groups, noise), groups, noise)


def test_reset_opacity_formula(gs_paths):
    from scene.gaussian_model import GaussianModel

    N = 200
    inp, groups, noise = case(19, N)
    pc = build_model(GaussianModel, groups, inp)
    before = {n: (t.detach().clone(), pc.optimizer.state[t]["exp_avg"].clone()) for n, t in pc._current().items()}
    old = pc._opacity
    pc.reset_opacity()
    assert pc._opacity is not old and isinstance(pc._opacity, torch.nn.Parameter) and pc._opacity.requires_grad
    assert pc.optimizer.param_groups[3]["params"][0] is pc._opacity and old not in pc.optimizer.state
    o = groups["opacity"][0].astype(np.float64)
    x = np.minimum(1.0 / (1.0 + np.exp(-o)), 0.01)
    want = np.log(x / (1.0 - x))
    got = pc._opacity.detach().numpy().astype(np.float64)
    assert got.shape == (N, 1) and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert (got <= np.log(0.01 / 0.99) + 1e-5).all() and (got < -4.5).any() and (np.abs(got - o) < 1e-5).any()
    st = pc.optimizer.state[pc._opacity]
    assert float(st["step"]) == 7.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    for n, t in pc._current().items():
        if n != "opacity":
            assert torch.equal(t.detach(), before[n][0]) and torch.equal(pc.optimizer.state[t]["exp_avg"], before[n][1])
