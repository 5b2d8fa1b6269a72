"""The optimizer step and the densification statistics (include/gsr.h ``gsr_adam_update`` / ``gsr_densification_stats``)
on the CPU: exported symbols, argument checks (they return before any device work), the float32 restatement
(tests/ref_optim.py) against a binary64 evaluation, and the "no CPU path" error of the Python layer."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsworld_amd import _lib
from tests import ref_optim as ro


def test_symbols_exported():
    assert {"gsr_adam_update", "gsr_densification_stats"} <= set(_lib.exported_symbols())
    lib = _lib.lib()
    assert hasattr(lib, "gsr_adam_update") and hasattr(lib, "gsr_densification_stats")
    assert _lib.ADAM_MAX_GROUPS == 8 and (_lib.VISIBLE_ALL, _lib.VISIBLE_MASK8, _lib.VISIBLE_RADII) == (0, 1, 2)


def _step(N=4, num_groups=1, M=3, kind=_lib.VISIBLE_ALL, visible=None, ptr=0x1000):
    """A GsrAdamStep whose pointers are never dereferenced: the checks under test return first."""
    s = _lib.GsrAdamStep()
    s.struct_size, s.N, s.num_groups, s.visible_kind, s.visible = C.sizeof(_lib.GsrAdamStep), N, num_groups, kind, visible
    for k in range(min(max(num_groups, 0), _lib.ADAM_MAX_GROUPS)):
        s.groups[k] = _lib.GsrAdamGroup(ptr, ptr, ptr, ptr, M, 1e-3, 0.9, 0.999, 1e-15)
    return s


def _rc(s):
    return _lib.lib().gsr_adam_update(C.byref(s), None)


def test_invalid_arguments_are_rejected():
    s = _step()
    s.struct_size -= 4
    assert _rc(s) == _lib.GSR_E_INVALID
    assert _rc(_step(num_groups=0)) == _lib.GSR_E_INVALID
    assert _rc(_step(num_groups=9)) == _lib.GSR_E_INVALID
    assert _rc(_step(M=0)) == _lib.GSR_E_INVALID
    assert _rc(_step(M=4097)) == _lib.GSR_E_INVALID
    assert _rc(_step(N=-1)) == _lib.GSR_E_INVALID
    s = _step()
    s.groups[0].param = None
    assert _rc(s) == _lib.GSR_E_INVALID
    assert _rc(_step(kind=3)) == _lib.GSR_E_INVALID
    assert _rc(_step(kind=_lib.VISIBLE_MASK8, visible=None)) == _lib.GSR_E_INVALID  # kind / NULL mismatch, both ways
    assert _rc(_step(kind=_lib.VISIBLE_ALL, visible=0x1000)) == _lib.GSR_E_INVALID
    assert b"gsr_adam_update" in _lib.lib().gsr_last_error()


def test_empty_model_returns_ok_without_device():
    assert _rc(_step(N=0)) == _lib.GSR_OK
    s = _step(N=0, num_groups=6)
    for k in range(6):
        s.groups[k].param = None  # (nothing is read at N == 0)
    assert _rc(s) == _lib.GSR_OK
    assert _lib.lib().gsr_densification_stats(0, None, None, None, None, None, None) == _lib.GSR_OK
    assert _lib.lib().gsr_densification_stats(-1, None, None, None, None, None, None) == _lib.GSR_E_INVALID


def test_restatement_against_binary64():
    """100 k seeded elements: |g| log-uniform over 1e-8 .. 1e2 with zeros, m = v = 0 on every fifth element.  The float32
    restatement stays within 1e-6 relative of the binary64 evaluation in p, 2e-7 in v, everything finite."""
    rng = np.random.default_rng(20)
    n = 100_000
    g = (10.0 ** rng.uniform(-8, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0.0
    m = (g * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    v = (g.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    m[::5] = 0.0
    v[::5] = 0.0
    # |p| in 0.1 .. 10: the step is at most lr / sqrt(1 - beta2) ~ 5e-3 with a handful of roundings (~4e-7 relative), so
    # its error is ~2e-9 absolute -- well inside 1e-6 of |p|, next to p's own half ulp (6e-8 relative)
    p = (rng.uniform(0.1, 10.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    lr, eps = 1.6e-4, 1e-15
    p32, m32, v32 = ro.adam_f32(p[:, None], g[:, None], m[:, None], v[:, None], None, lr, eps)
    p64, m64, v64 = ro.adam_f64(p[:, None], g[:, None], m[:, None], v[:, None], lr, eps)
    assert p32.dtype == np.float32 and np.isfinite(p32).all() and np.isfinite(m32).all() and np.isfinite(v32).all()
    assert np.isfinite(p64).all()
    assert (np.abs(p32 - p64) <= 1e-6 * np.abs(p64)).all()
    assert (np.abs(v32 - v64) <= 2e-7 * v64).all()  # (v' is 0 or >= 1e-19 here: never denormal)
    # invisible rows keep their bits, NaN gradients there are never read
    vis = rng.random(n) < 0.5
    g2 = g.copy()
    g2[~vis] = np.nan
    q, mq, vq = ro.adam_f32(p[:, None], g2[:, None], m[:, None], v[:, None], vis, lr, eps)
    np.testing.assert_array_equal(ro.bits(q)[~vis], ro.bits(p[:, None])[~vis])
    np.testing.assert_array_equal(ro.bits(mq)[~vis], ro.bits(m[:, None])[~vis])
    np.testing.assert_array_equal(ro.bits(q)[vis], ro.bits(p32)[vis])
    np.testing.assert_array_equal(ro.bits(vq)[vis], ro.bits(v32)[vis])


def test_sparse_adam_has_no_cpu_path():
    from gsworld_amd.optim import SparseGaussianAdam, densification_stats

    p = torch.nn.Parameter(torch.zeros(4, 3))
    opt = SparseGaussianAdam([{"params": [p], "lr": 1e-3, "name": "xyz"}], lr=0.0, eps=1e-15)
    p.grad = torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step(None, 4)
    assert torch.equal(p.detach(), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        densification_stats(torch.ones(4, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 1))
    # a group without a gradient is left out: nothing to do, nothing raised
    p.grad = None
    opt.step(None, 4)
