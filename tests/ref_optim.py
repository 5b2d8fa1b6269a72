"""Float32 NumPy restatements of the two definitions in include/gsr.h: ``gsr_adam_update`` and ``gsr_densification_stats``
(csrc/optim.hip).  Every operand is ``np.float32`` and the operations come in the written order, one rounding each: IEEE
binary32 add / mul / div / sqrt are correctly rounded on the host as in the kernels (contraction off, denormals kept), so
the GPU tests compare BITS, not tolerances.  :func:`adam_f64` evaluates the same formulas in binary64 (the CPU test bounds
the restatement's own rounding with it).  Nothing here is imported by the product package."""
from __future__ import annotations

import numpy as np

F = np.float32


def visible_rows(visible, N: int) -> np.ndarray:
    """bool (N,) of a ``visible`` argument: None (all), a bool / uint8 mask (!= 0) or int32 radii (> 0)."""
    if visible is None:
        return np.ones(N, bool)
    visible = np.asarray(visible).reshape(-1)
    assert visible.size == N
    return visible > 0 if visible.dtype == np.int32 else visible != 0


def adam_f32(p, g, m, v, visible, lr, eps, beta1=0.9, beta2=0.999):
    """-> (p', m', v') float32 (N, M) copies: the update on the rows ``visible`` marks, the input bits on the others."""
    p, g, m, v = (np.ascontiguousarray(a, F) for a in (p, g, m, v))
    N = p.shape[0]
    p2, m2, v2 = p.reshape(N, -1).copy(), m.reshape(N, -1).copy(), v.reshape(N, -1).copy()
    g2 = g.reshape(N, -1)
    r = visible_rows(visible, N)
    b1, b2, e = F(beta1), F(beta2), F(eps)
    omb1, omb2 = F(1) - b1, F(1) - b2  # formed once, in binary32
    nlr = -F(lr)
    with np.errstate(all="ignore"):
        gg, mm, vv, pp = g2[r], m2[r], v2[r], p2[r]
        m_new = (b1 * mm) + (omb1 * gg)
        v_new = (b2 * vv) + ((omb2 * gg) * gg)
        p_new = pp + ((nlr * m_new) / (np.sqrt(v_new) + e))
    assert m_new.dtype == F and v_new.dtype == F and p_new.dtype == F
    m2[r], v2[r], p2[r] = m_new, v_new, p_new
    return p2.reshape(p.shape), m2.reshape(p.shape), v2.reshape(p.shape)


def adam_f64(p, g, m, v, lr, eps, beta1=0.9, beta2=0.999):
    """The same formulas on every row in binary64, from the float32 inputs and the float32 constants."""
    p, g, m, v = (np.asarray(a, F).astype(np.float64) for a in (p, g, m, v))
    b1, b2, e, lr = (float(F(x)) for x in (beta1, beta2, eps, lr))
    m_new = b1 * m + (1.0 - b1) * g
    v_new = b2 * v + (1.0 - b2) * g * g
    with np.errstate(all="ignore"):
        p_new = p + (-lr * m_new) / (np.sqrt(v_new) + e)
    return p_new, m_new, v_new


def stats_f32(radii, grad2D, accum, denom, max_radii=None):
    """-> (accum', denom', max_radii' | None) float32 copies of the accumulators' shapes."""
    radii = np.asarray(radii, np.int32).reshape(-1)
    N = radii.size
    g = np.asarray(grad2D, F).reshape(N, 3)
    a, d = np.array(accum, F, copy=True), np.array(denom, F, copy=True)
    r = radii > 0
    with np.errstate(all="ignore"):
        gx, gy = g[r, 0], g[r, 1]
        norm = np.sqrt((gx * gx) + (gy * gy))
        a.reshape(-1)[r] = a.reshape(-1)[r] + norm
        d.reshape(-1)[r] = d.reshape(-1)[r] + F(1)
        mx = None
        if max_radii is not None:
            mx = np.array(max_radii, F, copy=True)
            mx.reshape(-1)[r] = np.fmax(mx.reshape(-1)[r], radii[r].astype(F))
    assert norm.dtype == F
    return a, d, mx


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F).view(np.uint32)
