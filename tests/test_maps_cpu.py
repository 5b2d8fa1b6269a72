"""Segmentation / depth maps (include/gsr.h gsr_render_maps) without a GPU: the C ABI's handshake, the loop's label check,
and the NumPy restatement of the maps that the GPU tests (tests/test_maps_gpu.py) hold the kernel to.

The restatement is the definition, walked pixel by pixel in float32: a pixel composites the depth-ordered list of its
16 x 16 tile as the colour compositor does (alpha = min(0.99, opacity exp(power)), skipped when power > 0 or alpha < 1/255,
T <- T (1 - alpha)); its median contributor is the first composited Gaussian after which T (1 - alpha) < 0.5; label and
depth (depth_scale / rec[0].w) are that Gaussian's, -1 / 0.0 where T never drops below 0.5."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as hp

F32 = np.float32
K255 = 1.0 / (1.0 - 1.0 / 255.0) + 1e-6  # (the most a flipped alpha of 1/255 changes every later T by)


def _fma(a, b, c):
    # (a b is exact in binary64 for binary32 operands; the sum is rounded twice -- at most an ulp of power off, which only
    #  matters at the thresholds the borderline test covers)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def restate_maps(splat, point_list, ranges, W, H, labels=None, depth_scale=1.0, super_tiles=False, chunk=256):
    """-> (label (H,W) int16, depth (H,W) float32, borderline (H,W) bool).  ``splat`` (P,12) float32 records as the state
    holds them, ``point_list`` / ``ranges``: the frame's lists -- per tile, or (``super_tiles``) per 2 x 1 super-tile with
    the tile rect as four bytes in the record's last word.  A pixel is borderline when some contributor up to its median
    (every contributor, if it has none) has |T (1 - alpha) / 0.5 - 1| <= 1e-4, or has an alpha within hp.BORDER_EPS of 1/255
    while the pixel's T next to its median (its last T, if it has none) lies within a factor 1 - 1/255 of 0.5 -- the most
    such a contributor changes when it flips: there an exp() that differs by an ulp may move the decision."""
    splat = np.ascontiguousarray(splat, dtype=F32)
    point_list = np.asarray(point_list).astype(np.int64)
    ranges = np.asarray(ranges).astype(np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    label = np.full((H, W), -1, np.int16)
    depth = np.zeros((H, W), F32)
    border = np.zeros((H, W), bool)
    rb = splat[:, 11].view(np.uint32)
    thr = F32(1.0) / F32(255.0)
    for ty in range(gy):
        for tx in range(gx):
            r0, r1 = ranges[ty * ((gx + 1) // 2) + tx // 2] if super_tiles else ranges[ty * gx + tx]
            idx = point_list[r0:r1]
            if super_tiles and idx.size:
                b = rb[idx]
                inside = (tx >= (b & 255)) & (tx < ((b >> 16) & 255)) & (ty >= ((b >> 8) & 255)) & (ty < (b >> 24))
                idx = idx[inside]
            xs = np.arange(tx * 16, min(tx * 16 + 16, W))
            ys = np.arange(ty * 16, min(ty * 16 + 16, H))
            pyy, pxx = np.meshgrid(ys, xs, indexing="ij")
            pfx, pfy = pxx.reshape(-1).astype(F32), pyy.reshape(-1).astype(F32)
            n = pfx.size
            T = np.ones(n, F32)
            done = np.zeros(n, bool)
            near_px = np.zeros(n, bool)
            near_a_px, tight_px = np.zeros(n, bool), np.zeros(n, bool)
            lab_t = np.full(n, -1, np.int16)
            dep_t = np.zeros(n, F32)
            for c0 in range(0, idx.size, chunk):
                g = idx[c0:c0 + chunk]
                rec = splat[g]
                dx = rec[None, :, 0] - pfx[:, None]
                dy = rec[None, :, 1] - pfy[:, None]
                cA, cC, cB = F32(-0.5) * rec[:, 4], F32(-0.5) * rec[:, 6], -rec[:, 5]
                q = _fma(cC[None, :] * dy, dy, (cA[None, :] * dx) * dx)
                power = _fma(cB[None, :] * dx, dy, q)
                ex = np.exp(np.minimum(power, 0).astype(np.float64)).astype(F32)
                alpha = np.minimum(F32(0.99), rec[None, :, 7] * ex)
                valid = (power <= 0) & (alpha >= thr)
                fac = F32(1.0) - np.where(valid, alpha, F32(0.0))
                seq = np.cumprod(np.concatenate([T[:, None], fac], 1), axis=1, dtype=F32)[:, 1:]
                cross = valid & (seq < F32(0.5))
                first = cross.any(1) & ~done
                j = np.argmax(cross, 1)
                upto = np.arange(g.size)[None, :] <= np.where(first, j, g.size)[:, None]
                near_T = valid & (np.abs(seq.astype(np.float64) / 0.5 - 1.0) <= 1e-4)
                near_a = (power <= 0) & (np.abs(alpha.astype(np.float64) * 255.0 - 1.0) <= hp.BORDER_EPS)
                # an alpha at 1/255 that flips scales every later T by (1 - 1/255) at most: it can move the decision only
                # where the T around the median (or the last T of a pixel without one) lies within that factor of 0.5
                t_at = seq[np.arange(n), j].astype(np.float64)
                t_before = np.where(j > 0, seq[np.arange(n), np.maximum(j - 1, 0)], T).astype(np.float64)
                tight_px |= first & ((t_before < 0.5 * K255) | (t_at * K255 > 0.5))
                near_px |= (near_T & upto).any(1) & ~done
                near_a_px |= (near_a & upto).any(1) & ~done
                gm = g[j]
                if labels is not None:
                    lab_t = np.where(first, np.asarray(labels)[gm].astype(np.int32).astype(np.int16), lab_t)
                dep_t = np.where(first, F32(depth_scale) / splat[gm, 3], dep_t)
                T = np.where(done | first, T, seq[:, -1])
                done |= first
                if done.all():
                    break
            label[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = lab_t.reshape(ys.size, xs.size)
            depth[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = dep_t.reshape(ys.size, xs.size)
            tight_px |= ~done & (T.astype(np.float64) < 0.5 * K255)
            near_px |= near_a_px & tight_px
            border[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = near_px.reshape(ys.size, xs.size)
    return label, depth, border


def _one_tile(recs):
    """A 16 x 16 image, one tile whose list is ``recs`` in depth order: (x, y, invdepth, A, B, C, opacity) each."""
    splat = np.zeros((len(recs), 12), F32)
    for i, (x, y, inv, A, B, Cc, op) in enumerate(recs):
        splat[i, [0, 1, 2, 3, 4, 5, 6, 7]] = [x, y, 1.0 / inv, inv, A, B, Cc, op]
    return splat, np.arange(len(recs)), np.array([[0, len(recs)]])


def test_restatement_opaque_front_splat():
    # a wide opaque splat in front of another: every pixel's median is the front one (alpha 0.99 at its centre)
    splat, pl, rg = _one_tile([(8.0, 8.0, 0.5, 1e-6, 0.0, 1e-6, 0.99), (8.0, 8.0, 0.25, 1e-6, 0.0, 1e-6, 0.99)])
    lab, dep, bd = restate_maps(splat, pl, rg, 16, 16, labels=np.array([5.0, 9.0], F32), depth_scale=2.0)
    assert (lab == 5).all() and np.allclose(dep, 4.0) and not bd.any()


def test_restatement_two_splats_cross_at_the_second():
    # 0.3 then 0.3: T = 0.7, then 0.49 < 0.5 -- the second one is the median
    splat, pl, rg = _one_tile([(8.0, 8.0, 1.0, 1e-9, 0.0, 1e-9, 0.3), (8.0, 8.0, 0.5, 1e-9, 0.0, 1e-9, 0.3)])
    lab, dep, _ = restate_maps(splat, pl, rg, 16, 16, labels=np.array([1.0, 2.0], F32))
    assert (lab == 2).all() and np.allclose(dep, 2.0)


def test_restatement_pixel_that_never_crosses_is_background():
    splat, pl, rg = _one_tile([(8.0, 8.0, 1.0, 1e-9, 0.0, 1e-9, 0.3)])
    lab, dep, _ = restate_maps(splat, pl, rg, 16, 16, labels=np.array([1.0], F32))
    assert (lab == -1).all() and (dep == 0.0).all()


def test_restatement_skips_alpha_below_1_over_255():
    # 0.3 and 0.2855 leave T = 0.50015; a third splat of alpha 0.003 < 1/255 would take T below 0.5 if it were composited
    splat, pl, rg = _one_tile([(8.0, 8.0, 1.0, 1e-9, 0.0, 1e-9, 0.3), (8.0, 8.0, 0.5, 1e-9, 0.0, 1e-9, 0.2855),
                               (8.0, 8.0, 0.4, 1e-9, 0.0, 1e-9, 0.003)])
    lab, dep, _ = restate_maps(splat, pl, rg, 16, 16, labels=np.array([1.0, 2.0, 3.0], F32))
    assert (lab == -1).all() and (dep == 0.0).all()
    # ... whereas an alpha of 0.005 is composited and is the median
    splat[2, 7] = 0.005
    lab, _, _ = restate_maps(splat, pl, rg, 16, 16, labels=np.array([1.0, 2.0, 3.0], F32))
    assert (lab == 3).all()


def test_restatement_super_tile_lists_take_the_tile_s_members_only():
    # one 32 x 16 super-tile list; the first record's rect covers tile 1 only, so tile 0 sees the second one alone
    splat, pl, rg = _one_tile([(8.0, 8.0, 0.5, 1e-9, 0.0, 1e-9, 0.9), (8.0, 8.0, 0.25, 1e-9, 0.0, 1e-9, 0.9)])
    rect = lambda x0, y0, x1, y1: np.array([x0 | (y0 << 8) | (x1 << 16) | (y1 << 24)], np.uint32).view(F32)[0]  # noqa: E731
    splat[0, 11], splat[1, 11] = rect(1, 0, 2, 1), rect(0, 0, 2, 1)
    lab, _, _ = restate_maps(splat, pl, rg, 32, 16, labels=np.array([1.0, 2.0], F32), super_tiles=True)
    assert (lab[:, :16] == 2).all() and (lab[:, 16:] == 1).all()


def test_render_maps_is_exported_and_checks_its_struct_size():
    from gsworld_amd import _lib

    L = _lib.lib()
    assert hasattr(L, "gsr_render_maps") and "gsr_render_maps" in _lib.exported_symbols()
    f = _lib.GsrMapFrame()
    f.struct_size = C.sizeof(_lib.GsrMapFrame) + 8
    assert L.gsr_render_maps(1, C.byref(f), None) == _lib.GSR_E_INVALID
    assert b"struct_size" in L.gsr_last_error()
    # the ctypes mirror has the library's size: the next check (no settings) is what refuses the frame now
    f.struct_size = C.sizeof(_lib.GsrMapFrame)
    assert L.gsr_render_maps(1, C.byref(f), None) == _lib.GSR_E_INVALID
    assert b"null settings" in L.gsr_last_error()
    assert L.gsr_render_maps(0, None, None) == _lib.GSR_OK


def test_loop_label_check_rejects_non_integral_or_out_of_range_labels():
    from gsworld_amd.closed_loop import ClosedLoopRenderer, check_map_labels

    ok = check_map_labels(torch.tensor([[0.0], [-1.0], [17.0], [32767.0], [-32768.0]]))
    assert ok.dtype == torch.float32 and ok.shape == (5,)
    for bad in ([0.0, 1.5], [40000.0], [-32769.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            check_map_labels(torch.tensor(bad))
    with pytest.raises(ValueError):
        ClosedLoopRenderer(None, {}, {}, maps=("segmentation", "normals"))


def test_pipelined_loop_refuses_maps():
    from gsworld_amd.closed_loop import PipelinedClosedLoop

    with pytest.raises(ValueError, match="ClosedLoopRenderer"):
        PipelinedClosedLoop(None, {}, {}, maps=("depth",))
