"""Binary64 references of the observation kernels (csrc/maps.hip, csrc/pointcloud.hip), independent of every GPU list
format.  The float32 restatements (tests/test_maps_cpu.py restate_maps, tests/test_pointcloud_cpu.py restate_pointcloud)
mirror their kernels' arithmetic and read the GPU's own lists and maps; these start from the oracle's geometry and per-tile
lists (oracle/gs_oracle.c, bit-exact with the GPU on exact frames) and from the definitions, evaluated in binary64.

* :func:`maps_f64` -- segmentation / depth maps by a binary64 walk over the oracle's per-tile lists, with a borderline mask.
* :func:`cloud_f64` -- one environment's point cloud by a binary64 unprojection, with crop / exclusion / stride selection.
* :func:`fps_check` -- what farthest-point sampling must satisfy, checked in binary64.

Bands (a pixel or point inside one may legitimately differ between binary32 and binary64):
  * T: a composited contributor up to the median with |T (1 - alpha) / 0.5 - 1| <= T_BAND (1e-4, the restatement's band;
    the binary32 product drifts from the binary64 one by a few ulp per contributor);
  * alpha: |alpha 255 - 1| <= ALPHA_BAND + e, and power: |power| <= e, with ALPHA_BAND = hp.BORDER_EPS (the exp() ulp band)
    and e the error bound of the kernel's binary32 power (POWER_ULPS ulp of its largest term: fmas and the rounded dx, dy);
  * crop: a coordinate within CROP_TOL (1 + |q|) of a crop face, CROP_TOL the stated unprojection tolerance.
Nothing here is imported by the product package."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import helpers as hp

T_BAND = 1e-4
ALPHA_BAND = hp.BORDER_EPS
POWER_ULPS = 8.0
CROP_TOL = 4e-6
THREADS = min(16, os.cpu_count() or 1)

_EPS32 = 2.0 ** -24  # (a binary32 ulp, relative, half of 2^-23)


def _tile_maps(tile, gx, W, H, means2D, conic, depths, ranges, point_list, labels, depth_scale):
    tx, ty = tile % gx, tile // gx
    xs = np.arange(tx * 16, min(tx * 16 + 16, W))
    ys = np.arange(ty * 16, min(ty * 16 + 16, H))
    pyy, pxx = np.meshgrid(ys, xs, indexing="ij")
    pfx, pfy = pxx.reshape(-1).astype(np.float64), pyy.reshape(-1).astype(np.float64)
    n = pfx.size
    r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
    idx = point_list[r0:r1]
    T = np.ones(n)
    done = np.zeros(n, bool)
    border = np.zeros(n, bool)
    lab = np.full(n, -1, np.int16)
    dep = np.zeros(n)
    c0, chunk = 0, 32
    while c0 < idx.size and not done.all():
        g = idx[c0:c0 + chunk]
        c0 += chunk
        chunk = min(2 * chunk, 1024)  # (most pixels decide after a few contributors; background ones walk the whole list)
        dx = means2D[g, 0][None, :] - pfx[:, None]
        dy = means2D[g, 1][None, :] - pfy[:, None]
        A, B, Cc, op = conic[g, 0][None, :], conic[g, 1][None, :], conic[g, 2][None, :], conic[g, 3][None, :]
        ta, tc, tb = 0.5 * A * dx * dx, 0.5 * Cc * dy * dy, B * dx * dy
        power = -(ta + tc) - tb
        err = POWER_ULPS * _EPS32 * (np.abs(ta) + np.abs(tc) + np.abs(tb))
        alpha = np.minimum(0.99, op * np.exp(np.minimum(power, 0.0)))
        valid = (power <= 0.0) & (alpha >= 1.0 / 255.0)
        seq = T[:, None] * np.cumprod(np.where(valid, 1.0 - alpha, 1.0), axis=1)
        cross = valid & (seq < 0.5)
        first = cross.any(1) & ~done
        j = np.argmax(cross, 1)
        upto = np.arange(g.size)[None, :] <= np.where(first, j, g.size)[:, None]
        near = valid & (np.abs(seq / 0.5 - 1.0) <= T_BAND)
        near |= (power <= err) & (np.abs(alpha * 255.0 - 1.0) <= ALPHA_BAND + err)
        near |= (np.abs(power) < err) & (op >= 1.0 / 255.0)
        border |= (near & upto).any(1) & ~done
        gm = g[j]
        if labels is not None:
            lab = np.where(first, labels[gm].astype(np.int32).astype(np.int16), lab)
        dep = np.where(first, depth_scale * depths[gm], dep)
        T = np.where(done | first, T, seq[:, -1])
        done |= first
    return ys, xs, lab.reshape(ys.size, xs.size), dep.reshape(ys.size, xs.size), border.reshape(ys.size, xs.size)


def maps_f64(geom, binning, W, H, labels=None, depth_scale=1.0, threads=THREADS):
    """Segmentation / depth maps of a frame from the oracle (``hp.oracle_forward``'s ``geom`` and ``binning``), in binary64.

    Per pixel the tile's depth-ordered list is walked: power = -(A dx^2 + C dy^2) / 2 - B dx dy, alpha = min(0.99, opacity
    exp(power)), skipped when power > 0 or alpha < 1/255, T <- T (1 - alpha); the median contributor is the first after
    which T < 0.5.  -> (label (H,W) int16 = (int16)(int)labels[g] or -1, depth (H,W) float64 = depth_scale depth[g] or 0.0,
    borderline (H,W) bool: a decision up to the median (over the whole list without one) inside a band of the module
    docstring).  ``labels`` None: the label map is all -1."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    means2D = np.asarray(geom["means2D"], np.float32).astype(np.float64)
    conic = np.asarray(geom["conic_opacity"], np.float32).astype(np.float64)
    depths = np.asarray(geom["depths"], np.float32).astype(np.float64)
    ranges = np.asarray(binning["ranges"]).astype(np.int64).reshape(gx * gy, 2)
    point_list = np.asarray(binning["point_list"]).astype(np.int64)
    labels = None if labels is None else np.asarray(labels, np.float32)
    label = np.full((H, W), -1, np.int16)
    depth = np.zeros((H, W))
    border = np.zeros((H, W), bool)

    def run(tile):
        return _tile_maps(tile, gx, W, H, means2D, conic, depths, ranges, point_list, labels, float(depth_scale))

    with ThreadPoolExecutor(max(1, threads)) as ex:
        for ys, xs, lab, dep, bd in ex.map(run, range(gx * gy)):
            label[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = lab
            depth[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = dep
            border[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = bd
    return label, depth, border


def _w2c64(viewmatrix):
    m = np.asarray(viewmatrix, np.float32).astype(np.float64).reshape(4, 4)
    return m.T  # (the 16 floats are W2C^T: W2C[r][k] = m[4k + r])


def unproject_f64(D, viewmatrix, tanfovx, tanfovy, depth_scale=1.0, A=None):
    """(H,W) float32 depth map -> (q (H*W,3) float64, is-a-point (H*W,) bool), row-major by pixel: ndc = (2x+1)/W - 1,
    view point (ndc_x tanfovx z, ndc_y tanfovy z, z) with z = D / depth_scale, q = A inv(W2C) (view point, 1) -- every step
    in binary64 from the float32 inputs (``A``: the 3 x 4 out_from_scene in binary64, identity when None)."""
    D = np.asarray(D, np.float32).astype(np.float64)
    H, W = D.shape
    y, x = np.mgrid[0:H, 0:W]
    z = D / float(depth_scale)
    ndx = (2.0 * x + 1.0) / W - 1.0
    ndy = (2.0 * y + 1.0) / H - 1.0
    tx, ty = float(np.float32(tanfovx)), float(np.float32(tanfovy))
    v = np.stack([(ndx * tx * z).reshape(-1), (ndy * ty * z).reshape(-1), z.reshape(-1), np.ones(H * W)], 1)
    c2w = np.linalg.inv(_w2c64(viewmatrix))
    A64 = np.eye(3, 4) if A is None else np.asarray(A, np.float64).reshape(-1)[:12].reshape(3, 4)
    M = A64 @ c2w
    return v @ M.T, (D > 0).reshape(-1)


def stride_ranks(n: int, M: int) -> np.ndarray:
    """Slot j < M holds the valid point of rank floor(j n / M), in exact (Python) integers."""
    return np.array([(j * n) // M for j in range(M)], np.int64) if M > 0 else np.zeros(0, np.int64)


def cloud_f64(views, spec, depth_scale=1.0):
    """The cloud of ONE environment in binary64, after the definition of csrc/pointcloud.hip's header.  ``views``: per
    camera dicts with ``depth`` (H,W) float32, ``label`` (H,W) int16 or None, ``viewmatrix`` (16,), ``tanfovx`` / ``tanfovy``;
    ``spec``: a :class:`gsworld_amd.pointcloud.PointCloudSpec`.
    -> dict: ``q`` (N,3) float64 and ``valid`` / ``border`` (N,) bool over every pixel of every camera in dense order (a
    point is borderline when a coordinate lies within CROP_TOL (1 + |q|) of a crop face); ``label`` (N,) int16; ``n`` the
    valid count; ``sel`` the dense indices of the selected points (STRIDE: the slots; FPS: the candidates, M = min(n,
    fps_candidates); DENSE: every valid point)."""
    A = np.asarray(spec.affine(), np.float64)
    qs, oks, bds, labs = [], [], [], []
    for v in views:
        q, ok = unproject_f64(v["depth"], v["viewmatrix"], v["tanfovx"], v["tanfovy"], depth_scale, A)
        npx = q.shape[0]
        lab = np.asarray(v["label"], np.int16).reshape(-1) if v.get("label") is not None else np.full(npx, -1, np.int16)
        bd = np.zeros(npx, bool)
        if spec.crop is not None:
            lo, hi = (np.asarray(c, np.float32).astype(np.float64) for c in spec.crop)
            tol = CROP_TOL * (1.0 + np.abs(q))
            bd = ok & np.any((np.abs(q - lo) <= tol) | (np.abs(q - hi) <= tol), axis=1)
            ok = ok & np.all((q >= lo) & (q <= hi), axis=1)
        if len(spec.exclude_labels):
            ok = ok & ~np.isin(lab, np.asarray(spec.exclude_labels, np.int16))
        qs.append(q)
        oks.append(ok)
        bds.append(bd)
        labs.append(lab)
    q, ok, bd, lab = np.concatenate(qs), np.concatenate(oks), np.concatenate(bds), np.concatenate(labs)
    idx = np.flatnonzero(ok)
    n = int(idx.size)
    if spec.num_points is None:
        sel = idx
    else:
        M = min(n, int(spec.num_points) if spec.sample == "stride" else int(spec.fps_candidates))
        sel = idx[stride_ranks(n, M)]
    return dict(q=q, valid=ok, border=bd, label=lab, n=n, sel=sel)


def fps_check(candidates_f64, picks, rel=1e-5):
    """Asserts what farthest-point sampling from candidate 0 must satisfy, in binary64: pick 0 is candidate 0, every pick is
    a candidate, and each later pick's minimum squared distance to the earlier picks is at least (1 - rel) x the largest
    such distance over all candidates.  ``candidates_f64`` (M,3); ``picks`` candidate indices in pick order (-1: a pick
    that is no candidate).  -> the smallest ratio (pick's distance / largest distance) seen, 1.0 if there is none."""
    P = np.asarray(candidates_f64, np.float64)
    picks = np.asarray(picks, np.int64)
    M = P.shape[0]
    if picks.size == 0:
        return 1.0
    assert picks[0] == 0, f"pick 0 is candidate {picks[0]}, not 0"
    assert ((picks >= 0) & (picks < M)).all(), f"picks {np.flatnonzero((picks < 0) | (picks >= M))[:5]} are no candidates"
    dmin = np.full(M, np.inf)
    worst = 1.0
    for k in range(1, picks.size):
        d = np.sum((P - P[picks[k - 1]]) ** 2, axis=1)
        np.minimum(dmin, d, out=dmin)
        best = float(dmin.max())
        got = float(dmin[picks[k]])
        assert got >= (1.0 - rel) * best, f"pick {k}: distance^2 {got!r} < (1 - {rel}) x {best!r}"
        if best > 0.0:
            worst = min(worst, got / best)
    return worst
