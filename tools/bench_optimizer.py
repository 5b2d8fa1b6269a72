#!/usr/bin/env python
"""The optimizer step of BASELINE.json configs[4] (500 k Gaussians, degree 3, 800 x 800): the six parameter tensors and the
gradients of one real backward at that view, stepped by

  (a) torch.optim.Adam (its default implementation),
  (b) torch.optim.Adam(fused=True), where this torch build accepts it,
  (c) gsworld_amd.optim.SparseGaussianAdam with every Gaussian visible (the bytes of (a) / (b)),
  (d) SparseGaussianAdam with the view's own radii (V of N Gaussians visible),
  (e) beside them, SparseGaussianAdam with a seeded random mask of 30 % (that view sees nearly every Gaussian),

timed with device events, every variant warmed, the variants alternated step by step within this one process; and the whole
training iteration (fused forward + photometric_loss + backward + densification statistics + optimizer) with (d) beside the
same iteration with (a).  Prints one JSON line (profiles/optim/bench_optimizer.json is a committed run of it).
Usage: bench_optimizer.py [--steps K] [--warmup W] [--num-gaussians N] [--size S]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gsworld_amd", "dropin"))

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from gsworld_amd import scenes  # noqa: E402
from gsworld_amd.optim import SparseGaussianAdam, densification_stats  # noqa: E402
from gsworld_amd.ssim import photometric_loss  # noqa: E402

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = (1.6e-4, 2.5e-3, 2.5e-3 / 20.0, 2.5e-2, 5e-3, 1e-3)  # upstream's defaults (spatial_lr_scale 1)
HBM_PEAK_GBS = 8000.0


def model_tensors(raw):
    return [raw.xyz, raw.features_dc, raw.features_rest, raw.opacity, raw.scaling, raw.rotation]


def fresh_params(tensors):
    return [torch.nn.Parameter(t.detach().clone().contiguous()) for t in tensors]


def groups_of(params):
    return [{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(params, LRS, NAMES)]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "mean_ms": sum(ms) / len(ms), "min_ms": ms[0],
            "p90_ms": ms[int(0.9 * (len(ms) - 1))]}


def timed_alternating(fns: dict, steps: int, warmup: int) -> dict:
    """Each round runs every function once between two device events; -> per-function statistics over ``steps`` rounds."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(steps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def run(steps=200, warmup=20, num_gaussians=500_000, size=800, device="cuda:0"):
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    S, N = size, num_gaussians
    cam = scenes.training_camera(S, S, 60.0).to(dev)
    raw = scenes.random_scene_camera_frame(N, seed=5).to(dev)
    tgt = scenes.random_scene_camera_frame(N, seed=5).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(6)
    tgt.xyz += (0.01 * torch.randn(tgt.xyz.shape, generator=gen)).to(dev)
    tgt.features_dc += (0.1 * torch.randn(tgt.features_dc.shape, generator=gen)).to(dev)
    bg = torch.zeros(3, device=dev)
    rast = GaussianRasterizer(GaussianRasterizationSettings(S, S, cam.tanfovx, cam.tanfovy, bg, 1.0, cam.world_view_transform,
                                                            cam.full_proj_transform, 3, cam.camera_center, False, False, False))

    def forward(params, grad=True):
        xyz, dc, rest, op, sc, rot = params
        means2D = torch.zeros_like(xyz, requires_grad=grad)
        color, radii, _ = rast(means3D=xyz, means2D=means2D, shs=dc, shs_rest=rest, opacities=op, scales=sc, rotations=rot,
                               param_space=7)
        return color, radii, means2D

    with torch.no_grad():
        gt = forward(model_tensors(tgt), grad=False)[0].clamp(0, 1)

    # one real backward at this view: the gradients every optimizer variant steps with
    base = fresh_params(model_tensors(raw))
    color, radii, means2D = forward(base)
    photometric_loss(color, gt, 0.2, clamp01=True).backward()
    grads = [p.grad.detach().contiguous() for p in base]
    radii = radii.detach().clone()
    V = int((radii > 0).sum().item())
    M_total = sum(p[0].numel() for p in base)

    def variant(make, visible=None, sparse=False):
        params = fresh_params(model_tensors(raw))
        for p, g in zip(params, grads):
            p.grad = g
        opt = make(groups_of(params))
        return (lambda: opt.step(visible, N)) if sparse else opt.step

    fns = {"a_torch_adam": variant(lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15))}
    fused_note = None
    try:
        fns["b_torch_adam_fused"] = variant(lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15, fused=True))
        fns["b_torch_adam_fused"]()
    except Exception as ex:  # noqa: BLE001  (this torch build has no fused Adam for these tensors)
        fns.pop("b_torch_adam_fused", None)
        fused_note = f"{type(ex).__name__}: {ex}"[:200]
    fns["c_sparse_all_visible"] = variant(lambda g: SparseGaussianAdam(g, lr=0.0, eps=1e-15), None, True)
    fns["d_sparse_view_radii"] = variant(lambda g: SparseGaussianAdam(g, lr=0.0, eps=1e-15), radii, True)
    # (configs[4]'s view sees nearly every Gaussian: a seeded random mask of 30 % beside it shows what sparsity is worth)
    mask = (torch.rand(N, generator=torch.Generator().manual_seed(7)) < 0.3).to(dev)
    V_mask = int(mask.sum().item())
    fns["e_sparse_random_mask_0.3"] = variant(lambda g: SparseGaussianAdam(g, lr=0.0, eps=1e-15), mask, True)
    opt_ms = timed_alternating(fns, steps, warmup)

    # the whole iteration, two models side by side
    def iteration(make, sparse):
        params = fresh_params(model_tensors(raw))
        opt = make(groups_of(params))
        accum, denom, maxr = (torch.zeros(N, device=dev) for _ in range(3))

        def it():
            color, radii, means2D = forward(params)
            photometric_loss(color, gt, 0.2, clamp01=True).backward()
            densification_stats(radii, means2D.grad, accum, denom, maxr)
            if sparse:
                opt.step(radii, N)
            else:
                opt.step()
            opt.zero_grad(set_to_none=True)
        return it

    it_ms = timed_alternating({"sparse_view_radii": iteration(lambda g: SparseGaussianAdam(g, lr=0.0, eps=1e-15), True),
                               "torch_adam": iteration(lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15), False)},
                              steps, warmup)

    def share(v_rows, ms, mask_bytes):
        b = 28 * M_total * v_rows + mask_bytes
        return {"algorithmic_bytes": int(b), "GBs": b / (ms * 1e-3) / 1e9, "frac_of_8TBs": b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}

    c, d = opt_ms["c_sparse_all_visible"]["median_ms"], opt_ms["d_sparse_view_radii"]["median_ms"]
    ref_key = "b_torch_adam_fused" if "b_torch_adam_fused" in opt_ms else "a_torch_adam"
    return {
        "metric": "optimizer step, ms (median of device-event times; variants alternated within one process)",
        "value": d, "unit": "ms", "steps": steps, "warmup": warmup, "dtype": "f32", "data": "synthetic",
        "optimizer_step_ms": opt_ms, "iteration_ms": it_ms,
        "c_over_" + ref_key: c / opt_ms[ref_key]["median_ms"], "d_over_c": d / c,
        "torch_adam_fused": "available" if fused_note is None else f"not available ({fused_note})",
        "roofline": {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "c_all_visible": share(N, c, 0), "d_view_radii": share(V, d, 4 * N),
                     "e_random_mask_0.3": dict(share(V_mask, opt_ms["e_sparse_random_mask_0.3"]["median_ms"], N),
                                               num_visible=V_mask),
                     "note": "28 M_total V + 4 N bytes (param r/w, grad r, two moments r/w of the visible Gaussians + the radii) "
                             "over the event time of the one launch"},
        "config": {"workload": f"{N} Gaussians (config-1 distribution, seed 5), {S}x{S}, degree 3: six parameter tensors, "
                               f"{M_total} floats per Gaussian, gradients of one backward at the view (BASELINE.json configs[4])",
                   "num_gaussians": N, "num_visible": V, "visible_fraction": V / N, "lrs": dict(zip(NAMES, LRS)),
                   "eps": 1e-15, "torch": torch.__version__}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--num-gaussians", type=int, default=500_000)
    ap.add_argument("--size", type=int, default=800)
    args = ap.parse_args()
    print(json.dumps(run(args.steps, args.warmup, args.num_gaussians, args.size)))


if __name__ == "__main__":
    main()
