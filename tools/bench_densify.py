#!/usr/bin/env python
"""One densify_and_prune of BASELINE.json configs[4] (500 k Gaussians, degree 3, 800 x 800): a GaussianModel(3, "sparse_adam")
with the statistics of a few real training iterations at that view, densified by

  (a) the fused route -- gsworld_amd.optim.densify_and_prune: plan (three launches), ONE host read, apply (one launch) --,
  (b) the literal sequence -- upstream's densify_and_clone / densify_and_split / prune_points on the model's prune_points /
      densification_postfix hooks (a subclass that overrides both takes it) --,

from the same state (restored on the host before every call), timed with device events and with the host clock, both warmed,
alternated call by call within this one process; and the fused route's two calls alone -- gsr_densify_plan and
gsr_densify_apply on preallocated buffers -- priced against the bytes they must move.  Two workloads: thresholds
that are medians of the state's own statistics (half of the Gaussians with a gradient are hot, half of all are small, 2 % are
transparent), and a gradient threshold of 0 (every Gaussian is cloned or split: growth at its limit).  Prints one JSON line and writes it to --out (profiles/optim/bench_densify.json is a committed run of it).
Usage: bench_densify.py [--steps K] [--warmup W] [--num-gaussians N] [--size S] [--iterations I] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gsworld_amd", "dropin"))
sys.path.insert(0, os.path.join(ROOT, "gsworld_amd", "gs_compat"))

from gaussian_renderer import render  # noqa: E402
from scene.gaussian_model import GaussianModel  # noqa: E402

from gsworld_amd import _C, scenes  # noqa: E402
from gsworld_amd.ssim import photometric_loss  # noqa: E402

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
HBM_PEAK_GBS = 8000.0
PERCENT_DENSE = 0.01
TRAIN_ARGS = types.SimpleNamespace(percent_dense=PERCENT_DENSE, position_lr_init=1.6e-4, feature_lr=2.5e-3, opacity_lr=2.5e-2,
                                   scaling_lr=5e-3, rotation_lr=1e-3)


class HookedModel(GaussianModel):
    """Overrides both hooks (as GSWorld's Semantic3DGSWrapper does): densify_and_prune takes the literal sequence."""

    def prune_points(self, mask):
        super().prune_points(mask)

    def densification_postfix(self, *args):
        super().densification_postfix(*args)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "mean_ms": sum(ms) / len(ms), "min_ms": ms[0],
            "p90_ms": ms[int(0.9 * (len(ms) - 1))]}


def timed_alternating(fns: dict, steps: int, warmup: int) -> dict:
    """``fns``: name -> (prepare, run).  Each round prepares (host only, untimed) and runs every function once between two
    device events and two host clock reads (the device idle before, synchronised after); -> per-function statistics."""
    ev, wall = {k: [] for k in fns}, {k: [] for k in fns}
    for r in range(warmup + steps):
        for k, (prepare, f) in fns.items():
            prepare()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= warmup:
                ev[k].append(a.elapsed_time(b))
                wall[k].append((t1 - t0) * 1e3)
    return {k: {"device_events": stats(ev[k]), "host_clock": stats(wall[k])} for k in fns}


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


def run(steps=20, warmup=3, num_gaussians=500_000, size=800, iterations=3, device="cuda:0"):
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    S, N = size, num_gaussians
    cam = scenes.training_camera(S, S, 60.0).to(dev)
    raw = scenes.random_scene_camera_frame(N, seed=5)
    pipe = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, antialiasing=False)
    bg = torch.zeros(3, device=dev)
    gt = torch.rand(3, S, S, generator=torch.Generator().manual_seed(8)).to(dev)
    pc = model_from(GaussianModel, raw, dev)
    for _ in range(iterations):  # real statistics and real moments
        out = render(cam, pc, pipe, bg)
        photometric_loss(out["render"], gt, 0.2).backward()
        pc.add_densification_stats(out["viewspace_points"], out["radii"])
        pc.optimizer.step(out["radii"], N)
        pc.optimizer.zero_grad(set_to_none=True)
    radii = out["radii"].detach()

    # thresholds: the medians of the state's own statistics
    with torch.no_grad():
        g = (pc.xyz_gradient_accum / pc.denom).nan_to_num(0.0).reshape(-1)
        max_grad = float(g[g > 0].median())  # (many seen Gaussians contribute to no pixel: their quotient is 0)
        dense_limit = float(pc.get_scaling.max(dim=1).values.median())
        extent = dense_limit / PERCENT_DENSE
        min_opacity = float(pc.get_opacity.reshape(-1).kthvalue(max(1, N // 50)).values)  # prunes 2 %

    # the state both routes start from, and the same state in a model whose class overrides the hooks
    hooked = model_from(HookedModel, raw, dev)
    snap = {}
    for model in (pc, hooked):
        cur = model._current()
        if model is hooked:
            for n in NAMES:
                cur[n].data.copy_(pc._current()[n].data)
                hooked.optimizer.state[cur[n]] = {k: v.clone() for k, v in pc.optimizer.state[pc._current()[n]].items()}
            hooked.xyz_gradient_accum, hooked.denom = pc.xyz_gradient_accum.clone(), pc.denom.clone()
            hooked.max_radii2D = pc.max_radii2D.clone()
        snap[model] = (dict(cur), {n: dict(model.optimizer.state[cur[n]]) for n in NAMES},
                       (model.xyz_gradient_accum, model.denom, model.max_radii2D))

    def restore(model):
        def f():
            cur, state, side = snap[model]
            for group in model.optimizer.param_groups:
                model.optimizer.state.pop(group["params"][0], None)
                group["params"][0] = cur[group["name"]]
                model.optimizer.state[cur[group["name"]]] = dict(state[group["name"]])
            model._rebind(cur)
            model.xyz_gradient_accum, model.denom, model.max_radii2D = side
        return f

    noise = torch.randn(N, 2, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(4))

    def share(b, ms):
        return {"algorithmic_bytes": int(b), "GBs": b / (ms * 1e-3) / 1e9, "frac_of_8TBs": b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}

    def measure(max_grad):
        counts = {}

        def densify(model):
            def f():
                model.densify_and_prune(max_grad, min_opacity, extent, 20, radii, noise=noise)
                counts[model.last_densify_route] = model.get_xyz.shape[0]
            return f

        route_ms = timed_alternating({"fused": (restore(pc), densify(pc)), "literal": (restore(hooked), densify(hooked))},
                                     steps, warmup)
        assert pc.last_densify_route == "fused" and hooked.last_densify_route == "literal"
        assert counts["fused"] == counts["literal"], counts
        restore(pc)()
        restore(hooked)()

        # the two calls of the fused route alone, on preallocated buffers
        cur, state, _ = snap[pc]
        f32 = np.float32
        plan_args = dict(grad_threshold=max_grad, min_opacity=min_opacity, dense_limit=f32(PERCENT_DENSE) * f32(extent),
                         world_limit=f32(0.1) * f32(extent), prune_world_size=True)
        cnt, ws = _C.densify_plan(pc.xyz_gradient_accum, pc.denom, cur["scaling"].detach(), cur["opacity"].detach(),
                                  **plan_args)
        K, Cn, Sp, n_out = (int(c) for c in cnt.tolist())
        assert n_out == counts["fused"]
        groups = []
        for n in NAMES:
            p = cur[n].detach()
            shape = (n_out,) + tuple(p.shape[1:])
            groups.append({"src": (p, state[n]["exp_avg"], state[n]["exp_avg_sq"]),
                           "dst": tuple(torch.empty(shape, device=dev) for _ in range(3)), "M": p[0].numel(),
                           "role": n if n in ("xyz", "scaling") else "copy"})
        parent = torch.empty((n_out,), dtype=torch.int32, device=dev)
        nothing = lambda: None  # noqa: E731
        call_ms = timed_alternating({
            "plan": (nothing, lambda: _C.densify_plan(pc.xyz_gradient_accum, pc.denom, cur["scaling"].detach(),
                                                      cur["opacity"].detach(), counts=cnt, workspace=ws, **plan_args)),
            "apply": (nothing, lambda: _C.densify_apply(N, n_out, ws, cur["xyz"].detach(), cur["scaling"].detach(),
                                                        cur["rotation"].detach(), noise, groups, parent))}, steps * 5, warmup)
        M_total = sum(g["M"] for g in groups)
        new = n_out - K
        apply_bytes = 12 * M_total * n_out + 4 * n_out + (12 * M_total * K + 4 * M_total * new + 4 * n_out * len(NAMES))
        plan_bytes = 4 * N * 6 + 2 * N + 12 * (N // 256) + 4 * n_out
        fused, literal = route_ms["fused"], route_ms["literal"]
        return {"max_grad": max_grad, "kept": K, "clones": Cn, "split": Sp, "num_out": n_out, "densify_and_prune_ms": route_ms,
                "fused_over_literal": {k: fused[k]["median_ms"] / literal[k]["median_ms"] for k in ("device_events", "host_clock")},
                "fused_calls_ms": call_ms,
                "roofline": {"plan": share(plan_bytes, call_ms["plan"]["device_events"]["median_ms"]),
                             "apply": share(apply_bytes, call_ms["apply"]["device_events"]["median_ms"])}}

    # two workloads: the state's own statistics (an occluded random cloud: few Gaussians have a gradient at all, so this is
    # nearly a pure prune), and growth at its limit (threshold 0: every Gaussian is cloned or split, N_out ~ 2 N)
    own = measure(max_grad)
    growth = measure(0.0)
    M_total = sum(p[0].numel() for p in snap[pc][0].values())
    return {
        "metric": "one densify_and_prune, ms (median of device-event times; routes alternated within one process)",
        "value": own["densify_and_prune_ms"]["fused"]["device_events"]["median_ms"], "unit": "ms", "steps": steps,
        "warmup": warmup, "dtype": "f32", "data": "synthetic", "own_statistics": own, "every_gaussian_hot": growth,
        "roofline": {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "note": "apply: 12 M_total N_out written (parameter and two moments of every output row) + the parent "
                             "output + what must be read (12 M_total per kept row, 4 M_total per new row, the row map once per "
                             "group); plan: accum, denom, scaling, opacity read, one flag byte written and read, the row map "
                             "written -- over the event time of the launches"},
        "config": {"workload": f"{N} Gaussians (config-1 distribution, seed 5), {S}x{S}, degree 3: six parameter tensors and "
                               f"their moments, {M_total} floats per Gaussian, statistics of {iterations} training iterations "
                               "at the view (BASELINE.json configs[4])",
                   "num_gaussians": N, "min_opacity": min_opacity, "extent": extent, "percent_dense": PERCENT_DENSE,
                   "torch": torch.__version__}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--num-gaussians", type=int, default=500_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim", "bench_densify.json"))
    args = ap.parse_args()
    line = json.dumps(run(args.steps, args.warmup, args.num_gaussians, args.size, args.iterations))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
