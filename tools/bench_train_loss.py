#!/usr/bin/env python
"""The loss of a training iteration at 800 x 800 with everything present -- a non-identity exposure, an alpha mask and the
inverse-depth term -- as

  (a) ``gsworld_amd.ssim.training_loss``: one autograd node, three launches forward and three backward,
  (b) the composition upstream's train.py writes: torch matmul / clamp / mul / abs / mean and ``fused_ssim``,

forward + backward (gradients to the colour, the exposure and the inverse depth), timed with device events, both warmed and
alternated call by call within this one process; and the whole iteration of tools/bench_train.py's configuration (500 k
Gaussians, raw parameters through the rasterizer, another of 8 nearby views every step) with (a) beside the same iteration
with (b).  The two are also compared: value and gradients of (a) against (b) on the same inputs.
Prints one JSON line and writes it to ``--out`` (profiles/train/bench_train_loss.json is a committed run of it).
Usage: bench_train_loss.py [--steps K] [--warmup W] [--num-gaussians N] [--size S] [--out PATH]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gsworld_amd", "dropin"))

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from fused_ssim import fused_ssim  # noqa: E402
from gsworld_amd import scenes  # noqa: E402
from gsworld_amd.camera import look_at_view  # noqa: E402
from gsworld_amd.ssim import training_loss  # noqa: E402

LAMBDA, DEPTH_WEIGHT = 0.2, 0.5


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


def fused_loss(color, gt, E, alpha, invd, mono, mask):
    return training_loss(color, gt, LAMBDA, exposure=E, alpha_mask=alpha, invdepth=invd, mono_invdepth=mono, depth_mask=mask,
                         depth_weight=DEPTH_WEIGHT)


def composed_loss(color, gt, E, alpha, invd, mono, mask):
    y = torch.matmul(color.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
    x = y.clamp(0, 1) * alpha
    loss = (1.0 - LAMBDA) * torch.abs(x - gt).mean() + LAMBDA * (1.0 - fused_ssim(x[None], gt[None]))
    return loss + DEPTH_WEIGHT * torch.abs((invd - mono) * mask).mean()


def run(steps=200, warmup=20, num_gaussians=500_000, size=800, device="cuda:0"):
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    S, N = size, num_gaussians
    gen = torch.Generator().manual_seed(11)
    gt = torch.rand(3, S, S, generator=gen).to(dev)
    color0 = (gt.cpu() + 0.2 * torch.randn(3, S, S, generator=gen)).to(dev)  # (leaves [0, 1] in places)
    E0 = torch.tensor([[1.10, 0.05, -0.03, 0.02], [-0.04, 0.90, 0.06, -0.01], [0.03, -0.02, 1.20, 0.04]], device=dev)
    alpha = (torch.rand(1, S, S, generator=gen) > 0.1).float().to(dev)
    invd0 = (torch.rand(1, S, S, generator=gen) + 0.1).to(dev)
    mono = (invd0.cpu() + 0.3 * torch.randn(1, S, S, generator=gen)).to(dev)
    mask = (torch.rand(1, S, S, generator=gen) > 0.3).float().to(dev)

    def loss_call(fn, backward=True):
        def f():
            c, E, d = (t.detach().requires_grad_(backward) for t in (color0, E0, invd0))
            loss = fn(c, gt, E, alpha, d, mono, mask)
            if backward:
                loss.backward()
            return loss, c.grad, E.grad, d.grad
        return f

    # the same function both ways
    (la, ca, ea, da), (lb, cb, eb, db) = loss_call(fused_loss)(), loss_call(composed_loss)()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    agreement = {"loss_fused": float(la.detach()), "loss_composed": float(lb.detach()), "dcolor_max_rel": rel(ca, cb),
                 "dexposure_max_rel": rel(ea, eb), "dinvdepth_max_rel": rel(da, db)}

    loss_ms = timed_alternating({"fused_fwd_bwd": loss_call(fused_loss), "composed_fwd_bwd": loss_call(composed_loss),
                                 "fused_fwd": loss_call(fused_loss, False), "composed_fwd": loss_call(composed_loss, False)},
                                steps, warmup)

    # the whole iteration of tools/bench_train.py's configuration: 8 views, raw parameters through the rasterizer
    cam = scenes.training_camera(S, S, 60.0).to(dev)
    raw = scenes.random_scene_camera_frame(N, seed=5).to(dev)
    bg = torch.zeros(3, device=dev)
    cams = [cam] + [look_at_view([0.03 * math.cos(k * math.pi / 3.5), 0.03 * math.sin(k * math.pi / 3.5), 0.0],
                                 [0.0, 0.0, 3.0], [0.0, -1.0, 0.0], cam.FoVx, cam.FoVy, S, S).to(dev) for k in range(1, 8)]
    rasts = [GaussianRasterizer(GaussianRasterizationSettings(S, S, c.tanfovx, c.tanfovy, bg, 1.0, c.world_view_transform,
                                                              c.full_proj_transform, 3, c.camera_center, False, False,
                                                              False)) for c in cams]
    params = [raw.xyz, raw.features_dc, raw.features_rest, raw.opacity, raw.scaling, raw.rotation]

    def forward(view, grad=True):
        for p in params:
            p.requires_grad_(grad)
            p.grad = None
        means2D = torch.zeros_like(raw.xyz, requires_grad=grad)
        return rasts[view](means3D=raw.xyz, means2D=means2D, shs=raw.features_dc, shs_rest=raw.features_rest,
                           opacities=raw.opacity, scales=raw.scaling, rotations=raw.rotation, param_space=7)

    with torch.no_grad():
        frames = [forward(v, False) for v in range(len(cams))]
        gts = [(0.9 * f[0].clamp(0, 1)).detach().clone() for f in frames]       # (darker: the exposure has work to do)
        monos = [(f[2] * 1.05).detach().clone() for f in frames]

    def iteration(fn):
        state = {"k": 0}

        def it():
            v = state["k"] % len(cams)
            state["k"] += 1
            color, radii, invd = forward(v)
            E = E0.detach().requires_grad_(True)
            fn(color, gts[v], E, alpha, invd, monos[v], mask).backward()
        return it

    it_ms = timed_alternating({"fused": iteration(fused_loss), "composed": iteration(composed_loss)}, max(steps // 4, 10),
                              max(warmup // 2, 8))
    a, b = loss_ms["fused_fwd_bwd"]["median_ms"], loss_ms["composed_fwd_bwd"]["median_ms"]
    return {
        "metric": "training loss forward + backward at 800x800 with exposure, alpha mask and depth term, ms (median of "
                  "device-event times; both variants alternated within one process)",
        "value": a, "unit": "ms", "steps": steps, "warmup": warmup, "dtype": "f32", "data": "synthetic",
        "loss_ms": loss_ms, "iteration_ms": it_ms, "fused_over_composed_loss": a / b,
        "fused_over_composed_iteration": it_ms["fused"]["median_ms"] / it_ms["composed"]["median_ms"],
        "agreement": agreement,
        "launches": {"fused": "3 forward (prologue, ssim pass, sum) + 3 backward (ssim pass, epilogue, exposure sums)",
                     "composed": "torch elementwise / reduction / matmul launches and their autograd + the two fused_ssim passes"},
        "config": {"size": S, "lambda_dssim": LAMBDA, "depth_weight": DEPTH_WEIGHT, "num_gaussians": N,
                   "iteration": f"{N} Gaussians (config-1 distribution, seed 5), {S}x{S}, forward + loss + backward, another of "
                                "8 nearby views every step (tools/bench_train.py --fused), no optimizer step",
                   "torch": torch.__version__}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--num-gaussians", type=int, default=500_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "bench_train_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_loss.py measures on a HIP device: none found")
    rec = run(args.steps, args.warmup, args.num_gaussians, args.size)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
