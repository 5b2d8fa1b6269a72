#!/usr/bin/env python
"""What per-environment appearance randomization costs in the closed loop: the configs[2] surrogate (the xarm6_align-like
scene at 1.47 M Gaussians, right_cam fixed + wrist_cam moving at 640 x 480, robot-link poses of the seeded xarm6 rollout) at
E = 1, 4 and 8 environments, three ways:

  a. none    -- today's loop (appearance=None);
  b. reset   -- appearance={robot, objects}: tables and backgrounds drawn once at reset (set_appearance), resting after;
  c. every   -- the same, tables redrawn and handed over on every step (step(appearance=...)).

Frames/s with the steps enqueued ahead and with the policy in the loop (``step(ensure=True)``); graph captured.  Prints one
JSON line.  Kernel times come from a kernel-trace run, e.g. ``rocprofv3 --kernel-trace --stats -d <dir> -o run -- python
tools/bench_appearance.py --envs 4 --only reset``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsworld_amd import appearance as appm  # noqa: E402
from gsworld_amd import closed_loop as cl, scenes  # noqa: E402
from gsworld_amd.camera import look_at_view  # noqa: E402

MODES = ("none", "reset", "every")
GROUPS = {"robot": list(range(1, 17)), "objects": [17, 18]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--num-gaussians", type=int, default=scenes.XARM6_ALIGN_NUM_GAUSSIANS)
    ap.add_argument("--envs", default="1,4,8")
    ap.add_argument("--only", choices=MODES)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    W, H = 640, 480
    raw = scenes.tabletop_scene("xarm6_align", n=args.num_gaussians)
    rollout = cl.xarm6_rollout()
    parts, actors = cl.xarm6_rollout_parts(rollout)
    ep = args.steps
    right = look_at_view([0.75, -0.05, 0.55], [0.3, 0.0, 0.05], [0, 0, 1], 0.9715089, 0.7551448, W, H)
    wrists = []
    for k in range(ep + 1):
        a = 2.0 * np.pi * k / ep
        wrists.append(look_at_view([0.55 - 0.10 * np.sin(a), 0.35, 0.25 + 0.05 * np.sin(2.0 * a)], [0.35, 0.05, 0.05],
                                   [0, 0, 1], 0.9715089, 0.7551448, W, H))

    def run(E, mode):
        poses = list(cl.rollout_poses(rollout, len(actors), steps=ep + 1, seed=0, num_envs=E))
        pinned = [(M.pin_memory(), s.pin_memory()) for M, s in poses]
        loop = cl.ClosedLoopRenderer(raw, parts, {"right_cam": right, "wrist_cam": wrists[0]}, scaled_parts=actors,
                                     device=dev, num_envs=E, appearance=None if mode == "none" else GROUPS)
        rnd = appm.AppearanceRandomizer(3, brightness=(0.7, 1.3), contrast=(0.8, 1.2), saturation=(0.6, 1.4),
                                        hue=(-0.3, 0.3), background=((0, 0, 0), (0.3, 0.3, 0.3)), seed=1)
        draws = [torch.from_numpy(rnd.sample(E)[0]).pin_memory() for _ in range(ep + 1)] if mode == "every" else None
        if mode != "none":
            t, b = rnd.sample(E)
            loop.set_appearance(t, b)
        loop.reset(*pinned[0])
        loop.capture()
        torch.cuda.synchronize()
        frames = (ep + 1) * 2 * E
        res = {}
        for key, ensure in (("frames_per_s", False), ("policy_in_loop_frames_per_s", True)):
            t0 = time.perf_counter()
            for k, (M, s) in enumerate(pinned):
                loop.step(M, s, cameras={"wrist_cam": wrists[k]}, ensure=ensure,
                          appearance=draws[k] if draws is not None else None)
            torch.cuda.synchronize()
            res[key] = round(frames / (time.perf_counter() - t0), 1)
        res["overflow_frames"] = loop.overflow_frames()
        del loop
        torch.cuda.empty_cache()
        return res

    res = {"workload": f"configs[2] surrogate: {args.num_gaussians} Gaussians, right_cam fixed + wrist_cam moving, {W}x{H}, "
                       f"{ep + 1} steps, graph captured, 3 appearance groups"}
    for E in [int(x) for x in args.envs.split(",") if x]:
        r = {m: run(E, m) for m in ([args.only] if args.only else MODES)}
        if not args.only:
            for m in MODES[1:]:
                r[f"{m}_ahead_ratio"] = round(r[m]["frames_per_s"] / r["none"]["frames_per_s"], 4)
                r[f"{m}_policy_ratio"] = round(r[m]["policy_in_loop_frames_per_s"] /
                                               r["none"]["policy_in_loop_frames_per_s"], 4)
        res[f"E{E}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
