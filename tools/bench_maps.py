#!/usr/bin/env python
"""What segmentation / depth maps cost in the closed loop: the configs[2] surrogate (bench.py's closed-loop section -- the
xarm6_align-like scene at 1.47 M Gaussians, two 640 x 480 cameras, the wrist one moving along the episode, robot-link poses
of the seeded xarm6 rollout) run by a ClosedLoopRenderer without and with ``maps=("segmentation", "depth")``.  Frames/s
with the steps enqueued ahead (random-action rollout) and with the policy in the loop (``step(ensure=True)``: a host wait
per step), the same episode twice per loop.  Prints one JSON line.

The maps kernel's time per frame against the compositor's comes from a separate kernel-trace run of this script
(``--only-maps``: the maps loop alone), e.g. ``rocprofv3 --kernel-trace --stats -d <dir> -o run -- python
tools/bench_maps.py --only-maps``: compare ``render_maps_kernel`` with ``render_stream_kernel`` there."""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsworld_amd import closed_loop as cl, scenes  # noqa: E402
from gsworld_amd.camera import look_at_view  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--num-gaussians", type=int, default=scenes.XARM6_ALIGN_NUM_GAUSSIANS)
    ap.add_argument("--only-maps", action="store_true", help="run the loop with maps only (kernel-trace runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    W, H = 640, 480
    raw = scenes.tabletop_scene("xarm6_align", n=args.num_gaussians)
    cams = {"right_cam": scenes.sensor_camera("xarm6_align", W, H),
            "wrist_cam": look_at_view([0.55, 0.35, 0.25], [0.35, 0.05, 0.05], [0, 0, 1], 0.9715089, 0.7551448, W, H)}
    rollout = cl.xarm6_rollout()
    parts, actors = cl.xarm6_rollout_parts(rollout)
    ep = args.steps
    poses = list(cl.rollout_poses(rollout, len(actors), steps=ep + 1, seed=0))
    pinned = [(M.pin_memory(), s.pin_memory()) for M, s in poses]

    def wrist_at(k):  # (bench.py: the wrist camera rides on the arm, a 10 cm sweep over the episode)
        a = 2.0 * math.pi * k / ep
        v = look_at_view([0.55 - 0.10 * math.sin(a), 0.35, 0.25 + 0.05 * math.sin(2.0 * a)], [0.35, 0.05, 0.05], [0, 0, 1],
                         0.9715089, 0.7551448, W, H)
        v.world_view_transform = v.world_view_transform.pin_memory()
        v.full_proj_transform = v.full_proj_transform.pin_memory()
        v.camera_center = v.camera_center.pin_memory()
        return v

    wrists = [wrist_at(k) for k in range(ep + 1)]
    frames = (ep + 1) * len(cams)

    def run(maps):
        loop = cl.ClosedLoopRenderer(raw, parts, cams, scaled_parts=actors, device=dev, maps=maps)
        loop.reset(*pinned[0])
        loop.capture()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for (M, s), w in zip(pinned, wrists):
            loop.step(M, s, cameras={"wrist_cam": w})
        torch.cuda.synchronize()
        ahead = frames / (time.perf_counter() - t0)
        t0 = time.perf_counter()
        for (M, s), w in zip(pinned, wrists):
            loop.step(M, s, cameras={"wrist_cam": w}, ensure=True)
        policy = frames / (time.perf_counter() - t0)
        out = {"frames_per_s": round(ahead, 1), "policy_in_loop_frames_per_s": round(policy, 1),
               "overflow_frames": loop.overflow_frames()}
        if maps:
            seg = loop.maps["right_cam"]["segmentation"]
            out["right_cam_labelled_pixel_fraction"] = round(float((seg >= 0).float().mean()), 4)
        del loop
        torch.cuda.empty_cache()
        return out

    res = {"workload": f"configs[2] surrogate: {args.num_gaussians} Gaussians, right_cam fixed + wrist_cam moving, "
                       f"{W}x{H}, {ep + 1} steps, graph captured", "frames_per_episode": frames}
    if not args.only_maps:
        res["without_maps"] = run(())
    res["with_maps"] = run(("segmentation", "depth"))
    if not args.only_maps:
        res["ahead_ratio"] = round(res["with_maps"]["frames_per_s"] / res["without_maps"]["frames_per_s"], 4)
        res["policy_ratio"] = round(res["with_maps"]["policy_in_loop_frames_per_s"] /
                                    res["without_maps"]["policy_in_loop_frames_per_s"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
