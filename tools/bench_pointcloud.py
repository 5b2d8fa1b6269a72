#!/usr/bin/env python
"""What point-cloud observations cost in the closed loop: the configs[2] surrogate (bench.py's closed-loop section -- the
xarm6_align-like scene at 1.47 M Gaussians, two 640 x 480 cameras, the wrist one moving along the episode, robot-link poses
of the seeded xarm6 rollout) run by a ClosedLoopRenderer with segmentation + depth maps only, and with a dense cloud, a
stride-sampled cloud (K = 1024) and an FPS cloud (K = 1024 from 8192 candidates) on top.  Frames/s with the steps enqueued
ahead and with the policy in the loop (``step(ensure=True)``), the same episode twice per loop.  Then the FPS call's device
time (HIP events around 50 calls of the functional API on synthetic 640 x 480 depth maps, one camera) at 1, 8 and 32
environments.  Prints one JSON line.

Per-kernel times come from a separate kernel-trace run of one configuration, e.g. ``rocprofv3 --kernel-trace --stats -d
<dir> -o run -- python tools/bench_pointcloud.py --only fps``: ``pc_*_kernel`` against ``render_maps_kernel`` and
``render_stream_kernel`` there."""
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
from gsworld_amd.pointcloud import PointCloudSpec, render_pointcloud  # noqa: E402

CONFIGS = {"maps": None, "dense": PointCloudSpec(), "stride": PointCloudSpec(num_points=1024, sample="stride"),
           "fps": PointCloudSpec(num_points=1024, sample="fps", fps_candidates=8192)}


def fps_scaling(dev, envs, calls=50):
    """Device ms per FPS call (pixel pass + scan + select + FPS) of E environments, one 640 x 480 camera each."""
    out = {}
    cam = look_at_view([0.6, 0.3, 0.5], [0.0, 0.0, 0.0], [0, 0, 1], 0.9715089, 0.7551448, 640, 480)
    cam.world_view_transform = cam.world_view_transform.to(dev)
    spec = PointCloudSpec(num_points=1024, sample="fps", fps_candidates=8192)
    for E in envs:
        gen = torch.Generator().manual_seed(E)
        depth = (0.3 + torch.rand((E, 480, 640, 1), generator=gen)).to(dev)
        res = render_pointcloud([depth], None, None, [cam], spec)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            render_pointcloud([depth], None, None, [cam], spec, out=res)
        t1.record()
        torch.cuda.synchronize()
        out[str(E)] = round(t0.elapsed_time(t1) / calls, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--num-gaussians", type=int, default=scenes.XARM6_ALIGN_NUM_GAUSSIANS)
    ap.add_argument("--only", choices=sorted(CONFIGS), help="run this loop configuration alone (kernel-trace runs)")
    ap.add_argument("--fps-envs", default="1,8,32")
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

    def run(spec):
        loop = cl.ClosedLoopRenderer(raw, parts, cams, scaled_parts=actors, device=dev, maps=("segmentation", "depth"),
                                     pointcloud=spec)
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
        if spec is not None:
            out["points_last_step"] = int(loop.pointcloud["count"][0])
        del loop
        torch.cuda.empty_cache()
        return out

    res = {"workload": f"configs[2] surrogate: {args.num_gaussians} Gaussians, right_cam fixed + wrist_cam moving, "
                       f"{W}x{H}, {ep + 1} steps, graph captured, segmentation + depth maps in every run",
           "frames_per_episode": frames}
    for name in ([args.only] if args.only else list(CONFIGS)):
        res[name] = run(CONFIGS[name])
    if not args.only:
        for name in ("dense", "stride", "fps"):
            res[f"{name}_ahead_ratio"] = round(res[name]["frames_per_s"] / res["maps"]["frames_per_s"], 4)
            res[f"{name}_policy_ratio"] = round(res[name]["policy_in_loop_frames_per_s"] /
                                                res["maps"]["policy_in_loop_frames_per_s"], 4)
        res["fps_call_ms_by_envs"] = fps_scaling(dev, [int(x) for x in args.fps_envs.split(",") if x])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
