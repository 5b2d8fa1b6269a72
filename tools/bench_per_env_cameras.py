#!/usr/bin/env python
"""What per-environment cameras cost in the closed loop: the configs[2] surrogate (bench.py's closed-loop section -- the
xarm6_align-like scene at 1.47 M Gaussians, right_cam fixed + wrist_cam moving at 640 x 480, robot-link poses of the seeded
xarm6 rollout) at E = 1, 4 and 8 environments, every environment given the SAME cameras, fed five ways:

  a. shared    -- today's loop: one ViewParams per camera for every environment (cameras={"wrist_cam": vp});
  b. lists     -- per_env_cameras=True, a list of E ViewParams per moving camera;
  c. host_ext  -- per_env_cameras=True, sim2real: the simulator's (E,3,4) extrinsic_cv as a pinned host tensor,
                  converted on the device inside the step (gsr_cameras_from_extrinsics);
  d. dev_ext   -- the same extrinsics as a device tensor (a GPU simulator's);
  e. host_conv -- the alternative without this feature: cam_maniskill2gs on the host per environment per camera per step,
                  fed as (b).

Frames/s with the steps enqueued ahead and with the policy in the loop (``step(ensure=True)``); graph captured.  Prints one
JSON line.  The conversion kernel's own time comes from a kernel-trace run, e.g. ``rocprofv3 --kernel-trace --stats -d <dir>
-o run -- python tools/bench_per_env_cameras.py --envs 8 --only host_ext``: ``cameras_kernel`` there."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsworld_amd import closed_loop as cl, scenes  # noqa: E402
from gsworld_amd.camera import cam_maniskill2gs, look_at_view  # noqa: E402

MODES = ("shared", "lists", "host_ext", "dev_ext", "host_conv")


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
    # a wrist_cam extrinsic per step; the scene camera it converts to is what every mode renders
    rigid = torch.eye(4)
    th = 0.3
    rigid[:2, :2] = torch.tensor([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    rigid[:3, 3] = torch.tensor([0.1, -0.05, 0.02])
    scale = 1.2
    K = torch.tensor([[605.0, 0.0, 320.0], [0.0, 605.0, 240.0], [0.0, 0.0, 1.0]])
    fovx, fovy = 2 * math.atan(W / (2 * 605.0)), 2 * math.atan(H / (2 * 605.0))

    def ext_at(k):
        a = 2.0 * math.pi * k / ep
        v = look_at_view([0.55 - 0.10 * math.sin(a), 0.35, 0.25 + 0.05 * math.sin(2.0 * a)], [0.35, 0.05, 0.05], [0, 0, 1],
                         fovx, fovy, W, H)
        w2c = v.world_view_transform.double().numpy().T
        c2w = np.linalg.inv(rigid.double().numpy()) @ np.linalg.inv(w2c)
        c2w[:3, 3] /= scale
        return torch.from_numpy(np.linalg.inv(c2w)[:3].astype(np.float32))

    exts = [ext_at(k) for k in range(ep + 1)]
    right_ext = ext_at(ep // 4)
    right = cam_maniskill2gs(right_ext, K, W, H, rigid, scale)

    def pin(v):
        v.world_view_transform = v.world_view_transform.pin_memory()
        v.full_proj_transform = v.full_proj_transform.pin_memory()
        v.camera_center = v.camera_center.pin_memory()
        return v

    wrists = [pin(cam_maniskill2gs(x, K, W, H, rigid, scale)) for x in exts]

    def run(E, mode):
        poses = list(cl.rollout_poses(rollout, len(actors), steps=ep + 1, seed=0, num_envs=E))
        pinned = [(M.pin_memory(), s.pin_memory()) for M, s in poses]
        per_env = mode != "shared"
        cams = {"right_cam": right, "wrist_cam": wrists[0]}
        loop = cl.ClosedLoopRenderer(raw, parts, cams, scaled_parts=actors, device=dev, num_envs=E, per_env_cameras=per_env,
                                     sim2real=(rigid, scale) if mode in ("host_ext", "dev_ext") else None)
        if mode == "host_ext":
            feed = [dict(extrinsics={"wrist_cam": x.expand(E, 3, 4).contiguous().pin_memory()}) for x in exts]
        elif mode == "dev_ext":
            feed = [dict(extrinsics={"wrist_cam": x.expand(E, 3, 4).contiguous().to(dev)}) for x in exts]
        elif mode == "lists":
            feed = [dict(cameras={"wrist_cam": [w] * E}) for w in wrists]
        elif mode == "shared":
            feed = [dict(cameras={"wrist_cam": w}) for w in wrists]
        else:
            feed = None
        ext_e = [x.expand(E, 3, 4) for x in exts]

        def step_kw(k):
            if feed is not None:
                return feed[k]
            # (e) the host conversion of every environment's camera, every step
            return dict(cameras={"wrist_cam": [cam_maniskill2gs(ext_e[k][e], K, W, H, rigid, scale) for e in range(E)]})

        if feed is not None and "extrinsics" in feed[0]:
            loop.set_extrinsics(feed[0]["extrinsics"])
        loop.reset(*pinned[0])
        loop.capture()
        torch.cuda.synchronize()
        frames = (ep + 1) * 2 * E
        t0 = time.perf_counter()
        for k, (M, s) in enumerate(pinned):
            loop.step(M, s, **step_kw(k))
        torch.cuda.synchronize()
        ahead = frames / (time.perf_counter() - t0)
        t0 = time.perf_counter()
        for k, (M, s) in enumerate(pinned):
            loop.step(M, s, ensure=True, **step_kw(k))
        policy = frames / (time.perf_counter() - t0)
        out = {"frames_per_s": round(ahead, 1), "policy_in_loop_frames_per_s": round(policy, 1),
               "overflow_frames": loop.overflow_frames()}
        del loop
        torch.cuda.empty_cache()
        return out

    res = {"workload": f"configs[2] surrogate: {args.num_gaussians} Gaussians, right_cam fixed + wrist_cam moving, {W}x{H}, "
                       f"{ep + 1} steps, graph captured, the same cameras in every environment"}
    for E in [int(x) for x in args.envs.split(",") if x]:
        r = {m: run(E, m) for m in ([args.only] if args.only else MODES)}
        if not args.only:
            for m in MODES[1:]:
                r[f"{m}_ahead_ratio"] = round(r[m]["frames_per_s"] / r["shared"]["frames_per_s"], 4)
                r[f"{m}_policy_ratio"] = round(r[m]["policy_in_loop_frames_per_s"] /
                                               r["shared"]["policy_in_loop_frames_per_s"], 4)
        res[f"E{E}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
