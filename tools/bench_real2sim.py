#!/usr/bin/env python
"""The two real2sim workloads at the reference's sizes, on a synthetic tabletop scene (seeded):

  (i)  label transfer -- 1 468 850 scan centres against a 200 k labelled cloud: the index build, the query (under the inverse
       alignment) and the label kernel, each timed alone -- and the same query at distCUDA2's own sizes (the scan's centres
       displaced by 5 mm, against the scan);
  (ii) one ICP iteration -- 200 k sources against the 1 468 850-point scan, correspondence distance 0.03: the query and the
       moment sums (the index over the scan is built once per registration: timed alone too).

Each is set beside what a user would write without the feature, on the same device: chunked ``torch.cdist(...).min(dim=1)``
for the search and a vectorised torch restatement of the label loop; and beside ``distCUDA2`` at 1 468 850 points in the same
process -- the same search shape at a known cost.  Device events, warmed, medians, the routes alternated round by round within
this one process.  Prints one JSON line and writes it to --out (profiles/real2sim/bench_real2sim.json is a committed run).
Usage: bench_real2sim.py [--steps K] [--warmup W] [--brute-steps B] [--scan N] [--cloud M] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsworld_amd import real2sim  # noqa: E402
from gsworld_amd.knn import distCUDA2  # noqa: E402

PARTS = 12
THRESHOLD = 0.1
ICP_DISTANCE = 0.03


def scene(n_scan, n_cloud, dev):
    """A labelled cloud on the surfaces of PARTS boxes inside a 1 m workspace, and a scan of it: 60 % of the centres within
    5 mm of those surfaces, 40 % background (a floor and uniform clutter in a 4 m room), under a similarity."""
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    centre, half = rnd(PARTS, 3) - 0.5, 0.03 + 0.09 * rnd(PARTS, 3)

    def surface(n):
        part = torch.randint(0, PARTS, (n,), device=dev, generator=g)
        p = (2 * rnd(n, 3) - 1)
        face = torch.randint(0, 3, (n,), device=dev, generator=g)
        sign = torch.where(rnd(n) < 0.5, -1.0, 1.0)
        p[torch.arange(n, device=dev), face] = sign
        return centre[part] + half[part] * p, part

    cloud, labels = surface(n_cloud)
    labels = labels.to(torch.int32)
    labels[::50] = -1
    near = int(0.6 * n_scan)
    scan, _ = surface(near)
    scan = scan + 0.005 * torch.randn(near, 3, device=dev, generator=g)
    floor = (rnd((n_scan - near) // 2, 3) - 0.5) * torch.tensor([4.0, 4.0, 0.01], device=dev) - torch.tensor([0, 0, 0.7], device=dev)
    clutter = (rnd(n_scan - near - floor.size(0), 3) - 0.5) * 4.0
    scan = torch.cat([scan, floor, clutter])[torch.randperm(n_scan, device=dev, generator=g)]
    c, s = np.cos(0.35), np.sin(0.35)
    T = np.eye(4)
    T[:3, :3] = 1.1 * np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    T[:3, 3] = (0.2, -0.1, 0.3)
    Tt = torch.from_numpy(T).to(dev)
    scan = (scan.double() @ Tt[:3, :3].T + Tt[:3, 3]).float().contiguous()
    return cloud.contiguous(), labels, scan, T


def brute_nearest(q, ref, transform=None):
    """Chunked torch.cdist(...).min(dim=1): chunks of about 2^30 distances."""
    if transform is not None:
        M = torch.from_numpy(np.asarray(transform, np.float32)).to(q.device)
        q = q @ M[:3, :3].T + M[:3, 3]
    chunk = max(1, (1 << 30) // max(1, ref.size(0)))
    dist, index = [], []
    for a in range(0, q.size(0), chunk):
        d, i = torch.cdist(q[a:a + chunk], ref).min(dim=1)
        dist.append(d)
        index.append(i)
    return torch.cat(index), torch.cat(dist), q


def torch_label_loop(points, index, ref_labels, box_labels, box_bounds, threshold):
    """segment_utils.py:85-112 vectorised in torch: what a user would write on the device without gsr_label_transfer."""
    L = ref_labels[index.long()].long()
    e = torch.maximum(torch.maximum(box_bounds[None, :, :3] - points[:, None, :], torch.zeros((), device=points.device)),
                      points[:, None, :] - box_bounds[None, :, 3:])
    bd = e.pow(2).sum(-1).sqrt()  # (M, rows)
    match = box_labels[None, :].long() == L[:, None]
    has_row = match.any(1)
    own = torch.where(match, bd, torch.full_like(bd, float("inf"))).min(1).values
    qual = torch.where(bd <= threshold, bd, torch.full_like(bd, float("inf")))
    best, row = qual.min(1)  # (the first minimum)
    relabel = torch.where(torch.isfinite(best), box_labels.long()[row], torch.full_like(L, -1))
    out = torch.where(own > threshold, relabel, L)
    return torch.where((L == -1) | ~has_row, torch.full_like(L, -1), out).to(torch.int32)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def run(steps=10, warmup=2, brute_steps=2, n_scan=1_468_850, n_cloud=200_000, device="cuda:0"):
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    cloud, labels, scan, T = scene(n_scan, n_cloud, dev)
    Tinv = np.linalg.inv(T)
    keep = labels >= 0
    boxes = real2sim.semantic_bounding_boxes(cloud[keep], labels[keep])
    del boxes[PARTS - 1]  # a label without a box row
    box_labels = torch.tensor(list(boxes), dtype=torch.int32, device=dev)
    box_bounds = torch.stack([torch.cat(b) for b in boxes.values()]).contiguous()
    L = real2sim._bind()
    import ctypes as C

    times = {}

    def rec(name, ms):
        times.setdefault(name, []).append(ms)

    # preallocated state of the fused routes
    cloud_index = real2sim.NearestIndex(cloud)
    scan_index = real2sim.NearestIndex(scan)
    out_lt = cloud_index.query_raw(scan, transform=Tinv)
    out_icp = scan_index.query_raw(cloud, transform=T, max_dist=ICP_DISTANCE)
    lab_out = torch.empty(n_scan, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def build(index, pts):
        real2sim.check(L.gsr_nn_build(index.n, C.c_void_p(pts.data_ptr()), C.c_void_p(index.mem.data_ptr()), index.index_bytes,
                                      stream))

    def label_kernel():
        a = real2sim.GsrLabelTransfer(struct_size=C.sizeof(real2sim.GsrLabelTransfer), n=n_scan, index=out_lt[0].data_ptr(),
                                      points=out_lt[2].data_ptr(), ref_labels=labels.data_ptr(), n_ref=n_cloud,
                                      n_boxes=len(boxes), box_labels=box_labels.data_ptr(), box_bounds=box_bounds.data_ptr(),
                                      threshold=THRESHOLD, labels=lab_out.data_ptr())
        real2sim.check(L.gsr_label_transfer(C.byref(a), stream))

    knn_out = torch.empty(n_scan, device=dev)
    # the query at distCUDA2's own sizes: the scan's centres displaced by N(0, 5 mm) against the scan itself
    shifted = scan + 0.005 * torch.randn(scan.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    out_eq = scan_index.query_raw(shifted)
    brute = {}
    for r in range(warmup + steps):
        w = r >= warmup
        for name, f in (("label_transfer.build_200k", lambda: build(cloud_index, cloud)),
                        ("label_transfer.query", lambda: cloud_index.query_raw(scan, transform=Tinv, out=out_lt)),
                        ("label_transfer.label_kernel", label_kernel),
                        ("label_transfer.label_torch_restatement",
                         lambda: torch_label_loop(out_lt[2], out_lt[0], labels, box_labels, box_bounds, THRESHOLD)),
                        ("icp.build_scan", lambda: build(scan_index, scan)),
                        ("icp.query", lambda: scan_index.query_raw(cloud, transform=T, max_dist=ICP_DISTANCE, out=out_icp)),
                        ("icp.moments", lambda: scan_index.moments(cloud, T, out_icp[0], out_icp[1])),
                        ("equal_size.query_scan_vs_scan", lambda: scan_index.query_raw(shifted, out=out_eq)),
                        ("distCUDA2_scan", lambda: distCUDA2(scan, out=knn_out))):
            ms, res = timed(f)
            if w:
                rec(name, ms)
            if name == "label_transfer.label_torch_restatement":
                brute["labels"] = res
        if r < 1 + brute_steps:  # (the first of them is the warm-up)
            for name, f in (("label_transfer.brute_cdist", lambda: brute_nearest(scan, cloud, Tinv)),
                            ("icp.brute_cdist", lambda: brute_nearest(cloud, scan, T))):
                ms, res = timed(f)
                if r >= 1:
                    rec(name, ms)
                brute[name] = res

    # what the two routes computed, compared at the size that was timed (cdist goes through a matrix product: it is the less
    # exact of the two, so differing indices are compared by the distance they reach)
    def agreement(ours, theirs, ref, limit=None):
        index, dist2, moved = ours
        bi, bd, _ = theirs
        found = index >= 0
        same = (index.long() == bi)[found].float().mean().item()
        mine = (moved[found] - ref[index[found].long()]).double().pow(2).sum(1).sqrt()
        other = (moved[found] - ref[bi[found]]).double().pow(2).sum(1).sqrt()
        out = {"same_index_fraction": same, "ours_farther_than_cdist_max": float((mine - other).max()),
               "cdist_farther_than_ours_max": float((other - mine).max())}
        if limit is not None:
            out["inliers"] = int(found.sum())
            out["cdist_inliers"] = int((bd <= limit).sum())
        return out

    agree = {"label_transfer": agreement(out_lt, brute["label_transfer.brute_cdist"], cloud),
             "icp": agreement(out_icp, brute["icp.brute_cdist"], scan, ICP_DISTANCE),
             "labels_equal_fraction": (lab_out == brute["labels"]).float().mean().item(),
             "labelled_fraction": (lab_out >= 0).float().mean().item()}
    t = {k: stats(v) for k, v in times.items()}
    med = lambda k: t[k]["median_ms"]  # noqa: E731
    return {
        "metric": "label-transfer query, ms: nearest labelled point of 200 k for 1 468 850 scan centres (median of "
                  "device-event times; routes alternated within one process)",
        "value": med("label_transfer.query"), "unit": "ms", "steps": steps, "warmup": warmup, "brute_steps": brute_steps,
        "dtype": "f32", "data": "synthetic", "times": t,
        "speedup": {"label_transfer.query_vs_cdist": med("label_transfer.brute_cdist") / med("label_transfer.query"),
                    "label_transfer.label_kernel_vs_torch": med("label_transfer.label_torch_restatement") / med("label_transfer.label_kernel"),
                    "icp.query_vs_cdist": med("icp.brute_cdist") / med("icp.query")},
        "yardsticks": {"distCUDA2_scan_ms": med("distCUDA2_scan"),
                       "query_scan_vs_scan_ms": med("equal_size.query_scan_vs_scan"),
                       "icp_iteration_ms": med("icp.query") + med("icp.moments"),
                       "label_transfer_total_ms": med("label_transfer.build_200k") + med("label_transfer.query") + med("label_transfer.label_kernel")},
        "agreement": agree,
        "config": {"scan_points": n_scan, "cloud_points": n_cloud, "boxes": len(boxes), "threshold": THRESHOLD,
                   "icp_distance": ICP_DISTANCE, "scene": scene.__doc__.strip().replace("\n   ", ""), "torch": torch.__version__}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--brute-steps", type=int, default=2)
    ap.add_argument("--scan", type=int, default=1_468_850)
    ap.add_argument("--cloud", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real2sim", "bench_real2sim.json"))
    args = ap.parse_args()
    line = json.dumps(run(args.steps, args.warmup, args.brute_steps, args.scan, args.cloud))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
