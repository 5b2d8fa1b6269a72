#!/usr/bin/env python
"""From a trained scan to the per-Gaussian labels a scene config names: every Gaussian centre of the scan is brought into the
frame of a labelled source cloud (the inverse of the 4 x 4 matrix that ``gsworld_amd.real2sim.registration_icp`` -- or any
alignment -- gave: matrix @ source = scan), takes the label of its nearest labelled point, and is validated against
per-label bounding boxes (GSWorld real2sim/scripts/segment_real_gs.py:82-105).  Writes ``<scan>_semantics_gs.npy``: int
labels, -1 = unlabelled -- the file ``GaussianModelMerger.assign_semantic_labels`` takes.

  scan      a Gaussian PLY (only x / y / z are read)
  source    the labelled cloud: a PLY with a ``semantics`` column, or an .npz with ``points`` (N,3) and ``labels`` (N)
  matrix    a .npy holding the 4 x 4 source -> scan transform
  --boxes   an .npz with ``labels`` (K), ``min`` (K,3), ``max`` (K,3): the box table, rows in the file's order
  --mesh    an .npz with ``vertices`` (V,3) and ``labels`` (V): the boxes are the per-label AABBs of the vertices
            (neither: the per-label AABBs of the source cloud itself)
  --no-bbox plain nearest-neighbour transfer; labels farther than --max-distance from their source point become -1

Usage: segment_gs.py scan.ply source.{ply,npz} matrix.npy [--boxes B.npz | --mesh M.npz | --no-bbox] [--threshold 0.1]
                     [--max-distance D] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_labelled_cloud(path):
    """-> (points float32 (N,3), labels int64 (N))."""
    if path.endswith(".npz"):
        z = np.load(path)
        return np.asarray(z["points"], np.float32).reshape(-1, 3), np.asarray(z["labels"]).reshape(-1).astype(np.int64)
    from gsworld_amd.ply import read_ply

    cols = read_ply(path)
    if "semantics" not in cols:
        raise ValueError(f"{path}: no `semantics` column")
    return np.stack((cols["x"], cols["y"], cols["z"]), 1).astype(np.float32), np.rint(cols["semantics"]).astype(np.int64)


def read_boxes(path):
    """-> {label: (min (3,), max (3,))} in the file's row order."""
    z = np.load(path)
    return {int(k): (np.asarray(lo, np.float64), np.asarray(hi, np.float64)) for k, lo, hi in zip(z["labels"], z["min"], z["max"])}


def output_path(scan, out):
    return out if out else os.path.splitext(scan)[0] + "_semantics_gs.npy"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scan")
    ap.add_argument("source")
    ap.add_argument("matrix")
    ap.add_argument("--boxes")
    ap.add_argument("--mesh")
    ap.add_argument("--no-bbox", action="store_true")
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--max-distance", type=float, default=None)
    ap.add_argument("--out")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()

    import torch

    from gsworld_amd import real2sim
    from gsworld_amd.ply import read_ply

    dev = torch.device(args.device)
    cols = read_ply(args.scan)
    scan = torch.from_numpy(np.stack((cols["x"], cols["y"], cols["z"]), 1).astype(np.float32)).to(dev)
    pts, lab = read_labelled_cloud(args.source)
    src, src_lab = torch.from_numpy(pts).to(dev), torch.from_numpy(lab).to(dev)
    T = np.asarray(np.load(args.matrix), np.float64).reshape(4, 4)
    if args.no_bbox:
        labels, dist = real2sim.transfer_labels(src, src_lab, scan, T)
    else:
        if args.boxes:
            boxes = read_boxes(args.boxes)
        elif args.mesh:
            z = np.load(args.mesh)
            boxes = real2sim.semantic_bounding_boxes(torch.from_numpy(np.asarray(z["vertices"], np.float32)).to(dev),
                                                     torch.from_numpy(np.asarray(z["labels"]).astype(np.int64)).to(dev))
        else:
            keep = src_lab >= 0
            boxes = real2sim.semantic_bounding_boxes(src[keep], src_lab[keep])
        labels, dist = real2sim.transfer_labels_with_bbox(src, src_lab, scan, T, boxes, args.threshold)
    if args.max_distance is not None:
        labels = torch.where(real2sim.validate_labels(dist, args.max_distance), labels, torch.full_like(labels, -1))
    out = output_path(args.scan, args.out)
    np.save(out, labels.cpu().numpy().astype(np.int64))
    counts = torch.bincount(labels.to(torch.int64) + 1)
    print(f"{out}: {labels.numel()} Gaussians, {int(counts[0])} unlabelled, "
          + ", ".join(f"{k - 1}: {int(c)}" for k, c in enumerate(counts.tolist()) if k and c))


if __name__ == "__main__":
    main()
