#!/usr/bin/env python3
"""Time of one proposal-recall table (datasets.recall.evaluate_recall_table -> wssdl_proposal_recall) at test size:
the 8 area ranges x 4 limits (None, 10, 100, 300) at 1000 images x 300 proposals x 1-3 gts, from the proposal
layer's device layout (rois [N, P, 5] f32, counts, scales), against the module's host path on the same inputs --
the reference's loop, one cell at a time.  The two are compared (bit for bit, match tables included) before anything
is timed, then timed ALTERNATING, `--rounds` times.  Prints one JSON line.

    python tools/recall_bench.py [--images 1000] [--per-image 300] [--rounds 5] [--iters 20] [--warmup 3] [--out FILE]
    python tools/recall_bench.py --kernels DIR    the per-kernel split: one `rocprofv3 --kernel-trace --stats` run of
                                                  this tool (a fresh child process, --op-only) writing under DIR

table_ms: time.perf_counter around `iters` back-to-back tables after a synchronise -- the op with its output
allocations, the upload of ground truth, ranges, limits and thresholds and the two read-backs (summary, overlaps);
each read-back synchronises, so this is the time a caller sees.  host_ms: time.perf_counter around one host table.
Kernel counts: what one table enqueues (counted from the op's code: 2 kernels, 3 memsets, 1 host-to-device copy,
whatever the number of cells) against the cells x images matrices the per-cell route computes."""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = (None, 10, 100, 300)


def make_inputs(n_images, per_image, seed=11):
    """rois [N, P, 5] f32 in network-input pixels (best first is not modelled: recall does not read scores), a
    third of them near a ground-truth box; 1-3 uint16 gts per image; scales as get_test_blobs would give."""
    rs = np.random.RandomState(seed)
    P = per_image
    rois = np.zeros((n_images, P, 5), np.float32)
    scales = rs.uniform(0.9, 1.6, n_images).astype(np.float32)
    roidb = []
    for i in range(n_images):
        n = rs.randint(1, 4)
        x, y = rs.randint(0, 500, n), rs.randint(0, 350, n)
        g = np.stack((x, y, x + rs.randint(20, 400, n), y + rs.randint(20, 400, n)), 1).astype(np.uint16)
        ov = np.zeros((n, 3), np.float32)
        ov[:, 1] = 1.0
        gf = g.astype(np.float64)
        roidb.append(dict(boxes=g, gt_classes=np.ones((n,), np.int32), gt_overlaps=ov,
                          seg_areas=((gf[:, 2] - gf[:, 0] + 1) * (gf[:, 3] - gf[:, 1] + 1)).astype(np.float32)))
        bx, by = rs.uniform(0, 600, P), rs.uniform(0, 400, P)
        b = np.stack((bx, by, bx + rs.uniform(16, 400, P), by + rs.uniform(16, 400, P)), 1)
        near = rs.rand(P) < 0.33
        b[near] = gf[rs.randint(0, n, P)][near] + rs.normal(0, 10, (int(near.sum()), 4))
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2])
        rois[i, :, 0] = i
        rois[i, :, 1:] = (np.maximum(b, 0) * np.float64(scales[i])).astype(np.float32)
    counts = np.full((n_images,), P, np.int32)
    counts[::97] = 0                                       # a few images without proposals
    return rois, counts, scales, roidb


def same(a, b):
    if list(a) != list(b):
        return False
    for k in a:
        if a[k]["num_pos"] != b[k]["num_pos"] or not np.array_equal(a[k]["hits"], b[k]["hits"]):
            return False
        if not (np.array_equal(a[k]["recalls"], b[k]["recalls"], equal_nan=True) and np.array_equal(a[k]["gt_overlaps"], b[k]["gt_overlaps"])):
            return False
        if "matches" in a[k] and not all(np.array_equal(a[k]["matches"][c], b[k]["matches"][c]) for c in ("image", "gt", "box", "overlap")):
            return False
    return True


def kernels(args):
    out = os.path.abspath(args.kernels)
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "recall_bench", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--op-only", "--images", str(args.images), "--per-image", str(args.per_image),
           "--iters", "10", "--warmup", "2"]
    subprocess.check_call(cmd, timeout=300)
    for f in sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)):
        print("# " + os.path.relpath(f, out))
        with open(f) as fh:
            for line in fh:
                if "recall_" in line or line.startswith('"Name"'):
                    print(line.rstrip())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--per-image", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--op-only", action="store_true", help="only run the device tables (the child of --kernels)")
    ap.add_argument("--kernels", default=None, help="directory for one rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    if args.kernels:
        return kernels(args)
    assert torch.cuda.is_available(), "recall_bench needs a GPU"
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.datasets import recall
    _lib.lib()
    rois, counts, scales, roidb = make_inputs(args.images, args.per_image)
    gt = recall.pack_recall_gt(roidb)
    triple = (torch.from_numpy(rois).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(scales).cuda())
    lists = [(rois[i, :counts[i], 1:] / scales[i]).astype(np.float64) for i in range(args.images)]     # im_proposals' arithmetic
    device = lambda m=False: recall.evaluate_recall_table(triple, gt, recall.ALL_EIGHT, LIMITS, return_matches=m)
    host = lambda m=False: recall.evaluate_recall_host(lists, gt, recall.ALL_EIGHT, LIMITS, return_matches=m)
    np.seterr(all="ignore")
    for _ in range(args.warmup):
        r = device()
    if args.op_only:
        for _ in range(args.iters):
            device()
        torch.cuda.synchronize()
        return
    same_as_host = same(device(True), host(True))
    table_ms, host_ms = [], []
    for _ in range(args.rounds):                           # alternating: the machine's other work hits both alike
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            r = device()
        torch.cuda.synchronize()
        table_ms.append(1e3 * (time.perf_counter() - t0) / args.iters)
        t0 = time.perf_counter()
        host()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    cells = len(recall.ALL_EIGHT) * len(LIMITS)
    line = {"tool": "recall_bench", "images": args.images, "per_image": args.per_image, "gt_boxes": int(len(gt["boxes"])),
            "areas": len(recall.ALL_EIGHT), "limits": [0 if l is None else l for l in LIMITS], "cells": cells, "rounds": args.rounds,
            "iters": args.iters, "warmup": args.warmup, "same_as_host": same_as_host,
            "table_ms": [round(v, 3) for v in table_ms], "host_ms": [round(v, 1) for v in host_ms],
            "table_ms_median": round(float(np.median(table_ms)), 3), "host_ms_median": round(float(np.median(host_ms)), 1),
            "host_over_table": round(float(np.median(host_ms) / np.median(table_ms)), 1),
            "device_launches_per_table": {"kernels": 2, "memsets": 3, "h2d_copies": 1, "iou_matrices": int((counts > 0).sum())},
            "per_cell_route_iou_matrices": cells * int((counts > 0).sum()),
            "ar_all": float(r[("all", None)]["ar"]), "recall_at_0.5_all_by_limit": [float(r[("all", l)]["recalls"][0]) for l in LIMITS]}
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(out + "\n")
    if not same_as_host:
        sys.exit(1)


if __name__ == "__main__":
    main()
