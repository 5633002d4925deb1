#!/usr/bin/env python3
"""Time of one detection evaluation (DetectionAccumulator.evaluate -> wssdl_eval_detections) at validation size:
1000 images x 300 detections x 2 classes x 21 FROC thresholds (+ the CorLoc threshold), against the module's host
path on the same inputs -- there is no earlier device version to compare with.  Prints one JSON line.

    python tools/eval_bench.py [--images 1000] [--per-image 300] [--iters 50] [--warmup 5] [--no-host] [--out FILE]
    python tools/eval_bench.py --kernels DIR      the per-kernel split: one `rocprofv3 --kernel-trace --stats` run of
                                                  this tool (a fresh child process, --op-only) writing under DIR

op_ms: HIP events around `iters` back-to-back evaluations after `warmup` ones -- the op with its output allocations,
the upload of ground truth and thresholds and the one read-back of the summary (the read-back synchronises, so this
is the time a validation loop sees).  host_ms: time.perf_counter around the host path, best of 2.  The two results
are compared before anything is timed."""
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
K = 3


def make_inputs(n_images, per_image, seed=7):
    """dets [N, K-1, P, 5] / counts as post_detections_batched_device leaves them (best first, 3-decimal ties
    everywhere), a third of the detections near a ground-truth box; 1-4 boxes per image."""
    rs = np.random.RandomState(seed)
    gt_roidb, P = [], per_image
    dets = np.zeros((n_images, K - 1, P, 5), np.float32)
    for i in range(n_images):
        n = rs.randint(1, 5)
        x, y = rs.randint(1, 600, n), rs.randint(1, 400, n)
        boxes = np.stack((x, y, x + rs.randint(40, 300, n), y + rs.randint(40, 300, n)), 1)
        gt_roidb.append(dict(boxes=boxes, gt_classes=rs.randint(1, K, n), difficult=(rs.rand(n) < 0.1).astype(np.uint8)))
        for j in range(K - 1):
            bx, by = rs.uniform(0, 600, P), rs.uniform(0, 400, P)
            b = np.stack((bx, by, bx + rs.uniform(30, 300, P), by + rs.uniform(30, 300, P)), 1)
            near = rs.rand(P) < 0.33
            src = boxes[rs.randint(0, n, P)] - 1.0
            b[near] = src[near] + rs.normal(0, 12, (int(near.sum()), 4))
            dets[i, j, :, :4] = b
            dets[i, j, :, 4] = np.sort(rs.beta(0.5, 2.0, P))[::-1]
    counts = np.full((n_images, K - 1), P, np.int32)
    return dets, counts, gt_roidb


def same(a, b):
    to_np = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    for k in ("class_offsets", "npos", "ni", "nok", "num_all_fps", "arr_ok", "num_fp_per_img", "order", "tp", "fp", "rec", "prec", "ap07"):
        if not np.array_equal(to_np(a[k]), to_np(b[k]), equal_nan=True):
            return False
    return bool(np.allclose(a["ap_area"], b["ap_area"], rtol=0, atol=1e-10))


def kernels(args):
    out = os.path.abspath(args.kernels)
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "eval_bench", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--op-only", "--images", str(args.images), "--per-image", str(args.per_image),
           "--iters", "10", "--warmup", "2"]
    subprocess.check_call(cmd, timeout=300)
    for f in sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)):
        print("# " + os.path.relpath(f, out))
        with open(f) as fh:
            for line in fh:
                if "eval_" in line or line.startswith('"Name"'):
                    print(line.rstrip())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--per-image", type=int, default=300)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host path")
    ap.add_argument("--op-only", action="store_true", help="only run the evaluations (the child of --kernels)")
    ap.add_argument("--kernels", default=None, help="directory for one rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    if args.kernels:
        return kernels(args)
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.datasets import FROC_THRESHOLDS, DetectionAccumulator, eval_detections, pack_gt
    _lib.lib()
    dets, counts, gt_roidb = make_inputs(args.images, args.per_image)
    gt = pack_gt(gt_roidb)
    thr = [0.5] + list(FROC_THRESHOLDS)
    acc = DetectionAccumulator(K)
    step = 8
    d_dev, c_dev = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    for b0 in range(0, args.images, step):
        acc.add(d_dev[b0:b0 + step], c_dev[b0:b0 + step], b0)
    whole = acc.gathered(args.images)                    # the gather of the batches is timed apart
    run = lambda: eval_detections((whole[0], whole[1], 0), gt, K, score_thresh=thr)
    for _ in range(args.warmup):
        r = run()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.iters):
        r = run()
    e.record()
    torch.cuda.synchronize()
    op_ms = s.elapsed_time(e) / args.iters
    if args.op_only:
        return
    s.record()
    for _ in range(args.iters):
        acc.gathered(args.images)
    e.record()
    torch.cuda.synchronize()
    gather_ms = s.elapsed_time(e) / args.iters
    line = {"tool": "eval_bench", "images": args.images, "per_image": args.per_image, "classes": K, "thresholds": len(thr),
            "detections": int(counts.sum()), "gt_boxes": int(len(gt[1])), "iters": args.iters, "warmup": args.warmup,
            "op_ms": round(op_ms, 4), "gather_ms": round(gather_ms, 4),
            "ap07": [float(a) for a in r["ap07"]], "nok_at_0.5": [int(n) for n in r["nok"][:, 0]]}
    if not args.no_host:
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            h = eval_detections((dets, counts, 0), gt, K, score_thresh=thr)
            dt = 1e3 * (time.perf_counter() - t0)
            best = dt if best is None else min(best, dt)
        line["host_ms"] = round(best, 2)
        line["same_as_host"] = same(r, h)
        line["host_over_op"] = round(best / op_ms, 1)
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
