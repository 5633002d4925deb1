#!/usr/bin/env python3
"""Test-time throughput of the batched detection path (im_detect_batch + postprocess_detections_batch) at
batch sizes 1, 4 and 8, on the shapes of two bench.py workloads, and the device time of the post-detection
op per image: one wssdl_post_detections_batched call for the batch against N wssdl_post_detections calls on
the same rows.  One process; prints one JSON line per (workload, batch size).

    python tools/detect_bench.py [--workloads resnet101_1600_test,resnet18_sup_b2] [--batches 1,4,8]
                                 [--steps 10] [--warmup 3] [--iters 20] [--out FILE]

Images/s: warm-up steps, then `steps` timed steps between two torch.cuda.synchronize() calls.  Post-detection
times: HIP events around `iters` back-to-back calls (launch gaps included), divided by iters * N.
MIOpen picks its convolution solvers by heuristic here (no find); bench.py's numbers use a find-db.

    python tools/detect_bench.py --post-agnostic [--rounds 15] [--iters 20] [--out FILE]

The class-agnostic row (cfg.TEST.CLS_AGNOSTIC_NMS) at the reference's test shape -- 8 images x 300 rows, K = 3,
max_per_image = 300, seeded synthetic rows whose class boxes share a centre -- without a network: in every round, one
after the other on the same tensors, (a) the agnostic device op, (b) the per-class device op, both with the read-back
of the counts the path needs, and (c) the step-by-step per-image loop (FUSED_POST_DETECTIONS = False, flag on).  Each
is a host clock around `iters` calls that end in a device synchronise; the row reports the median over the rounds and
the spread (min, max).  The outputs of (a) and (c) are compared bit for bit before anything is timed.
"""
import argparse
import json
import os
import sys
import time

# the same process settings as bench.py (must precede the torch import): hipBLASLt for the per-RoI head, no naive
# reference convolutions timed in the first step, a fixed stream-K grid
os.environ.setdefault("TORCH_BLAS_PREFER_HIPBLASLT", "1")
for _d in ("FWD", "BWD", "WRW"):
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + _d, "0")
os.environ.setdefault("TENSILE_STREAMK_DYNAMIC_GRID", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# test-time shapes of two bench.py workloads (bench.py WORKLOADS), copied
WORKLOADS = {
    "resnet101_1600_test": dict(net="Resnet_train", depth=101, im=(1000, 1600)),
    "resnet18_sup_b2": dict(net="Resnet_train_alter", depth=18, im=(600, 1000)),
}


def events_ms(fn, iters):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def run(name, wl, bs, args):
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn.detect_batch import (im_detect_batch, post_detections_batched_device,
                                                      postprocess_detections_batch)
    from wssdl_bus_amd.fast_rcnn.post_detections import post_detections_device
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(3)
    net = get_network(wl["net"], wl["depth"]).cuda().to(memory_format=torch.channels_last)
    net.eval()
    im_h, im_w = wl["im"]
    blobs = synthetic.make_batch(bs, 0, im_h, im_w, seed=3)
    data, info = blobs["data"], blobs["im_info"]

    def step():
        scores, boxes, rois = im_detect_batch(net, data, info)
        return postprocess_detections_batch(scores, boxes, rois, bs, scores.shape[1], thresh=0.05, max_per_image=300)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    n_det = sum(int(d[j].shape[0]) for d in out for j in d)

    # the post-detection op alone, on this batch's network outputs
    scores, boxes, rois = im_detect_batch(net, data, info)
    K = int(scores.shape[1])
    rows = [torch.nonzero(rois[:, 0] == i).reshape(-1) for i in range(bs)]
    per_image = [(scores[r].contiguous(), boxes[r].contiguous()) for r in rows]
    batched = events_ms(lambda: post_detections_batched_device(scores, boxes, rois, bs, K), args.iters)
    single = events_ms(lambda: [post_detections_device(s, b, K) for s, b in per_image], args.iters)
    del net
    torch.cuda.empty_cache()
    return {
        "tool": "detect_bench", "workload": name, "net": "%s-%d" % (wl["net"], wl["depth"]), "image": list(wl["im"]),
        "batch_size": bs, "steps": args.steps, "warmup": args.warmup,
        "images_per_s": round(bs * args.steps / elapsed, 3), "ms_per_batch": round(1e3 * elapsed / args.steps, 3),
        "rois": int(rois.shape[0]), "classes": K, "detections": n_det,
        "post_detect_batched_ms_per_image": round(batched / bs, 4),
        "post_detect_single_ms_per_image": round(single / bs, 4),
        "post_detect_iters": args.iters,
    }


def post_agnostic_rows(n_images=8, rows=300, K=3, seed=7):
    """(scores [R,K], boxes [R,4K], rois [R,5]) on the GPU: the class boxes of one row share a centre"""
    import numpy as np
    rs = np.random.RandomState(seed)
    R = n_images * rows
    ctr = rs.uniform(50, 900, size=(R, 1, 2)) * [1.0, 0.6] + rs.normal(0, 6, size=(R, K, 2))
    wh = rs.uniform(30, 220, size=(R, K, 2))
    boxes = np.concatenate((ctr - wh / 2, ctr + wh / 2), axis=2).reshape(R, 4 * K).astype(np.float32)
    scores = rs.uniform(0, 1, size=(R, K)).astype(np.float32)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(n_images), rows)
    return tuple(torch.from_numpy(a).cuda() for a in (scores, boxes, rois))


def run_post_agnostic(args):
    import statistics
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device, postprocess_detections_batch
    N, rows, K, cap = 8, 300, 3, 300
    scores, boxes, rois = post_agnostic_rows(N, rows, K)

    def device_op(agnostic):
        dets, counts = post_detections_batched_device(scores, boxes, rois, N, K, 0.05, cap, max_rows_per_image=rows,
                                                      agnostic=agnostic)
        return dets, counts.cpu()

    def loop():
        old = cfg.TEST.FUSED_POST_DETECTIONS
        cfg.TEST.FUSED_POST_DETECTIONS = False
        try:
            return postprocess_detections_batch(scores, boxes, rois, N, K, 0.05, cap)
        finally:
            cfg.TEST.FUSED_POST_DETECTIONS = old

    def clock_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.iters

    old_flag = cfg.TEST.CLS_AGNOSTIC_NMS
    cfg.TEST.CLS_AGNOSTIC_NMS = True
    try:
        dets, counts = device_op(True)
        want = loop()
        n = counts.tolist()
        same = all(torch.equal(dets[i, j - 1, :n[i][j - 1]], want[i][j]) for i in range(N) for j in range(1, K))
        if not same:
            raise SystemExit("the agnostic device op and the step-by-step loop disagree: nothing timed")
        _, per_class_counts = device_op(False)
        variants = (("agnostic_op", lambda: device_op(True)), ("per_class_op", lambda: device_op(False)),
                    ("step_by_step_loop", loop))
        for _, fn in variants:                          # warm-up of every shape the timed window uses
            for _ in range(3):
                fn()
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(clock_ms(fn))
    finally:
        cfg.TEST.CLS_AGNOSTIC_NMS = old_flag
    out = {"tool": "detect_bench", "row": "post_agnostic", "images": N, "rows_per_image": rows, "classes": K,
           "max_per_image": cap, "rounds": args.rounds, "iters": args.iters, "outputs_bit_equal": bool(same),
           "detections_agnostic": int(counts.sum()), "detections_per_class": int(per_class_counts.sum())}
    for name, v in times.items():
        out[name + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--post-agnostic", action="store_true",
                    help="only the class-agnostic post-detection row (no network): device ops against the per-image loop")
    ap.add_argument("--rounds", type=int, default=15, help="alternating rounds of the --post-agnostic row")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "detect_bench needs a GPU"
    from wssdl_bus_amd import _lib
    _lib.lib()
    lines = []
    if args.post_agnostic:
        lines.append(json.dumps(run_post_agnostic(args)))
        print(lines[0], flush=True)
    for name in ([] if args.post_agnostic else args.workloads.split(",")):
        for bs in (int(b) for b in args.batches.split(",")):
            line = json.dumps(run(name, WORKLOADS[name], bs, args))
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
