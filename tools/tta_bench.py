#!/usr/bin/env python3
"""Test-time augmentation (cfg.TEST.FLIP_AUG / BBOX_VOTE): the device time of wssdl_post_detections_views at the working
size -- 8 images x 2 views x 300 rows, K = 3, max_per_image = 300, seeded synthetic rows, view 1 of every image
mirrored -- against its yardstick, and the test-time throughput of detect_images with and without FLIP_AUG.

    python tools/tta_bench.py [--rounds 15] [--iters 200] [--host-iters 2] [--steps 5] [--warmup 2] [--no-detect]
                              [--out FILE]

Part 1, alternating in every round on the same tensors (measuring-on-mi355x, section 5: warm every shape, alternate the
variants in one process, report the spread):
  (a) the views op, voting off          wssdl_post_detections_views, 8 x 2 views, pitch 600
  (b) the views op, voting on           the same plus post_vote_kernel
  (c) the yardstick                     wssdl_post_detections_batched on the SAME rows as 16 images x 300: the
                                        parent's op ranking and sweeping the same 4800 rows in 32 segments of 300
                                        instead of 16 segments of 600
  (e) the same segmentation, old kernels wssdl_post_detections_batched on 8 images x 600 rows of a blob whose batch column
                                        and mirrored boxes were rewritten beforehand: (a) minus the un-mirror work
  (d) the host step-by-step route      postprocess_detections_batch(views=2) with FUSED_POST_DETECTIONS off and
                                        BBOX_VOTE on: per image and class a hip_nms with its read-back, then the vote
                                        on the host
(a)-(c) and (e) are device events around `iters` back-to-back calls (no read-back in them; launch gaps included); (d) is a host
clock around `host-iters` calls.  Medians over the rounds with (min, max).  Before anything is timed (b) is compared
with (d) bit for bit.  The kernels of one call of each are counted with torch.profiler in a window of their own.

Part 2: images/s of detect_images (tools/detect_bench.py's method: warm-up steps, then `steps` timed steps between two
synchronisations) on 8 planes of 600 x 1000 with ResNet-18, FLIP_AUG off and on.  The forward doubles under FLIP_AUG;
that is the feature's price.  What it buys in AP / FROC is not measured here: there is no data set in this tree.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("TORCH_BLAS_PREFER_HIPBLASLT", "1")
for _d in ("FWD", "BWD", "WRW"):
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + _d, "0")
os.environ.setdefault("TENSILE_STREAMK_DYNAMIC_GRID", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, V, ROWS, K, CAP, WIDTH = 8, 2, 300, 3, 300, 1000.0


def tta_rows(seed=7):
    """(scores [R,K], boxes [R,4K], rois [R,5], flip_width [N*V]) on the GPU, R = N * V * ROWS; the boxes of a row share
    a centre, the rows of a view cluster around 40 centres (NMS and voting both have work); view 1 reports mirrored
    coordinates"""
    rs = np.random.RandomState(seed)
    R = N * V * ROWS
    centres = rs.uniform(60, WIDTH - 60, size=(N, 40, 2)) * [1.0, 0.6]
    src = np.repeat(np.arange(N * V), ROWS)
    ctr = centres[src // V, rs.randint(0, 40, size=R)][:, None, :] + rs.normal(0, 8, size=(R, K, 2))
    wh = rs.uniform(30, 110, size=(R, K, 2))
    b = np.clip(np.concatenate((ctr - wh / 2, ctr + wh / 2), axis=2), 0, WIDTH - 1).astype(np.float32)
    mirrored = (src % V) == 1
    x1, x2 = b[mirrored, :, 0].copy(), b[mirrored, :, 2].copy()
    b[mirrored, :, 0] = np.float32(WIDTH) - x2 - np.float32(1)
    b[mirrored, :, 2] = np.float32(WIDTH) - x1 - np.float32(1)
    scores = rs.uniform(0, 1, size=(R, K)).astype(np.float32)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = src
    fw = np.where(np.arange(N * V) % V == 1, WIDTH, -1.0).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (scores, b.reshape(R, 4 * K), rois, fw))


def events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def clock_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    return [s for s in names if "memcpy" not in s.lower() and "memset" not in s.lower()]


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def run_op(args):
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import (post_detections_batched_device, post_detections_views_device,
                                                      postprocess_detections_batch, unmirror_boxes)
    scores, boxes, rois, fw = tta_rows()
    P = V * ROWS

    def views_op(vote):
        return post_detections_views_device(scores, boxes, rois, N, V, fw, K, 0.05, CAP, max_rows_per_image=P, agnostic=False,
                                            vote_thresh=0.5 if vote else 0.0)

    def yardstick():
        return post_detections_batched_device(scores, boxes, rois, N * V, K, 0.05, CAP, max_rows_per_image=ROWS, agnostic=False)

    # (e) the same segmentation without the new kernels: batch column = output image, mirrored rows un-mirrored beforehand
    ub, image = unmirror_boxes(boxes, rois, N, V, fw)
    urois = rois.clone()
    urois[:, 0] = image.to(torch.float32)

    def same_segments():
        return post_detections_batched_device(scores, ub, urois, N, K, 0.05, CAP, max_rows_per_image=P, agnostic=False)

    def host_route():
        old = cfg.TEST.FUSED_POST_DETECTIONS, cfg.TEST.BBOX_VOTE, cfg.TEST.BBOX_VOTE_THRESH, cfg.TEST.CLS_AGNOSTIC_NMS
        cfg.TEST.FUSED_POST_DETECTIONS, cfg.TEST.BBOX_VOTE, cfg.TEST.BBOX_VOTE_THRESH, cfg.TEST.CLS_AGNOSTIC_NMS = \
            False, True, 0.5, False
        try:
            return postprocess_detections_batch(scores, boxes, rois, N, K, 0.05, CAP, views=V, flip_width=fw)
        finally:
            (cfg.TEST.FUSED_POST_DETECTIONS, cfg.TEST.BBOX_VOTE, cfg.TEST.BBOX_VOTE_THRESH, cfg.TEST.CLS_AGNOSTIC_NMS) = old

    dets, counts = views_op(True)
    n = counts.cpu().tolist()
    want = host_route()
    same = all(torch.equal(dets[i, j - 1, :n[i][j - 1]], want[i][j]) for i in range(N) for j in range(1, K))
    if not same:
        raise SystemExit("the views op and the host step-by-step route disagree: nothing timed")
    plain, _ = views_op(False)
    moved = sum(int((dets[i, j - 1, :n[i][j - 1], :4] != plain[i, j - 1, :n[i][j - 1], :4]).any(1).sum())
                for i in range(N) for j in range(1, K))
    sd, sc = same_segments()
    if not (torch.equal(sc, counts) and all(torch.equal(sd[i, j - 1, :n[i][j - 1]], plain[i, j - 1, :n[i][j - 1]])
                                            for i in range(N) for j in range(1, K))):
        raise SystemExit("the views op (voting off) and the batched op on the rewritten blob disagree: nothing timed")
    device = (("views_op_vote_off", lambda: views_op(False)), ("views_op_vote_on", lambda: views_op(True)),
              ("batched_16x300", yardstick), ("batched_8x600_rewritten", same_segments))
    for _, fn in device:
        for _ in range(5):
            fn()
    times = {name: [] for name, _ in device}
    times["host_step_by_step"] = []
    for _ in range(args.rounds):
        for name, fn in device:
            times[name].append(events_ms(fn, args.iters))
        times["host_step_by_step"].append(clock_ms(host_route, args.host_iters))
    out = {"tool": "tta_bench", "row": "op", "images": N, "views": V, "rows_per_view": ROWS, "classes": K, "max_per_image": CAP,
           "rounds": args.rounds, "iters": args.iters, "host_iters": args.host_iters, "outputs_bit_equal": bool(same),
           "detections": int(counts.sum()), "detections_moved_by_voting": moved}
    for name, v in times.items():
        out[name + "_ms"] = stat(v)
    ratios = [a / c for a, c in zip(times["views_op_vote_off"], times["batched_16x300"])]
    out["ratio_vote_off_to_batched_16x300"] = stat(ratios)
    out["ratio_vote_off_to_batched_8x600_rewritten"] = stat([a / c for a, c in zip(times["views_op_vote_off"],
                                                                                   times["batched_8x600_rewritten"])])
    share = [(b - a) / b for a, b in zip(times["views_op_vote_off"], times["views_op_vote_on"])]
    out["vote_kernel_share_of_vote_on"] = stat(share)
    kernels = {}
    for name, fn in device:
        names = kernel_names(fn)
        kernels[name] = {"device_kernels": len(names), "new": sorted(set(s.split("(")[0].split("::")[-1] for s in names
                                                                      if "post_view" in s or "post_vote" in s))}
    names = kernel_names(host_route)
    kernels["host_step_by_step"] = {"device_kernels": len(names)}
    out["kernels"] = kernels
    # the bytes the new passes move: the un-mirror / key pass and the voting kernel
    R = N * V * ROWS
    out["bytes"] = {"view_keys_pass": R * 4 + R * (K - 1) * (4 + 16) + N * (K - 1) * P * (8 + 16 + 4),
                    "vote_kernel_per_detection": P * (4 + 4 + 16) + 20 + 16}
    return out


def run_detect(args, flip):
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import detect_images
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(3)
    net = get_network("Resnet_train_alter", 18).cuda().to(memory_format=torch.channels_last)
    net.eval()
    rs = np.random.RandomState(3)
    planes = [rs.randint(0, 256, size=(600, 1000)).astype(np.uint8) for _ in range(8)]
    old = cfg.TEST.FLIP_AUG
    cfg.TEST.FLIP_AUG = flip
    try:
        for _ in range(args.warmup):
            detect_images(net, planes, "Resnet", batch_size=8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            all_boxes = detect_images(net, planes, "Resnet", batch_size=8)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        cfg.TEST.FLIP_AUG = old
    del net
    torch.cuda.empty_cache()
    return {"tool": "tta_bench", "row": "detect_images", "net": "Resnet_train_alter-18", "image": [600, 1000], "batch_size": 8,
            "flip_aug": bool(flip), "steps": args.steps, "warmup": args.warmup,
            "images_per_s": round(8 * args.steps / elapsed, 3), "ms_per_batch": round(1e3 * elapsed / args.steps, 3),
            "detections": sum(len(all_boxes[j][i]) for j in range(1, len(all_boxes)) for i in range(8))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-detect", action="store_true", help="only part 1 (no network)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tta_bench needs a GPU"
    from wssdl_bus_amd import _lib
    _lib.lib()
    lines = [json.dumps(run_op(args))]
    print(lines[-1], flush=True)
    if not args.no_detect:
        for flip in (False, True, False, True):
            lines.append(json.dumps(run_detect(args, flip)))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
