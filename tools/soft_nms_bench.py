#!/usr/bin/env python3
"""Soft-NMS at test time (cfg.TEST.SOFT_NMS): the device time of wssdl_post_detections_soft at the working size of
tools/tta_bench.py -- 8 images x 2 views x 300 rows, K = 3, max_per_image = 300, the same seeded rows, view 1 of every
image mirrored -- against the hard views op on the same rows and the package's host path of the same statement.

    python tools/soft_nms_bench.py [--rounds 15] [--iters 100] [--host-iters 1] [--out FILE]

Alternating in every round on the same tensors (measuring-on-mi355x, section 5: warm every shape, alternate the variants
in one process, report the spread):
  (a) the soft op, linear and Gaussian        wssdl_post_detections_soft, 16 segments of pitch 600
  (b) the hard op                             wssdl_post_detections_views, agnostic off, voting off
  (c) the host path, linear and Gaussian      postprocess_detections_batch(views=2) under cfg.TEST.SOFT_NMS with
                                              FUSED_POST_DETECTIONS off: un-mirror, NumPy pick loop per image and class
(a) and (b) are device events around `iters` back-to-back calls (no read-back in them; launch gaps included); (c) is a
host clock around `host-iters` calls.  Medians over the rounds with (min, max).  Before anything is timed (a) is compared
with (c) bit for bit, both methods.  The pick loop is serial per segment and the segments run side by side, so the time per
pick is derived from the longest segment: the soft op's median / the picks of the longest segment (counted with the cap
off).  The other two launches are in that time: an upper bound of the cost of one turn."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import tta_bench as TB  # noqa: E402

N, V, ROWS, K, CAP = TB.N, TB.V, TB.ROWS, TB.K, TB.CAP
METHODS = ("linear", "gaussian")


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def run(args):
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_views_device, postprocess_detections_batch
    from wssdl_bus_amd.fast_rcnn.soft_nms import post_detections_soft_device
    scores, boxes, rois, fw = TB.tta_rows()
    P = V * ROWS

    def soft(method, cap=CAP):
        return post_detections_soft_device(scores, boxes, rois, N, V, fw, K, 0.05, cap, method=method, max_rows_per_image=P)

    def hard():
        return post_detections_views_device(scores, boxes, rois, N, V, fw, K, 0.05, CAP, max_rows_per_image=P, agnostic=False,
                                            vote_thresh=0.0)

    def host(method):
        old = cfg.TEST.FUSED_POST_DETECTIONS, cfg.TEST.SOFT_NMS
        cfg.TEST.FUSED_POST_DETECTIONS, cfg.TEST.SOFT_NMS = False, method
        try:
            return postprocess_detections_batch(scores, boxes, rois, N, K, 0.05, CAP, views=V, flip_width=fw)
        finally:
            cfg.TEST.FUSED_POST_DETECTIONS, cfg.TEST.SOFT_NMS = old

    out = {"tool": "soft_nms_bench", "images": N, "views": V, "rows_per_view": ROWS, "classes": K, "max_per_image": CAP,
           "nms_thresh": float(cfg.TEST.NMS), "sigma": float(cfg.TEST.SOFT_NMS_SIGMA),
           "min_score": float(cfg.TEST.SOFT_NMS_MIN_SCORE), "rounds": args.rounds, "iters": args.iters,
           "host_iters": args.host_iters}
    for m in METHODS:
        dets, counts = soft(m)
        n = counts.cpu().tolist()
        want = host(m)
        if not all(torch.equal(dets[i, j - 1, :n[i][j - 1]], want[i][j]) for i in range(N) for j in range(1, K)):
            raise SystemExit("the soft op (%s) and the host path disagree: nothing timed" % m)
        picks = soft(m, cap=0)[1].cpu().reshape(-1).tolist()         # no cap: every pick of every segment is counted
        out[m + "_picks_per_segment"] = {"mean": round(sum(picks) / len(picks), 1), "min": min(picks), "max": max(picks)}
        out[m + "_detections_after_cap"] = int(counts.sum())
    out["outputs_bit_equal_to_host_path"] = True
    out["hard_detections"] = int(hard()[1].sum())
    device = [("hard_views_op", hard)]
    for m in METHODS:
        device.append(("soft_" + m, lambda m=m: soft(m)))
    for _, fn in device:
        for _ in range(5):
            fn()
    times = {name: [] for name, _ in device}
    for m in METHODS:
        times["host_" + m] = []
    for _ in range(args.rounds):
        for name, fn in device:
            times[name].append(TB.events_ms(fn, args.iters))
        for m in METHODS:
            times["host_" + m].append(TB.clock_ms(lambda m=m: host(m), args.host_iters))
    for name, v in times.items():
        out[name + "_ms"] = stat(v)
    for m in METHODS:
        out["ratio_soft_%s_to_hard" % m] = stat([a / b for a, b in zip(times["soft_" + m], times["hard_views_op"])])
        out["ratio_host_%s_to_soft" % m] = stat([a / b for a, b in zip(times["host_" + m], times["soft_" + m])])
        out["us_per_pick_" + m] = round(1e3 * statistics.median(times["soft_" + m]) / out[m + "_picks_per_segment"]["max"], 4)
    names = TB.kernel_names(lambda: soft("gaussian"))
    out["kernels_of_one_call"] = sorted(s.split("(")[0].split("::")[-1] for s in names)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "soft_nms_bench needs a GPU"
    from wssdl_bus_amd import _lib
    _lib.lib()
    line = json.dumps(run(args))
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
