#!/usr/bin/env python3
"""Time of wssdl_draw_detections (csrc/draw_detect.hip) on N planes with ground truth and detections, as HIP events see
the two kernels, against the bytes the op must move (sum(h * w) * 4: one read, three written).

    python tools/draw_bench.py [--images 8] [--height 600] [--width 1000] [--dets 10] [--reps 50]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--dets", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from wssdl_bus_amd.fast_rcnn import vis
    rs = np.random.RandomState(0)
    N, h, w, K, P = a.images, a.height, a.width, 3, 300
    classes = ['__background__', 'benign', 'malignant']
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    arena = t(rs.randint(0, 256, N * h * w).astype(np.uint8))
    items = vis._item_table([(h, w)] * N, [w] * N, [i * h * w for i in range(N)], [i * h * w * 3 for i in range(N)])
    xy = rs.rand(N, K - 1, P, 2) * [w * 0.6, h * 0.6]
    dets = np.concatenate([xy, xy + 40 + rs.rand(N, K - 1, P, 2) * [w * 0.3, h * 0.3], 0.5 + 0.5 * rs.rand(N, K - 1, P, 1)], 3).astype(np.float32)
    counts = np.full((N, K - 1), a.dets, np.int32)
    gb = np.tile(np.asarray([[w * 0.2, h * 0.2, w * 0.7, h * 0.8]], np.float32), (N, 1))
    args = (arena, items, t(gb), t(np.ones(N, np.int32)), np.arange(N + 1, dtype=np.int32), t(dets), t(counts), t(vis.colour_table(classes)),
            t(vis.glyph_table()), t(vis.label_table(classes)), vis.DrawStyle(), torch.empty(N * h * w * 3, dtype=torch.uint8, device="cuda"))
    for _ in range(5):
        vis.draw_raw(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        vis.draw_raw(*args)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    times = np.sort(times)
    moved = N * h * w * 4
    print("draw %d x %d x %d, %d + 1 items per image: median %.3f ms (min %.3f, max %.3f) over %d calls, %.1f MB must move, "
          "%.0f GB/s at the median (the call includes two small uploads and the workspace allocation)"
          % (N, h, w, (K - 1) * a.dets, np.median(times), times[0], times[-1], a.reps, moved / 1e6, moved / np.median(times) / 1e6))


if __name__ == "__main__":
    main()
