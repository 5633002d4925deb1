#!/usr/bin/env python3
"""Random proposal-recall cases (datasets/imdb.py:125-213, evaluate_recall): the one-call device table
(wssdl_proposal_recall) against the package's host path, bit for bit -- the match table (gt, box, overlap) row for
row, hits, num_pos, recalls and ar of every (area, limit) cell.  Random image counts (1 ... 40), 0 ... 24 gts per image
on a coarse uint16 grid (twin boxes included), 0 ... 700 candidates on quarter pixels (so ties are frequent), random
subsets of the eight area ranges, limits at, below and above the counts; every other case goes through the f32 +
scale form, whose host side is f32(box) / f32(scale).  Cases in which an image has fewer usable boxes than valid gts
must raise AssertionError on both sides.
    python3 tools/recall_fuzz.py [--cases 60] [--seed 0]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wssdl_bus_amd.datasets import recall  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
rs = np.random.RandomState(args.seed)
SIZES = (6, 10, 20, 33, 40, 97, 100, 130, 260, 520)


def random_case():
    n_images = int(rs.randint(1, 41))
    max_boxes = int(rs.choice([5, 24, 63, 64, 65, 300, 700]))
    gts, cands = [], []
    for _ in range(n_images):
        G = int(rs.choice([0, 1, 2, 3, 24])) if rs.rand() < 0.8 else int(rs.randint(0, 25))
        g = np.zeros((G, 4), np.float64)
        for k in range(G):
            w, h = rs.choice(SIZES, 2)
            x, y = rs.randint(0, 16, 2) * 8
            g[k] = [x, y, x + w - 1, y + h - 1]
            if k and rs.rand() < 0.2:
                g[k] = g[k - 1]
        # mostly at least as many boxes as gts: fewer is the reference's assertion, wanted in a minority of cases
        n = 0 if rs.rand() < 0.1 else int(rs.randint(1 if rs.rand() < 0.03 else min(max(G, 1), max_boxes), max_boxes + 1))
        b = np.zeros((n, 4), np.float64)
        for p in range(n):
            if G and rs.rand() < 0.7:
                src = g[rs.randint(G)]
                b[p] = src + (rs.randint(-8, 9, 4) / 4.0 if rs.rand() < 0.5 else np.array([0, 0, 0, src[3] - src[1] + 1]) * rs.randint(0, 2))
            else:
                x, y = rs.randint(0, 256, 2)
                b[p] = [x, y, x + rs.randint(4, 200), y + rs.randint(4, 200)]
            b[p, 2:] = np.maximum(b[p, 2:], b[p, :2])
        gts.append(g)
        cands.append(np.maximum(b, 0.0))
    areas_of = [((g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)).astype(np.float32) for g in gts]
    gt = dict(boxes=np.concatenate(gts, 0), areas=np.concatenate(areas_of, 0).astype(np.float64),
              offsets=np.cumsum([0] + [len(g) for g in gts]).astype(np.int32))
    areas = tuple(a for a in recall.ALL_EIGHT if rs.rand() < 0.5) or ("all",)
    most = max(len(g) for g in gts)
    pool = [1, 3, 24, 64, 300, 1000] if rs.rand() < 0.1 else [v for v in (1, 3, 24, 64, 300, 1000) if v >= most]
    limits = tuple(dict.fromkeys([None] + [int(v) for v in rs.choice(pool, int(rs.randint(0, 4)))]))
    return gt, cands, areas, limits


def tables_equal(a, b):
    if list(a) != list(b):
        return False
    for k in a:
        if a[k]["num_pos"] != b[k]["num_pos"] or not np.array_equal(a[k]["hits"], b[k]["hits"]):
            return False
        for what in ("recalls", "gt_overlaps"):
            if not np.array_equal(a[k][what], b[k][what], equal_nan=True):
                return False
        if not np.array_equal(np.float64(a[k]["ar"]), np.float64(b[k]["ar"]), equal_nan=True):
            return False
        for col in ("image", "gt", "box", "overlap"):
            if not np.array_equal(a[k]["matches"][col], b[k]["matches"][col]):
                return False
    return True


bad = raised = 0
for k in range(args.cases):
    gt, cands, areas, limits = random_case()
    if k % 2:
        N, P = len(cands), max(1, max(len(c) for c in cands))
        scales = rs.uniform(0.4, 2.7, N).astype(np.float32)
        rois = np.zeros((N, P, 5), np.float32)
        for i, c in enumerate(cands):
            rois[i, :len(c), 1:] = (c * np.float64(scales[i])).astype(np.float32)
            cands[i] = (rois[i, :len(c), 1:] / scales[i]).astype(np.float64)
        device_in = (torch.from_numpy(rois).cuda(), torch.tensor([len(c) for c in cands], dtype=torch.int32).cuda(),
                     torch.from_numpy(scales).cuda())
    else:
        device_in = cands
    want = got = None
    with np.errstate(all="ignore"):
        try:
            want = recall.evaluate_recall_host(cands, gt, areas, limits, return_matches=True)
        except AssertionError:
            pass
        try:
            got = recall.evaluate_recall_table(device_in, gt, areas, limits, return_matches=True)
        except AssertionError:
            pass
    raised += want is None
    ok = (want is None) == (got is None) and (want is None or tables_equal(got, want))
    if not ok:
        bad += 1
        print("MISMATCH case %d images %d gts %d areas %s limits %s form %s" %
              (k, len(cands), len(gt["boxes"]), areas, limits, "f32+scale" if k % 2 else "f64"), flush=True)
    if (k + 1) % 20 == 0:
        print("case %d ok so far (%d mismatches)" % (k + 1, bad), flush=True)
print("cases %d mismatches %d (%d cases raised the reference's assertion on both sides)" % (args.cases, bad, raised))
sys.exit(1 if bad else 0)
