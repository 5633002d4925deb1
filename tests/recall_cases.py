"""The cases of the proposal-recall tests, shared by tests/test_recall_cpu.py, tests/test_gpu_recall.py and
tests/golden/make_golden_recall.py (which runs the reference on them).  NumPy only: building a case needs neither the
package nor a GPU.

A case is dict(gt_boxes [k,4] uint16 per image, candidates [n,4] f64 per image, areas, limits, raises): the smallest
shapes at which the greedy matching can go wrong.

  tie_box        one gt, two boxes of identical IoU: box 0 wins.  The IoU is 0.5 = thresholds[0] exactly (`>=`).
  tie_gt         two gts with equal column maxima: gt 0 is matched first.
  shared_best    one box is the best of two gts: the second gt falls to its next-best box (where the greedy matching
                 differs from a plain column maximum).
  zero_overlap   a gt that overlaps nothing: overlap 0, the first unused box.
  mixed          an image without boxes (counts in num_pos only), an image without gt, an image without a valid gt in
                 'small', and an image of 5 boxes under limits below, at and above its count.
  sizes          P in {1, 63, 64, 65, 255, 257, 300, 2000} x G in {1, 2, 20}, every pair with P >= G, one image each.
  random200      200 seeded images: uint16 ground truth on a coarse grid, boxes on quarter pixels, so ties are
                 frequent; tie_census() counts them and the CPU test asserts that every tie class occurs.
  too_few        1 box and 2 gts: the reference's assert(gt_ovr >= 0) fires (raises=True).
"""
import numpy as np

ALL_EIGHT = ('all', 'small', 'medium', 'large', '96-128', '128-256', '256-512', '512-inf')
SIZES_P = (1, 63, 64, 65, 255, 257, 300, 2000)
SIZES_G = (1, 2, 20)


def seg_areas(gt_boxes):
    """The roidb's seg_areas of integer boxes: (x2 - x1 + 1) * (y2 - y1 + 1) as f32."""
    b = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    return ((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)).astype(np.float32)


def _case(gt, cand, areas=('all',), limits=(None,), raises=False):
    return dict(gt_boxes=[np.asarray(g, np.uint16).reshape(-1, 4) for g in gt],
                candidates=[np.asarray(c, np.float64).reshape(-1, 4) for c in cand],
                areas=tuple(areas), limits=tuple(limits), raises=raises)


def _boxes_near(rs, gts, n, canvas):
    """n candidate boxes on quarter pixels: jittered or stretched copies of the gts and free boxes."""
    out = np.zeros((n, 4), np.float64)
    for p in range(n):
        kind = rs.randint(0, 4)
        if len(gts) and kind < 3:
            g = np.asarray(gts[rs.randint(len(gts))], np.float64)
            if kind == 0:                                     # the gt itself, moved by quarter pixels
                b = g + rs.randint(-8, 9, 4) / 4.0
            elif kind == 1:                                   # same corner, twice the height or width: IoU 0.5 exactly
                b = g.copy()
                if rs.randint(2):
                    b[3] = g[3] + (g[3] - g[1] + 1)
                else:
                    b[2] = g[2] + (g[2] - g[0] + 1)
            else:                                             # a coarse shift: equal IoUs between neighbours
                b = g + np.repeat(rs.randint(-2, 3, 2), 2)[[0, 2, 1, 3]] * 4.0
        else:
            x, y = rs.randint(0, canvas, 2)
            b = np.array([x, y, x + rs.randint(4, canvas // 2), y + rs.randint(4, canvas // 2)], np.float64)
        b[2], b[3] = max(b[2], b[0]), max(b[3], b[1])
        out[p] = np.maximum(b, 0.0)
    return out


def _random_gts(rs, n, canvas, sizes):
    g = np.zeros((n, 4), np.uint16)
    for k in range(n):
        w, h = sizes[rs.randint(len(sizes))], sizes[rs.randint(len(sizes))]
        x, y = rs.randint(0, canvas // 8, 2) * 8
        g[k] = [x, y, x + w - 1, y + h - 1]
    return g


def _sizes_case():
    rs = np.random.RandomState(31)
    gt, cand = [], []
    for G in SIZES_G:
        for P in SIZES_P:
            if P < G:
                continue                                      # (fewer boxes than gts is the case `too_few`)
            g = _random_gts(rs, G, 256, (16, 40, 100, 200, 300, 520))
            gt.append(g)
            cand.append(_boxes_near(rs, g, P, 512))
    return _case(gt, cand, areas=ALL_EIGHT, limits=(None, 64, 300))


def _random200_case():
    rs = np.random.RandomState(32)
    gt, cand = [], []
    for i in range(200):
        G = rs.randint(0, 4)
        g = _random_gts(rs, G, 64, (10, 20, 40, 100, 130, 260))
        if G >= 2 and rs.rand() < 0.3:
            g[1] = g[0]                                       # twin gts: equal columns
            g[1, 3] = g[0, 3] + (2 if rs.rand() < 0.5 else 0)
        n = 0 if rs.rand() < 0.1 else rs.randint(3, 40)
        gt.append(g)
        cand.append(_boxes_near(rs, g, n, 128))
    return _case(gt, cand, areas=ALL_EIGHT, limits=(None, 3, 10, 100))


def build_cases():
    c = {}
    c['tie_box'] = _case([[[0, 0, 9, 9]]], [[[0, 0, 9, 19], [0, 0, 19, 9]]])
    c['tie_gt'] = _case([[[0, 0, 9, 9], [100, 100, 109, 109]]], [[[100, 100, 109, 119], [0, 0, 9, 19]]])
    c['shared_best'] = _case([[[0, 0, 9, 9], [0, 0, 9, 11]]], [[[0, 0, 9, 10], [0, 0, 9, 14]]])
    c['zero_overlap'] = _case([[[500, 500, 520, 520], [0, 0, 9, 9]]], [[[0, 0, 9, 9], [20, 20, 30, 30], [40, 40, 50, 50]]])
    c['mixed'] = _case(
        [[[0, 0, 9, 9], [0, 0, 99, 99]],                      # no boxes: num_pos only
         [],                                                  # no gt
         [[10, 10, 209, 209]],                                # no valid gt in 'small'
         [[0, 0, 19, 19], [40, 40, 59, 59], [5, 5, 24, 24]]],  # 5 boxes under limits 3, 5, 8, None
        [[], [[0, 0, 9, 9], [3, 3, 30, 30]], [[12, 12, 200, 200], [0, 0, 50, 50]],
         [[41, 41, 58.5, 58.5], [0, 0, 19, 19], [5, 5, 24, 24], [4.25, 4.25, 25, 25], [0, 0, 60, 60]]],
        areas=('all', 'small', 'medium', 'large'), limits=(3, 5, 8, None))
    c['sizes'] = _sizes_case()
    c['random200'] = _random200_case()
    c['too_few'] = _case([[[0, 0, 9, 9], [20, 20, 29, 29]]], [[[0, 0, 9, 9]]], raises=True)
    return c


_CASES = None


def cases():
    """name -> case, built once and shared (treat as read-only)."""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def roidb_of(case):
    """The case's ground truth as roidb entries (class 1 boxes, one-hot dense gt_overlaps, f32 seg_areas)."""
    out = []
    for g in case['gt_boxes']:
        k = len(g)
        ov = np.zeros((k, 3), np.float32)
        ov[:, 1] = 1.0
        out.append(dict(boxes=g, gt_classes=np.ones((k,), np.int32), gt_overlaps=ov, seg_areas=seg_areas(g), flipped=False))
    return out


def tie_census(case, overlaps, area_ranges, area_index):
    """How often each tie class occurs in the case's matching, over all its cells.  `overlaps(boxes, gts)` is an f64
    IoU function [n, k]; area_ranges / area_index name the bounds.  Counts rounds with
      box_tie     two unused boxes at the chosen gt's column maximum (the lowest index wins),
      gt_tie      two unused gts at the round's best column maximum (the lowest index wins),
      shared_best the chosen gt's best box over ALL boxes was already taken by another gt,
      zero        a recorded overlap of 0,
      threshold   a recorded overlap of exactly 0.5."""
    count = dict(box_tie=0, gt_tie=0, shared_best=0, zero=0, threshold=0)
    for area in case['areas']:
        lo, hi = area_ranges[area_index[area]]
        for limit in case['limits']:
            for g, boxes in zip(case['gt_boxes'], case['candidates']):
                a = seg_areas(g).astype(np.float64)
                g = g[(a >= lo) & (a <= hi)].astype(np.float64)
                if limit is not None and len(boxes) > limit:
                    boxes = boxes[:limit]
                if len(boxes) == 0 or len(g) == 0:
                    continue
                ov = overlaps(boxes, g)
                first_choice = ov.argmax(axis=0)
                for _ in range(len(g)):
                    col_max = ov.max(axis=0)
                    gi = col_max.argmax()
                    bi = ov[:, gi].argmax()
                    best = col_max[gi]
                    count['gt_tie'] += int((col_max == best).sum() > 1)
                    count['box_tie'] += int((ov[:, gi] == best).sum() > 1)
                    count['shared_best'] += int(first_choice[gi] != bi)
                    count['zero'] += int(best == 0)
                    count['threshold'] += int(best == 0.5)
                    ov[bi, :] = -1
                    ov[:, gi] = -1
    return count
