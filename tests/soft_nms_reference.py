"""NumPy statement of Soft-NMS at test time (wssdl_post_detections_soft, include/wssdl_bus_hip.h) on the pieces the
neighbouring statements are made of: tta_reference.image_rows (the views' rows of an output image, un-mirrored) and
post_agnostic_reference.cap.  Also the case builders of tests/test_soft_nms_cpu.py and tests/test_gpu_soft_nms.py.
Helper module: no test in it."""
import numpy as np

import decode_reference as D
import post_agnostic_reference as PA
import tta_reference as T

F32 = np.float32
THRESH = 0.05
NMS = 0.3
SIGMA = 0.5
FLOOR = 0.001
HARD, LINEAR, GAUSSIAN = 0, 1, 2


def soft_class(cands, method, nms_thresh, sigma, min_score, record=None, ties=None):
    """step 2 for one class of one image: cands [n,5] f32 (box, score) in ascending row order, all live.  Returns the
    emitted rows [m,5] f32 in pick order.  record: a list that receives every f64 exp argument (method 2); ties: a list
    that receives 1 per pick that had to choose among equal scores."""
    c = np.ascontiguousarray(np.asarray(cands, F32).reshape(-1, 5))
    n = len(c)
    x1, y1, x2, y2 = (c[:, k].copy() for k in range(4))
    s = c[:, 4].copy()
    area = ((x2 - x1) + F32(1)) * ((y2 - y1) + F32(1))
    assert area.dtype == F32
    live = np.ones(n, bool)
    out = []
    with np.errstate(all="ignore"):
        while live.any():
            idx = np.flatnonzero(live)
            top = s[idx].max()
            best = idx[s[idx] == top]
            if ties is not None and len(best) > 1:
                ties.append(1)
            i = best[-1]                                            # among equal scores the largest local row
            out.append((x1[i], y1[i], x2[i], y2[i], s[i]))
            live[i] = False
            j = np.flatnonzero(live)
            if len(j) == 0:
                break
            w = np.maximum(F32(0), (np.minimum(x2[i], x2[j]) - np.maximum(x1[i], x1[j])) + F32(1))
            h = np.maximum(F32(0), (np.minimum(y2[i], y2[j]) - np.maximum(y1[i], y1[j])) + F32(1))
            inter = w * h
            ov = inter / ((area[i] + area[j]) - inter)
            assert ov.dtype == F32
            o64 = ov.astype(np.float64)
            if method == HARD:
                wt = np.where(o64 >= nms_thresh, F32(0), F32(1))
            elif method == LINEAR:
                wt = np.where(o64 >= nms_thresh, F32(1) - ov, F32(1))
            else:
                arg = -(o64 * o64) / np.float64(sigma)
                if record is not None:
                    record.append(arg[ov != 0])
                wt = np.exp(arg).astype(F32)
                wt[ov == 0] = F32(1)
            dec = s[j] * wt.astype(F32)
            assert dec.dtype == F32
            s[j] = dec
            live[j[~(dec > F32(min_score))]] = False
    return np.asarray(out, F32).reshape(-1, 5)


def post_soft_image(scores, boxes, K, thresh, max_per_image, method, nms_thresh, sigma, min_score, record=None, ties=None):
    """steps 1-4 on one output image's merged, un-mirrored rows: {j: dets [n,5] f32}"""
    scores = np.asarray(scores, F32).reshape(-1, K)
    boxes = np.asarray(boxes, F32).reshape(-1, 4 * K)
    dets = {}
    for j in range(1, K):
        inds = np.where((scores[:, j] > F32(thresh)) & (scores[:, j] > F32(min_score)))[0]
        cands = np.hstack((boxes[inds, 4 * j:4 * j + 4], scores[inds, j:j + 1])).astype(F32)
        dets[j] = soft_class(cands, method, nms_thresh, sigma, min_score, record, ties)
    return PA.cap(dets, K, max_per_image)


def post_soft(rois, scores, boxes, n_images, views, flip_width, K, thresh, max_per_image, method, nms_thresh=NMS,
              sigma=SIGMA, min_score=FLOOR, pitch=None, record=None, ties=None):
    """the whole statement: a list of n_images entries {j: dets [n,5]}; None for an image whose views span more than
    `pitch` rows (the op's counts[t, 0] = -1)"""
    out = []
    for t in range(n_images):
        s, b, span = T.image_rows(rois, scores, boxes, t, views, n_images, flip_width)
        if pitch is not None and span > pitch:
            out.append(None)
            continue
        out.append(post_soft_image(s, b, K, thresh, max_per_image, method, nms_thresh, sigma, min_score, record, ties))
    return out


def exp_arguments(case, thresh=THRESH, nms_thresh=NMS, sigma=SIGMA, min_score=FLOOR):
    """every f64 argument the Gaussian statement hands to exp on this case (cap off: the cap does not change them)"""
    rec = []
    post_soft(case["rois"], case["scores"], case["boxes"], case["n_images"], case["views"], case["flip_width"], case["K"],
              thresh, 0, GAUSSIAN, nms_thresh, sigma, min_score, record=rec)
    return np.concatenate(rec) if rec else np.zeros((0,), np.float64)


def gaussian_is_safe(case, **kw):
    """the precondition for bit equality under method 2: every exp value of the case lies more than 4 f64 ulps from
    every f32 midpoint (decode_reference.exp_value_is_safe), so two faithful f64 exps round to the same f32"""
    a = exp_arguments(case, **kw)
    return bool(D.exp_value_is_safe(np.exp(a)).all()), len(a)


# ------------------------------------------------------------------------------------------------ case builders ---
def set_candidate_counts(case, counts, rs, thresh=THRESH):
    """counts {(t, j): n}: class j of output image t keeps exactly n rows above the threshold (fresh scores in
    (0.06, 0.95) on n of its rows drawn at random, 0.01 on the others); the other segments stay as drawn"""
    col = case["rois"][:, 0]
    V = case["views"]
    for (t, j), n in counts.items():
        rows = np.where((col >= t * V) & (col < (t + 1) * V))[0]
        assert 0 <= n <= len(rows), (t, j, n, len(rows))
        case["scores"][rows, j] = F32(0.01)
        pick = rs.choice(rows, size=n, replace=False)
        case["scores"][pick, j] = rs.uniform(0.06, 0.95, size=n).astype(F32)
    return case


def plant_decayed_tie(case, t=0, j=1):
    """On the first three rows of output image t (view 0), class j: a top box A (0.97) and two boxes B, C that do not
    meet each other, have IoU exactly 1/3 with A each (A shifted by half its width to either side) and share the score
    0.9: after A's pick both carry the same decayed score, and the later row, C, goes first.  Far from every drawn box
    (y >= 800)."""
    col = case["rois"][:, 0]
    rows = np.where(col == t * case["views"])[0][:3]
    assert len(rows) == 3
    w = case["flip_width"][t * case["views"]]
    for r, (x1, s) in zip(rows, ((300, 0.97), (325, 0.9), (275, 0.9))):
        b = np.asarray([x1, 800, x1 + 49, 849], F32)
        if w >= 0:
            b = np.asarray([w - b[2] - 1, b[1], w - b[0] - 1, b[3]], F32)
        case["boxes"][r, 4 * j:4 * j + 4] = b
        case["scores"][r, j] = F32(s)
    return case


def build_case(seed, rows, views, K, counts=None, tie=False, method_safe=True, **kw):
    """tta_reference.build_case plus the candidate counts and the planted decayed tie, redrawn WHOLE (next attempt
    seed) until every exp of the Gaussian statement is safe -- never trimmed: decay chains, one value cannot be swapped.
    With the builder's scores that was never needed (0 unsafe in 17 235 .. 18 529 exps per case), so more than 3
    attempts is an error, not a filter."""
    for attempt in range(3):
        c = T.build_case(seed + 100003 * attempt, rows, views, K, **kw)
        rs = np.random.RandomState(seed * 7 + attempt)
        if counts:
            set_candidate_counts(c, counts, rs)
        if tie:
            plant_decayed_tie(c)
        if not method_safe:
            return c
        ok, n = gaussian_is_safe(c)
        if ok:
            c["exp_calls"] = n
            return c
    raise AssertionError("no draw with safe exponentials in 3 attempts")


def hand_case():
    """three boxes on integers, one class: A = [0,0,9,9] (0.9); B = [0,0,9,4] (0.8), half of A: IoU 50/100 = 0.5;
    C = [6,0,15,4] (0.7): with A 20/130 = 2/13, with B 20/80 = 0.25.  The f32 quotients 0.5 and 0.25 are exact."""
    return np.asarray([[0, 0, 9, 9, 0.9], [0, 0, 9, 4, 0.8], [6, 0, 15, 4, 0.7]], F32)


def hand_case_at_threshold():
    """the planted pair of tta_reference.build_case: a 6 x 13 box across a 13 x 6 one, 36 / 120: the f32 quotient is
    f32(0.3), which as a double is >= 0.3 -- the pair decays under linear at Nt = 0.3 (the >= side)"""
    return np.asarray([[500, 800, 505, 812, 0.9], [500, 800, 512, 805, 0.8]], F32)
