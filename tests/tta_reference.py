"""NumPy statement of test-time flip augmentation and box voting (wssdl_post_detections_views,
include/wssdl_bus_hip.h), one output image at a time, on the pieces the neighbouring statements are made of:
post_agnostic_reference.per_class / union_pass / cap (the reference's fast_rcnn/test_bus.py:360-401 on np_oracle.nms),
np_oracle.bbox_overlaps (utils/bbox.pyx) and np_oracle.flip_boxes (datasets/imdb.py:106-121).  Also the case builders
of tests/test_tta_cpu.py and tests/test_gpu_tta.py.  Helper module: no test in it."""
import numpy as np

import post_agnostic_reference as PA
from oracle import np_oracle as O

THRESH = 0.05
NMS = 0.3


def unmirror(boxes, width):
    """step 1 for the rows of one mirrored source image of original width `width`: per class
    x1' = max((w - x2) - 1, 0), x2' = (w - x1) - 1, every operation in f32 (np_oracle.flip_boxes, then the clamp)"""
    b = np.array(boxes, dtype=np.float32, copy=True)
    w = np.float32(width)
    for j in range(b.shape[1] // 4):
        f = O.flip_boxes(b[:, 4 * j:4 * j + 4], w)
        assert f.dtype == np.float32
        f[:, 0] = np.maximum(f[:, 0], np.float32(0))
        b[:, 4 * j:4 * j + 4] = f
    return b


def image_rows(rois, scores, boxes, t, views, n_images, flip_width):
    """the rows of output image t in ascending row order, all views together, un-mirrored: (scores [n,K], boxes [n,4K],
    span) -- span = last - first + 1 of its rows in the blob (dead rows in between included: what the pitch must hold)"""
    col = rois[:, 0]
    live = (col >= 0) & (col < n_images * views)
    src = np.where(live, col, 0).astype(np.int64)
    rows = np.where(live & (src // views == t))[0]
    if len(rows) == 0:
        return scores[:0], boxes[:0].astype(np.float32), 0
    b = np.array(boxes[rows], dtype=np.float32, copy=True)
    if flip_width is not None:
        for s in np.unique(src[rows]):
            if flip_width[s] >= 0:
                m = src[rows] == s
                b[m] = unmirror(b[m], flip_width[s])
    return scores[rows], b, int(rows[-1] - rows[0] + 1)


def vote(dets, cands, vote_thresh):
    """step 5 for one class: dets [n,5] after NMS and cap, cands [m,5] the class's rows above the score threshold
    (pre-NMS, un-mirrored, ascending row order).  A candidate votes when bbox_overlaps(candidate, detection) >=
    vote_thresh; f64 sums serially in row order, one division, one rounding to f32."""
    out = np.array(dets, dtype=np.float32, copy=True)
    if len(out) == 0 or len(cands) == 0:
        return out
    ov = O.bbox_overlaps(np.ascontiguousarray(cands[:, :4], dtype=np.float64),
                         np.ascontiguousarray(out[:, :4], dtype=np.float64))            # [m, n]
    for i in range(len(out)):
        sw = 0.0
        sx = [0.0, 0.0, 0.0, 0.0]
        for c in np.where(ov[:, i] >= vote_thresh)[0]:
            s = float(cands[c, 4])
            sw += s
            for k in range(4):
                sx[k] += s * float(cands[c, k])
        assert sw > 0, "the detection itself votes"
        for k in range(4):
            out[i, k] = np.float32(np.float64(sx[k]) / np.float64(sw))
    return out


def post_views_image(scores, boxes, K, thresh, max_per_image, nms_thresh, agnostic, vote_thresh):
    """steps 2-5 on one output image's merged, un-mirrored rows: {j: dets [n,5] f32}"""
    scores = np.asarray(scores, np.float32).reshape(-1, K)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4 * K)
    dets = PA.per_class(scores, boxes, K, thresh, nms_thresh)
    if agnostic:
        dets = PA.union_pass(dets, K, nms_thresh)
    dets = PA.cap(dets, K, max_per_image)
    if vote_thresh > 0:
        for j in range(1, K):
            inds = np.where(scores[:, j] > thresh)[0]
            cands = np.hstack((boxes[inds, 4 * j:4 * j + 4], scores[inds, j:j + 1])).astype(np.float32)
            dets[j] = vote(dets[j], cands, vote_thresh)
    return dets


def post_views(rois, scores, boxes, n_images, views, flip_width, K, thresh, max_per_image, nms_thresh, agnostic,
               vote_thresh, pitch=None):
    """the whole statement: a list of n_images entries {j: dets [n,5]}; None for an image whose views span more than
    `pitch` rows (the op's counts[t, 0] = -1)"""
    out = []
    for t in range(n_images):
        s, b, span = image_rows(rois, scores, boxes, t, views, n_images, flip_width)
        if pitch is not None and span > pitch:
            out.append(None)
            continue
        out.append(post_views_image(s, b, K, thresh, max_per_image, nms_thresh, agnostic, vote_thresh))
    return out


def canon(a):
    """rows of EQUAL score come in an order the reference leaves to argsort"""
    a = np.asarray(a, np.float32).reshape(-1, 5)
    return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0], -a[:, 4]))] if len(a) else a


def same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ case builders ---
def _view_rows(rs, n, K, width, quarter=True):
    """n rows of one view in the image's own frame: clusters of boxes around a few centres (NMS and voting both have
    work), coordinates on quarter pixels inside [0, width - 1]"""
    centres = rs.uniform(40, width - 40, size=(max(n // 5, 1), 2)) * [1.0, 0.6]
    ctr = centres[rs.randint(0, len(centres), size=n)][:, None, :] + rs.normal(0, 5, size=(n, K, 2))
    wh = rs.uniform(30, 90, size=(n, K, 2))
    b = np.concatenate((ctr - wh / 2, ctr + wh / 2), axis=2)
    b = np.clip(b, 0, width - 1)
    if quarter:
        b = np.round(b * 4) / 4
    scores = rs.uniform(0, 0.95, size=(n, K)).astype(np.float32)         # (planted rows score above 0.95)
    return scores, b.reshape(n, 4 * K).astype(np.float32)


def mirror_into_view(boxes, width):
    """what a mirrored view reports for boxes given in the image's own frame (exact on quarter pixels)"""
    b = np.array(boxes, dtype=np.float32, copy=True)
    w = np.float32(width)
    x1, x2 = b[:, 0::4].copy(), b[:, 2::4].copy()
    b[:, 0::4] = w - x2 - np.float32(1)
    b[:, 2::4] = w - x1 - np.float32(1)
    return b


def build_case(seed, rows, views, K, mirrored=(1,), padded=None, low=(), empty=(), plant=None, cap_ties=False,
               width=1000.0, nms_thresh=NMS, thresh=THRESH):
    """A blob of len(rows) output images x `views` views; rows[t] = rows per view of image t.  Views listed in
    `mirrored` report mirrored coordinates (flip_width = width there).  padded: every view padded to that many rows with
    dead rows (batch index -1, garbage).  low / empty: (t, v) pairs whose view scores below every threshold / has no
    row.  plant: 'nms' or 'vote' puts a pair with IoU exactly 0.3 / 0.5 on top of image 0, view 0.  cap_ties: four
    far-apart rows of class 1 share one score.  Redraws until ties_are_harmless holds on every image's merged,
    un-mirrored candidates."""
    n_images = len(rows)
    for attempt in range(200):
        rs = np.random.RandomState(seed * 1000 + attempt)
        R, S, B = [], [], []
        fw = np.full((n_images * views,), -1.0, np.float32)
        for t in range(n_images):
            for v in range(views):
                src = t * views + v
                n = 0 if (t, v) in empty else rows[t]
                s, b = _view_rows(rs, n, K, width)
                if (t, v) in low:
                    s[:] = np.float32(0.01)
                if t == 0 and v == 0 and plant is not None and n >= 2:
                    # with the +1 pixel convention: 'vote' -- a 10 x 10 box inside a 20 x 10 one, 100 / 200 = 0.5 exactly
                    # (the larger one is suppressed at 0.3 and votes at 0.5); 'nms' -- a 6 x 13 box across a 13 x 6 one,
                    # areas 78 and 78, intersection 36, 36 / 120 = 0.3: the f32 quotient of cpu_nms is f32(0.3), which
                    # as a double is >= 0.3, so the pair sits on the suppressing side of the boundary
                    pair = {"vote": ([500, 800, 509, 809], [500, 800, 519, 809]),
                            "nms": ([500, 800, 505, 812], [500, 800, 512, 805])}[plant]
                    for q in range(2):
                        b[q] = np.tile(np.asarray(pair[q], np.float32), K)
                        s[q, 1:] = (0.99 - 0.01 * q - 0.001 * np.arange(1, K)).astype(np.float32)
                if cap_ties and t == 0 and v == 0 and n >= 8:
                    # four rows of class 1 with the image's best score, far from each other and from every other box:
                    # all four survive, and a cap below four keeps all four (ties stay)
                    s[4:8, 1] = np.float32(0.9975)
                    b[4:8, 4:8] = np.asarray([[10, 700, 60, 750]], np.float32) + \
                        np.arange(4, dtype=np.float32)[:, None] * np.asarray([[200, 0, 200, 0]], np.float32)
                if v in mirrored:
                    fw[src] = np.float32(width)
                    b = mirror_into_view(b, width)
                r = np.zeros((n, 5), np.float32)
                r[:, 0] = src
                r[:, 1:] = rs.uniform(0, 500, size=(n, 4))
                R.append(r)
                S.append(s)
                B.append(b)
                if padded is not None:
                    d = padded - n
                    dr = rs.uniform(0, 500, size=(d, 5)).astype(np.float32)
                    dr[:, 0] = -1
                    R.append(dr)
                    S.append(rs.uniform(0, 1, size=(d, K)).astype(np.float32))
                    B.append(rs.uniform(0, 900, size=(d, 4 * K)).astype(np.float32))
        rois = np.concatenate(R) if R else np.zeros((0, 5), np.float32)
        scores = np.concatenate(S) if S else np.zeros((0, K), np.float32)
        boxes = np.concatenate(B) if B else np.zeros((0, 4 * K), np.float32)
        ok = True
        for t in range(n_images):
            s, b, _ = image_rows(rois, scores, boxes, t, views, n_images, fw)
            ok = ok and PA.ties_are_harmless(s, b, K, thresh, nms_thresh)
        if ok:
            return dict(rois=rois, scores=scores, boxes=boxes, flip_width=fw, n_images=n_images, views=views, K=K)
    raise AssertionError("no draw without harmful ties in 200 attempts")


def pitch_of(case):
    """the smallest pitch the case fits: the longest span of an output image's rows"""
    p = 1
    for t in range(case["n_images"]):
        p = max(p, image_rows(case["rois"], case["scores"], case["boxes"], t, case["views"], case["n_images"],
                              case["flip_width"])[2])
    return p
