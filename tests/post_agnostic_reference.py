"""NumPy statement of the class-agnostic post-detection step (reference fast_rcnn/test_bus.py:360-401 with
cfg.TEST.CLS_AGNOSTIC_NMS = True) on oracle.np_oracle.nms, which is pinned to the reference's compiled utils/nms.pyx
(tests/golden/nms_utils.npz).  The rest of those lines is array bookkeeping, restated here line by line.  Helper
module: no test in it."""
import numpy as np

from oracle import np_oracle as O


def per_class(scores, boxes, K, thresh, nms_thresh):
    """:360-370 -- per class j >= 1: rows with scores[:, j] > thresh, NMS, kept rows in descending score order."""
    out = {}
    for j in range(1, K):
        inds = np.where(scores[:, j] > thresh)[0]
        d = np.hstack((boxes[inds, 4 * j:4 * j + 4], scores[inds, j:j + 1])).astype(np.float32)
        out[j] = d[O.nms(d, nms_thresh)] if len(d) else d.reshape(0, 5)
    return out


def cap(dets, K, max_per_image):
    """:389-396 -- image_thresh = sort(all kept scores)[-max_per_image]; every class keeps score >= image_thresh."""
    if max_per_image > 0:
        alls = np.hstack([dets[j][:, 4] for j in range(1, K)])
        if len(alls) > max_per_image:
            th = np.sort(alls)[-max_per_image]
            dets = {j: dets[j][dets[j][:, 4] >= th] for j in range(1, K)}
    return dets


def union_pass(dets, K, nms_thresh):
    """:371-384 -- the classes' kept rows concatenated in class order, each tagged with its class; one more NMS over
    all of them; class j keeps the survivors tagged j (in the order NMS returned them: descending score)."""
    all_dets = np.vstack([np.hstack((dets[j], np.full((len(dets[j]), 1), j, np.float32))) for j in range(1, K)])
    if len(all_dets):
        keep = O.nms(np.ascontiguousarray(all_dets[:, :5]), nms_thresh)
        all_dets = all_dets[keep]
    return {j: np.ascontiguousarray(all_dets[all_dets[:, 5] == j][:, :5]) for j in range(1, K)}


def post_detections(scores, boxes, K, thresh, max_per_image, nms_thresh, agnostic=True):
    """{j: dets [n,5] f32} of one image; agnostic=False is the per-class statement (no union pass)."""
    scores = np.asarray(scores, np.float32).reshape(-1, K)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4 * K)
    dets = per_class(scores, boxes, K, thresh, nms_thresh)
    if agnostic:
        dets = union_pass(dets, K, nms_thresh)
    return cap(dets, K, max_per_image)


def iou_f64(a, b):
    """IoU of boxes a [n,4] against b [m,4] with the +1 pixel convention, f64 (for preconditions, not for results)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]) + 1
    ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]) + 1
    inter = np.clip(iw, 0, None) * np.clip(ih, 0, None)
    area = lambda x: (x[:, 2] - x[:, 0] + 1) * (x[:, 3] - x[:, 1] + 1)      # noqa: E731
    return inter / (area(a)[:, None] + area(b)[None, :] - inter)


def ties_are_harmless(scores, boxes, K, thresh, nms_thresh):
    """The precondition under which greedy NMS does not depend on the order among equal scores: among the rows above
    the score threshold (all classes together, as the union pass sees them) any two EQUAL scores belong to boxes whose
    IoU is below nms_thresh."""
    scores = np.asarray(scores, np.float32).reshape(-1, K)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4 * K)
    s = np.concatenate([scores[scores[:, j] > thresh, j] for j in range(1, K)])
    b = np.concatenate([boxes[scores[:, j] > thresh, 4 * j:4 * j + 4] for j in range(1, K)])
    order = np.argsort(s, kind="stable")
    s, b = s[order], b[order]
    start = 0
    for end in range(1, len(s) + 1):
        if end == len(s) or s[end] != s[start]:
            if end - start > 1:
                ov = iou_f64(b[start:end], b[start:end])
                np.fill_diagonal(ov, 0.0)
                if ov.max() >= nms_thresh:
                    return False
            start = end
    return True
