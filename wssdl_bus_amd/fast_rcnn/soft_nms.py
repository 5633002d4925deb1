"""Soft-NMS at test time (Bodla et al., 2017; an addition, not in the reference): cfg.TEST.SOFT_NMS = 'linear' or
'gaussian' lowers the score of an overlapped box instead of deleting it.  The statement is the header comment of
wssdl_post_detections_soft (include/wssdl_bus_hip.h); its NumPy form for the tests is tests/soft_nms_reference.py.

post_detections_soft_device is the device op (csrc/soft_nms.hip: one set of launches for the batch, all views, no
read-back); soft_nms_host / postprocess_soft_host are the same statement on the host with equal bits, for CPU
tensors, cfg.TEST.FUSED_POST_DETECTIONS = False and pitches above WSSDL_POST_SOFT_MAX_ROWS.  postprocess_soft_batch and
postprocess_soft are what detect_batch.postprocess_detections_batch and post_detections.postprocess_detections route
to under the switch.  cfg.TEST.SOFT_NMS, SOFT_NMS_SIGMA and SOFT_NMS_MIN_SCORE are read at every call."""
import numpy as np
import torch

from .config import cfg

HARD, LINEAR, GAUSSIAN = 0, 1, 2
_METHODS = {"hard": HARD, "linear": LINEAR, "gaussian": GAUSSIAN}
_FLT_MIN = float(np.finfo(np.float32).tiny)


def soft_nms_method(method=None):
    """The op's `method` for a name ('hard' | 'linear' | 'gaussian') or number; None reads cfg.TEST.SOFT_NMS, where
    'off' gives None (no Soft-NMS).  Anything else: ValueError.  Under cfg.TEST.SOFT_NMS != 'off' the switches
    CLS_AGNOSTIC_NMS and BBOX_VOTE raise ValueError: what each would mean with decayed scores is not defined here."""
    if method is None:
        name = cfg.TEST.SOFT_NMS
        if name == "off":
            return None
        if name not in ("linear", "gaussian"):
            raise ValueError("cfg.TEST.SOFT_NMS must be 'off', 'linear' or 'gaussian', got %r" % (name,))
        if cfg.TEST.CLS_AGNOSTIC_NMS or cfg.TEST.BBOX_VOTE:
            raise ValueError("cfg.TEST.SOFT_NMS = %r cannot be combined with cfg.TEST.CLS_AGNOSTIC_NMS or "
                             "cfg.TEST.BBOX_VOTE" % (name,))
        return _METHODS[name]
    if isinstance(method, str):
        if method not in _METHODS:
            raise ValueError("Soft-NMS method must be 'hard', 'linear' or 'gaussian', got %r" % (method,))
        return _METHODS[method]
    if method not in (HARD, LINEAR, GAUSSIAN):
        raise ValueError("Soft-NMS method must be 0 (hard), 1 (linear) or 2 (gaussian), got %r" % (method,))
    return int(method)


def _parameters(method, thresh, nms_thresh, sigma, min_score):
    """(method, nms_thresh, sigma, min_score) with the cfg defaults, checked like the entry point checks them"""
    m = soft_nms_method(method)
    if m is None:
        raise ValueError("cfg.TEST.SOFT_NMS is 'off'")
    nt = float(cfg.TEST.NMS if nms_thresh is None else nms_thresh)
    sg = float(cfg.TEST.SOFT_NMS_SIGMA if sigma is None else sigma)
    ms = float(np.float32(cfg.TEST.SOFT_NMS_MIN_SCORE if min_score is None else min_score))
    if m == HARD and min_score is None:
        ms = max(_FLT_MIN, min(ms, float(np.float32(thresh))))       # the hard op has no floor of its own
    if m == GAUSSIAN and not (sg > 0.0 and np.isfinite(sg)):
        raise ValueError("Soft-NMS: sigma must be positive and finite, got %r" % (sg,))
    if m != GAUSSIAN and not (0.0 < nt <= 1.0):
        raise ValueError("Soft-NMS: the NMS threshold must lie in (0, 1], got %r" % (nt,))
    if not (_FLT_MIN <= ms < 1.0):
        raise ValueError("Soft-NMS: the score floor must lie in [FLT_MIN, 1), got %r" % (ms,))
    if not thresh >= 0:
        raise ValueError("Soft-NMS: the score threshold must be >= 0, got %r" % (thresh,))
    return m, nt, sg, ms


def soft_nms_host(dets, method, nms_thresh, sigma, min_score):
    """Step 2 of the statement for one class of one image on the host: dets [n,5] f32 NumPy (box, score), the
    candidates in ascending row order, all above min_score.  Returns the emitted detections [m,5] f32 in the order of
    the picks (descending score).  Every f32 operation is rounded on its own; the Gaussian weight goes through f64."""
    m = soft_nms_method(method)
    d = np.ascontiguousarray(np.asarray(dets, dtype=np.float32).reshape(-1, 5))
    one, zero, floor = np.float32(1), np.float32(0), np.float32(min_score)
    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    s = d[:, 4].copy()
    s[~(s > floor)] = zero
    area = (x2 - x1 + one) * (y2 - y1 + one)
    out = np.zeros((len(d), 5), np.float32)
    n = 0
    with np.errstate(all="ignore"):
        for _ in range(len(d)):
            top = s.max() if len(s) else zero
            if not top > zero:
                break
            i = int(np.flatnonzero(s == top)[-1])                    # among equal scores the later row
            out[n, :4] = d[i, :4]
            out[n, 4] = top
            n += 1
            s[i] = zero
            live = np.flatnonzero(s > zero)
            if len(live) == 0:
                break
            w = np.maximum(zero, np.minimum(x2[i], x2[live]) - np.maximum(x1[i], x1[live]) + one)
            h = np.maximum(zero, np.minimum(y2[i], y2[live]) - np.maximum(y1[i], y1[live]) + one)
            inter = w * h
            ov = inter / ((area[i] + area[live]) - inter)
            ov64 = ov.astype(np.float64)
            if m == GAUSSIAN:
                wt = np.exp(-(ov64 * ov64) / np.float64(sigma)).astype(np.float32)
                wt[ov == zero] = one
            elif m == LINEAR:
                wt = np.where(ov64 >= nms_thresh, one - ov, one).astype(np.float32)
            else:
                wt = np.where(ov64 >= nms_thresh, zero, one).astype(np.float32)
            dec = s[live] * wt
            s[live] = np.where(dec > floor, dec, zero)
    return out[:n]


def _cap(dets, num_classes, max_per_image):
    """test_bus.py:389-396 over the emitted scores: image_thresh = sort(all scores)[-max_per_image], ties stay"""
    if max_per_image > 0:
        alls = np.concatenate([dets[j][:, 4] for j in range(1, num_classes)])
        if len(alls) > max_per_image:
            th = np.sort(alls)[-max_per_image]
            dets = {j: dets[j][dets[j][:, 4] >= th] for j in range(1, num_classes)}
    return dets


@torch.no_grad()
def postprocess_soft_host(scores, boxes, num_classes, thresh=0.05, max_per_image=300, method=None, nms_thresh=None,
                          sigma=None, min_score=None):
    """The statement for ONE image's rows (already un-mirrored, ascending row order) on the host: scores [n,K],
    boxes [n,4K] tensors of any device -> {j: dets [m,5] f32} on the device of `scores`, bit for bit the device op's."""
    m, nt, sg, ms = _parameters(method, thresh, nms_thresh, sigma, min_score)
    s = scores.detach().to(torch.float32).cpu().numpy().reshape(-1, num_classes)
    b = boxes.detach().to(torch.float32).cpu().numpy().reshape(-1, 4 * num_classes)
    out = {}
    for j in range(1, num_classes):
        inds = np.where((s[:, j] > np.float32(thresh)) & (s[:, j] > np.float32(ms)))[0]
        cands = np.hstack((b[inds, 4 * j:4 * j + 4], s[inds, j:j + 1])).astype(np.float32)
        out[j] = soft_nms_host(cands, m, nt, sg, ms)
    out = _cap(out, num_classes, int(max_per_image))
    return {j: torch.from_numpy(np.ascontiguousarray(out[j])).to(scores.device) for j in range(1, num_classes)}


def _views_pitch(r, N, V, max_rows_per_image):
    """P of the op: max_rows_per_image, default views * cfg.TEST.RPN_POST_NMS_TOP_N (<= 0: the longest image's span)"""
    P = int(max_rows_per_image) if max_rows_per_image is not None else V * int(cfg.TEST.RPN_POST_NMS_TOP_N)
    if P <= 0:
        col = r[:, 0]
        live = torch.nonzero((col >= 0) & (col < N * V)).reshape(-1)
        P = 1
        if live.numel():
            img = torch.div(col[live].to(torch.int64), V, rounding_mode="floor")
            lo = torch.full((N,), r.shape[0], dtype=torch.int64, device=r.device).scatter_reduce(0, img, live, "amin")
            hi = torch.full((N,), -1, dtype=torch.int64, device=r.device).scatter_reduce(0, img, live, "amax")
            P = max(int((hi - lo + 1).max()), 1)
    return P


@torch.no_grad()
def post_detections_soft_device(scores, boxes, rois, n_images, views, flip_width, num_classes, thresh=0.05,
                                max_per_image=300, method=None, max_rows_per_image=None, nms_thresh=None, sigma=None,
                                min_score=None):
    """Soft-NMS of a batch as one C-ABI call (wssdl_post_detections_soft: one set of launches, no read-back, one
    workspace allocation, on the current stream).  The blob behind scores [R,K] / boxes [R,4K] / rois [R,5] holds
    n_images * views source images exactly as post_detections_views_device takes them (flip_width [n_images * views]
    or None).  method: 'hard' | 'linear' | 'gaussian' or 0 | 1 | 2, None reads cfg.TEST.SOFT_NMS; nms_thresh, sigma and
    min_score default to cfg.TEST.NMS, SOFT_NMS_SIGMA and SOFT_NMS_MIN_SCORE (under 'hard' the floor defaults to no
    more than `thresh`, so that the output is the views op's).
    Returns (dets [N, K-1, P, 5] f32, counts [N, K-1] i32) on the GPU, P = max_rows_per_image (default
    views * cfg.TEST.RPN_POST_NMS_TOP_N, or the longest image when that is <= 0; at most WSSDL_POST_SOFT_MAX_ROWS);
    counts[i, 0] == -1 flags an image whose views span more than P rows."""
    from .. import _lib
    m, nt, sg, ms = _parameters(method, thresh, nms_thresh, sigma, min_score)
    _lib.require_cuda(scores, boxes, rois)
    s = scores.to(torch.float32).contiguous()
    b = boxes.to(torch.float32).contiguous()
    r = rois.to(torch.float32).contiguous()
    R, K = s.shape
    N, V = int(n_images), int(views)
    if K != num_classes or b.shape != (R, 4 * K) or r.shape != (R, 5):
        raise ValueError("expected scores [R,K], boxes [R,4K], rois [R,5] with K = num_classes")
    fw = None
    if flip_width is not None:
        fw = torch.as_tensor(flip_width, dtype=torch.float32).to(s.device).contiguous()
        if fw.shape != (N * V,):
            raise ValueError("flip_width must hold n_images * views entries")
    P = _views_pitch(r, N, V, max_rows_per_image)
    if P > _lib.POST_SOFT_MAX_ROWS:
        raise ValueError("Soft-NMS on the device: max_rows_per_image = %d exceeds WSSDL_POST_SOFT_MAX_ROWS = %d"
                         % (P, _lib.POST_SOFT_MAX_ROWS))
    L = _lib.lib()
    dets = torch.empty((N, K - 1, max(P, 1), 5), dtype=torch.float32, device=s.device)
    counts = torch.empty((N, K - 1), dtype=torch.int32, device=s.device)
    with torch.cuda.device(s.device):
        n = L.wssdl_post_detections_soft_workspace_bytes(N, V, P, K)
        ws = torch.empty((max(n, 256),), dtype=torch.uint8, device=s.device)
        _lib.check(L.wssdl_post_detections_soft(_lib.ptr(r), _lib.ptr(s), _lib.ptr(b), R, N, V,
                                                _lib.ptr(fw) if fw is not None else None, P, K, float(thresh), m, nt, sg,
                                                ms, int(max_per_image), _lib.ptr(dets), _lib.ptr(counts), _lib.ptr(ws), n,
                                                _lib.stream()), "wssdl_post_detections_soft")
    return dets, counts


def soft_device_fit(scores, num_classes, rows_per_image):
    """whether the device op takes these tensors under the current switches"""
    from .. import _lib
    return bool(scores.is_cuda and scores.shape[1] == num_classes and 2 <= num_classes <= 65 and
                cfg.TEST.get("FUSED_POST_DETECTIONS", True) and int(rows_per_image) <= _lib.POST_SOFT_MAX_ROWS)


@torch.no_grad()
def postprocess_soft_batch(scores, boxes, rois, n_images, num_classes, thresh=0.05, max_per_image=300, views=1,
                           flip_width=None):
    """postprocess_detections_batch under cfg.TEST.SOFT_NMS: a list of n_images dicts {j: dets [n,5]}.  GPU tensors
    the op takes go through post_detections_soft_device and one read-back of the counts; everything else through
    the host path image by image (unmirror_boxes, postprocess_soft_host), with equal bits."""
    from .detect_batch import unmirror_boxes
    n_images, views = int(n_images), int(views)
    soft_nms_method()                                               # the cfg errors, before anything runs
    top = int(cfg.TEST.RPN_POST_NMS_TOP_N)
    if 1 <= views <= 8 and soft_device_fit(scores, num_classes, views * top if top > 0 else scores.shape[0]):
        dets, counts = post_detections_soft_device(scores, boxes, rois, n_images, views, flip_width, num_classes, thresh,
                                                   max_per_image)
        n = counts.cpu().tolist()
        over = [i for i in range(n_images) if n[i][0] < 0]
        if over:
            raise ValueError("image(s) %s have more RoI rows than max_rows_per_image = %d (views * "
                             "cfg.TEST.RPN_POST_NMS_TOP_N)" % (over, dets.shape[2]))
        return [{j: dets[i, j - 1, :n[i][j - 1]] for j in range(1, num_classes)} for i in range(n_images)]
    ub, image = unmirror_boxes(boxes, rois, n_images, views, flip_width)
    out = []
    for i in range(n_images):
        rows = torch.nonzero(image == i).reshape(-1)
        out.append(postprocess_soft_host(scores[rows], ub[rows], num_classes, thresh, max_per_image))
    return out


@torch.no_grad()
def postprocess_soft(scores, boxes, num_classes, thresh=0.05, max_per_image=300):
    """post_detections.postprocess_detections under cfg.TEST.SOFT_NMS: one image's rows -> {j: dets [n,5]}; the
    device op with the image as a batch of one (pitch = its rows) where it applies, else the host path."""
    soft_nms_method()
    R = int(scores.shape[0])
    if R > 0 and soft_device_fit(scores, num_classes, R):
        rois = torch.zeros((R, 5), dtype=torch.float32, device=scores.device)
        dets, counts = post_detections_soft_device(scores, boxes, rois, 1, 1, None, num_classes, thresh, max_per_image,
                                                   max_rows_per_image=R)
        n = counts.cpu().tolist()[0]
        return {j: dets[0, j - 1, :n[j - 1]] for j in range(1, num_classes)}
    return postprocess_soft_host(scores, boxes, num_classes, thresh, max_per_image)
