"""Shared by test_boxcode_reference_cpu.py, test_gpu_boxcode_reference.py and tools/proposal_fuzz.py: the box arithmetic
of the three kernels that feed training -- decode_anchor (csrc/proposal.hip), anchor_targets_kernel (csrc/anchor_target.hip)
and roi_targets_kernel (csrc/roi_targets.hip) -- restated in NumPy operation by operation, an f64 evaluation of the same
formulas with a bound counted from the statement's roundings, the guards under which two faithful f64 exp / log
implementations round to the same f32, and the seeded cases.  NumPy only: no import of the package, none of oracle/.

The statements: every f32 operation in np.float32 (NumPy rounds each elementwise f32 operation on its own, the library is
built with -ffp-contract=off; f32 and f64 division are IEEE on both sides), every f64 operation in np.float64, the one
transcendental of each formula as an f64 exp / log rounded once to f32.

What the statements leave undefined, because no case reaches it: an operand that is NaN (the kernels clip with fminf /
fmaxf, which drop a NaN; the statement uses np.fmin / np.fmax, which do the same), the sign of a zero that the clip's
max(v, 0) returns for v = -0.0 (no case decodes a corner to -0.0: a difference a - b of f32 values is -0.0 only for
a = -0.0, b = +0.0), and the logarithm of a ground-truth box of non-positive width (every case keeps x2 >= x1, y2 >= y1)."""
import numpy as np

import decode_reference as D
from decode_reference import F32, U

F64 = np.float64


def exp_is_safe(d):
    """decode_reference.exp_is_safe: the f64 value of exp(d) lies more than 4 f64 ulps from every f32 rounding midpoint.
    (An exp beyond the f32 range is safe: every value that far out rounds to inf.)"""
    with np.errstate(over="ignore"):
        return D.exp_is_safe(d)


STRIDE = 16
SCALES = (8, 16, 32)
SMALL_SCALES = (1, 2, 4)


# ----------------------------------------------------------------------------------------------- anchors ---

def generate_anchors(base_size=16, ratios=(0.5, 1.0, 2.0), scales=SCALES):
    """the base anchors [len(ratios) * len(scales), 4] f64, ratio-major: a (0, 0, base - 1, base - 1) window re-shaped to
    every aspect ratio at constant area (sides rounded half to even), then scaled about its centre"""
    c = 0.5 * (base_size - 1)
    out = []
    for r in ratios:
        w = np.round(np.sqrt(float(base_size) * base_size / r))
        h = np.round(w * r)
        for s in scales:
            out.append([c - 0.5 * (w * s - 1), c - 0.5 * (h * s - 1), c + 0.5 * (w * s - 1), c + 0.5 * (h * s - 1)])
    return np.array(out, F64)


def shifted_anchors(H, W, stride=STRIDE, scales=SCALES):
    """[H * W * A, 4] f64, row (h * W + w) * A + a = base[a] + stride * (w, h, w, h): integer-valued"""
    base = generate_anchors(scales=scales)
    gx, gy = np.meshgrid(np.arange(W) * float(stride), np.arange(H) * float(stride))
    sh = np.stack((gx.ravel(), gy.ravel(), gx.ravel(), gy.ravel()), 1)
    return (base[None] + sh[:, None]).reshape(-1, 4)


def log_value_is_safe(v):
    """True where the f64 value v (a logarithm) lies more than 4 f64 ulps from every midpoint between adjacent f32
    values: two faithful f64 log implementations (each within 1 ulp of the true value) then round to the same f32.
    The rule of decode_reference.exp_value_is_safe, for values of either sign (np.spacing carries the value's sign)."""
    v = np.asarray(v, F64)
    f = v.astype(F32)
    up = (f.astype(F64) + np.nextafter(f, F32(np.inf)).astype(F64)) / 2.0                    # exact in f64
    down = (f.astype(F64) + np.nextafter(f, F32(-np.inf)).astype(F64)) / 2.0
    margin = 4.0 * np.abs(np.spacing(v))
    return (np.abs(v - up) > margin) & (np.abs(v - down) > margin)


def log_is_safe(x):
    """log_value_is_safe of log(x), x the f64 argument the kernel's log sees"""
    with np.errstate(all="ignore"):
        return log_value_is_safe(np.log(np.asarray(x, F64)))


# ---------------------------------------------------------------------------------------- 1: the proposal ---

def _exp32(d):
    with np.errstate(over="ignore"):
        return np.exp(d.astype(F64)).astype(F32)


def _exp32_mutant(d):
    return np.exp(d.astype(F32))                                       # NumPy's own f32 exponential


def _exp32_one_ulp(d):
    return np.nextafter(_exp32(d), F32(np.inf))                        # the worst a faithful f32 exponential may return


def _decode_axis(a1, a2, dc, ds, lim, ex=None):
    """one axis of decode_anchor, operation by operation, on f32 scalars or arrays: anchor corners a1, a2, centre delta
    dc, size delta ds, the clip limit im - 1.  Returns (raw low corner, raw high corner, clipped low, clipped high).
    proposal_statement and the filter-edge search (_one_anchor) both go through here."""
    half, one, zero = F32(0.5), F32(1.0), F32(0.0)
    aw = (a2 - a1) + one
    c = a1 + half * aw
    pc = dc * aw
    pc = pc + c
    pw = (ex or _exp32)(ds) * aw
    hp = half * pw
    lo, hi = pc - hp, pc + hp
    return lo, hi, np.fmax(np.fmin(lo, lim), zero), np.fmax(np.fmin(hi, lim), zero)


def softmax_arguments(x, A):
    """(bg - max, fg - max) [N, M] f32 each: the two arguments the fused softmax's exponentials see"""
    x = np.asarray(x, F32)
    N = x.shape[0]
    bg, fg = x[..., :A].reshape(N, -1), x[..., A:].reshape(N, -1)
    mx = np.fmax(bg, fg)
    return bg - mx, fg - mx


def proposal_scores(x, A, from_logits):
    """[N, M] f32 in (h, w, a) order: channel A + a; with from_logits e1 / (e0 + e1), e = f32(exp(f64(x - max)))"""
    x = np.asarray(x, F32)
    if not from_logits:
        return x[..., A:].reshape(x.shape[0], -1).copy()
    t0, t1 = softmax_arguments(x, A)
    e0, e1 = _exp32(t0), _exp32(t1)
    s = e1 / (e0 + e1)
    assert s.dtype == F32
    return s


def proposal_statement(x, pred, im_info, min_size=16.0, stride=STRIDE, scales=SCALES, from_logits=False, mutant=None):
    """dict(boxes [N, M, 4] f32, valid [N, M] bool, scores [N, M] f32, bw, bh [N, M] f32, ms [N] f32, order: per image
    the candidate order of candidate_order): decode_anchor, operation by operation.  x [N, H, W, 2A] (probabilities,
    or scores with from_logits), pred [N, H, W, 4A].

    mutant (test_boxcode_reference_cpu.py only): 'gt' filters with > for >=, 'filter_first' applies the size filter to
    the unclipped box, 'exp_f32' takes NumPy's f32 exponential, 'exp_ulp' the correctly rounded one moved one f32 ulp
    up (what a faithful expf may return; unlike NumPy's it is the same on every machine)."""
    x, pred, info = np.asarray(x, F32), np.asarray(pred, F32), np.asarray(im_info, F32)
    N, H, W = x.shape[:3]
    anc = shifted_anchors(H, W, stride, scales).astype(F32)            # integer-valued f64 cast to f32
    A = anc.shape[0] // (H * W)
    d = pred.reshape(N, -1, 4)
    one = F32(1.0)
    ex = {"exp_f32": _exp32_mutant, "exp_ulp": _exp32_one_ulp}.get(mutant, _exp32)
    out = {}
    with np.errstate(all="ignore"):
        corners, raw = [None] * 4, [None] * 4
        for a in (0, 1):                                               # x, then y
            lim = (info[:, 1 - a] - one)[:, None]                      # im - 1 in f32: (w, h) = im_info[1], im_info[0]
            raw[a], raw[a + 2], corners[a], corners[a + 2] = _decode_axis(anc[None, :, a], anc[None, :, a + 2], d[:, :, a],
                                                                          d[:, :, a + 2], lim, ex)
        boxes = np.stack(corners, 2)
        ms = F32(min_size) * info[:, 2]
        src = raw if mutant == "filter_first" else corners
        bw = (src[2] - src[0]) + one
        bh = (src[3] - src[1]) + one
        if mutant == "gt":
            valid = (bw > ms[:, None]) & (bh > ms[:, None])
        else:
            valid = (bw >= ms[:, None]) & (bh >= ms[:, None])
    assert boxes.dtype == F32 and ms.dtype == F32 and bw.dtype == F32
    out.update(boxes=boxes, valid=valid, scores=proposal_scores(x, A, from_logits), bw=bw, bh=bh, ms=ms)
    out["order"] = candidate_order(out["scores"], valid)               # before any top-N cut
    return out


def candidate_order(scores, valid, topn=0):
    """per image the indices of the valid anchors by descending score, cut to topn when topn > 0.

    The tie rule, from score_key (csrc/nms.hip.h): the sort key is (order-preserving score bits << 32) | anchor index,
    and the candidates go by DESCENDING key, so of two valid anchors with the same score bits the one with the HIGHER
    index comes first (+0.0 ranks above -0.0).  The reference's own argsort()[::-1] leaves ties undefined; the cases
    keep the scores of an image pairwise distinct."""
    out = []
    for s, v in zip(np.asarray(scores, F32), np.asarray(valid, bool)):
        idx = np.nonzero(v)[0]
        idx = idx[np.lexsort((-idx, -s[idx].astype(F64)))]
        out.append(idx[:topn] if topn > 0 else idx)
    return out


def proposal_evaluate_f64(x, pred, im_info, stride=STRIDE, scales=SCALES, from_logits=False):
    """(boxes [N, M, 4] f64, bound [N, M, 4], scores [N, M] f64, score_bound [N, M]): the statement's formulas on the
    same f32 inputs in f64 (clipped to the same f32 limits), and the elementwise bound on |statement - f64|.

    Each f32 operation contributes U times the magnitude of its result; an error carried by an operand passes through
    an addition unchanged and through a multiplication scaled by the other factor.  The anchors are integers below 2^24:
    aw = (a2 - a1) + 1 and cx = a1 + 0.5 aw are exact.  So
        pcx = d.x * aw + cx       epc = U |d.x aw| + U |pcx|
        pw  = fl32(exp(d.z)) * aw epw = U E aw + U |pw|                    (E = exp(d.z); fl32: one rounding; the f64
                                                                           exp itself adds < 2^-52 relative)
        x   = pcx -+ 0.5 pw       ex  = epc + 0.5 epw + U |x|              (0.5 * pw is exact)
    The clip is monotone and 1-Lipschitz, so it adds nothing.  Where fl32(E) overflows to inf the count does not apply:
    then E >= 2^128 (1 - 2^-25), both sides have |x| > 10^38 before the clip, the clip returns the same limit on both
    sides and the bound is 0.  Magnitudes are taken from the f64 evaluation; what that neglects is second order in U,
    covered by the factor 1.001.
    The score with from_logits: t = fl32(x - max) is 0 for one channel and carries U |t| for the other, so
        e = fl32(exp(t))          ee  = E U |t| + U E                      (0 for the channel with t = 0: e = 1)
        S = e0 + e1               eS  = ee0 + ee1 + U S
        s = e1 / S                es  = s (ee1 / e1 + eS / S + U)
    Without from_logits the score is an input: bound 0."""
    x, pred, info = np.asarray(x, F32), np.asarray(pred, F32), np.asarray(im_info, F32)
    N, H, W = x.shape[:3]
    anc = shifted_anchors(H, W, stride, scales)
    A = anc.shape[0] // (H * W)
    d = pred.reshape(N, -1, 4).astype(F64)
    boxes, bound = np.zeros(d.shape), np.zeros(d.shape)
    with np.errstate(all="ignore"):
        for a in (0, 1):
            aw = ((anc[:, a + 2] - anc[:, a]) + 1.0)[None]
            c = anc[None, :, a] + 0.5 * aw
            E = np.exp(d[:, :, a + 2])
            over = np.isinf(E.astype(F32))
            pc = d[:, :, a] * aw + c
            epc = U * np.abs(d[:, :, a] * aw) + U * np.abs(pc)
            pw = E * aw
            epw = U * E * aw + U * np.abs(pw)
            lim = (info[:, 1 - a] - F32(1.0)).astype(F64)[:, None]
            for col, sign in ((a, -1.0), (a + 2, 1.0)):
                v = pc + sign * 0.5 * pw
                boxes[:, :, col] = np.maximum(np.minimum(v, lim), 0.0)
                bound[:, :, col] = np.where(over, 0.0, 1.001 * (epc + 0.5 * epw + U * np.abs(v)))
    if not from_logits:
        s = x[..., A:].reshape(N, -1).astype(F64)
        return boxes, bound, s, np.zeros(s.shape)
    t0, t1 = (t.astype(F64) for t in softmax_arguments(x, A))
    E0, E1 = np.exp(t0), np.exp(t1)
    ee0 = np.where(t0 == 0, 0.0, E0 * U * np.abs(t0) + U * E0)
    ee1 = np.where(t1 == 0, 0.0, E1 * U * np.abs(t1) + U * E1)
    S = E0 + E1
    eS = ee0 + ee1 + U * S
    s = E1 / S
    return boxes, bound, s, 1.001 * s * (ee1 / E1 + eS / S + U)


def proposal_exp_arguments(case, from_logits):
    """every argument an exponential of the run sees: the dw, dh columns, and with from_logits both softmax arguments"""
    d = case["pred"].reshape(-1, 4)[:, 2:4].ravel()
    if not from_logits:
        return d
    A = case["A"]
    return np.concatenate((d,) + tuple(t.ravel() for t in softmax_arguments(case["logits"], A)))


# ----------------------------------------------------------------------------------- 2: the anchor targets ---

def _iou_f64(b, g):
    """[B, G] f64 IoU in the operation order of the reference's Cython kernel (and of iou_f64 in anchor_target.hip)"""
    b, g = np.asarray(b, F64), np.asarray(g, F64)
    garea = ((g[:, 2] - g[:, 0]) + 1.0) * ((g[:, 3] - g[:, 1]) + 1.0)
    iw = (np.minimum(b[:, None, 2], g[None, :, 2]) - np.maximum(b[:, None, 0], g[None, :, 0])) + 1.0
    ih = (np.minimum(b[:, None, 3], g[None, :, 3]) - np.maximum(b[:, None, 1], g[None, :, 1])) + 1.0
    barea = (((b[:, 2] - b[:, 0]) + 1.0) * ((b[:, 3] - b[:, 1]) + 1.0))[:, None]
    ua = (barea + garea[None]) - iw * ih
    with np.errstate(all="ignore"):
        return np.where((iw > 0) & (ih > 0), (iw * ih) / ua, 0.0)


def admitted_rows(gt, num_gt, dataset):
    """how many leading rows of an image's gt array the arg-max runs over: SNUBH and SNUBH_FG the rows of class != 0
    (counted among the first num_gt; they come first), every other dataset all num_gt rows"""
    g = np.asarray(gt, F32)[:int(num_gt)]
    return int(np.sum(g[:, 4] != 0)) if dataset in ("SNUBH", "SNUBH_FG") else g.shape[0]


def anchor_assignment(gt_boxes, num_gt, im_info, n_images, H, W, dataset, stride=STRIDE, scales=SCALES):
    """(inside [n, M] bool, arg [n, M] int; -1 where there is no target): the inside test (x1, y1 >= 0, x2 < w, y2 < h,
    im_info as f64) and the first maximum of the f64 IoU over the admitted rows"""
    anc = shifted_anchors(H, W, stride, scales)
    info = np.asarray(im_info, F32).astype(F64)
    M = anc.shape[0]
    inside, arg = np.zeros((n_images, M), bool), np.full((n_images, M), -1, np.int64)
    for n in range(n_images):
        inside[n] = (anc[:, 0] >= 0) & (anc[:, 1] >= 0) & (anc[:, 2] < info[n, 1]) & (anc[:, 3] < info[n, 0])
        k = admitted_rows(gt_boxes[n], num_gt[n], dataset)
        if k > 0:
            ov = _iou_f64(anc, np.asarray(gt_boxes[n], F32)[:k, :4])
            arg[n] = np.where(inside[n], ov.argmax(1), -1)             # np.argmax: the first maximum
    return inside, arg


def _anchor_target_terms(gt_boxes, arg, n_images, H, W, stride, scales):
    """the pieces both the statement and the f64 evaluation start from: f64 anchor side, f32 gt side"""
    anc = shifted_anchors(H, W, stride, scales)
    ew, eh = (anc[:, 2] - anc[:, 0]) + 1.0, (anc[:, 3] - anc[:, 1]) + 1.0
    ec = (anc[:, 0] + 0.5 * ew, anc[:, 1] + 0.5 * eh)
    g = np.stack([np.asarray(gt_boxes[n], F32)[np.maximum(arg[n], 0), :4] for n in range(n_images)])    # [n, M, 4]
    return (ew, eh), ec, g


def _to_planes(t, H, W):
    """[n, M, 4] in (h, w, a) order -> the [n, 4A, H, W] plane layout: channel a * 4 + j"""
    n = t.shape[0]
    return np.ascontiguousarray(t.reshape(n, H, W, -1).transpose(0, 3, 1, 2))


def anchor_targets_statement(gt_boxes, num_gt, im_info, n_images, n_out, H, W, dataset, stride=STRIDE, scales=SCALES):
    """bbox_targets [n_out, 4A, H, W] f32.  Anchor side f64 (ew = (a2 - a1) + 1, ecx = a1 + 0.5 ew), gt side f32
    (gw = (g2 - g0) + 1, gcx = g0 + 0.5 gw) until the two meet: t0 = f32((f64(gcx) - ecx) / ew), t2 = f32(log(f64(gw) /
    ew)).  Written for every inside anchor from its arg-max gt, zero elsewhere and for the images past n_images."""
    inside, arg = anchor_assignment(gt_boxes, num_gt, im_info, n_images, H, W, dataset, stride, scales)
    e, ec, g = _anchor_target_terms(gt_boxes, arg, n_images, H, W, stride, scales)
    M = arg.shape[1]
    t = np.zeros((n_out, M, 4), F32)
    half, one = F32(0.5), F32(1.0)
    with np.errstate(all="ignore"):
        for a in (0, 1):
            gs = (g[:, :, a + 2] - g[:, :, a]) + one
            gc = g[:, :, a] + half * gs
            assert gs.dtype == F32 and gc.dtype == F32
            t[:n_images, :, a] = ((gc.astype(F64) - ec[a][None]) / e[a][None]).astype(F32)
            t[:n_images, :, a + 2] = np.log(gs.astype(F64) / e[a][None]).astype(F32)
    t[:n_images][arg < 0] = 0.0
    return _to_planes(t, H, W)


def anchor_targets_evaluate_f64(gt_boxes, num_gt, im_info, n_images, n_out, H, W, dataset, stride=STRIDE, scales=SCALES):
    """(targets [n_out, 4A, H, W] f64, bound, log_args [n, M, 2] f64; NaN where there is no target): the same formulas
    on the same f32 gt boxes in f64, for the statement's own assignment.

    The anchor side is exact (integers).  The gt side carries the two f32 roundings of gw and the one of gcx:
        gw  = (g2 - g0) + 1       egw = U |g2 - g0| + U |gw|
        gcx = g0 + 0.5 gw         egc = 0.5 egw + U |gcx|
        t0  = fl32((gcx - ecx) / ew)      e0 = egc / ew + U |t0|            (the two f64 operations add < 2^-52 relative)
        t2  = fl32(log(gw / ew))          e2 = egw / gw + U |t2|            (d log = d gw / gw; the f64 division and log
                                                                            add < 2^-51 relative)
    Second-order terms are covered by the factor 1.001.  log_args are the f64 quotients the statement's log sees."""
    inside, arg = anchor_assignment(gt_boxes, num_gt, im_info, n_images, H, W, dataset, stride, scales)
    e, ec, g32 = _anchor_target_terms(gt_boxes, arg, n_images, H, W, stride, scales)
    g = g32.astype(F64)
    M = arg.shape[1]
    t, b = np.zeros((n_out, M, 4)), np.zeros((n_out, M, 4))
    largs = np.full((n_images, M, 2), np.nan)
    with np.errstate(all="ignore"):
        for a in (0, 1):
            d = g[:, :, a + 2] - g[:, :, a]
            gs = d + 1.0
            egs = U * np.abs(d) + U * np.abs(gs)
            gc = g[:, :, a] + 0.5 * gs
            egc = 0.5 * egs + U * np.abs(gc)
            t0 = (gc - ec[a][None]) / e[a][None]
            t2 = np.log(gs / e[a][None])
            t[:n_images, :, a], b[:n_images, :, a] = t0, 1.001 * (egc / e[a][None] + U * np.abs(t0))
            t[:n_images, :, a + 2], b[:n_images, :, a + 2] = t2, 1.001 * (egs / np.abs(gs) + U * np.abs(t2))
            gs32 = (g32[:, :, a + 2] - g32[:, :, a]) + F32(1.0)
            largs[:, :, a] = np.where(arg >= 0, gs32.astype(F64) / e[a][None], np.nan)
    t[:n_images][arg < 0] = 0.0
    b[:n_images][arg < 0] = 0.0
    return _to_planes(t, H, W), _to_planes(b, H, W), largs


# -------------------------------------------------------------------------------------- 3: the RoI targets ---

def roi_assignment(rows, gt_boxes, num_gt):
    """(arg [R] int, max IoU [R] f64) of returned rows (batch index, box): the first maximum of the f64 IoU over the
    positive boxes (class != 0 among the first num_gt rows: they come first) of the row's image; -1 for a row of no image"""
    rows = np.asarray(rows, F32)
    arg, best = np.full(rows.shape[0], -1, np.int64), np.zeros(rows.shape[0])
    for r in range(rows.shape[0]):
        i = int(rows[r, 0])
        if 0 <= i < len(num_gt):
            k = admitted_rows(gt_boxes[i], num_gt[i], "SNUBH")
            if k > 0:
                ov = _iou_f64(rows[r:r + 1, 1:5], np.asarray(gt_boxes[i], F32)[:k, :4])[0]
                arg[r], best[r] = int(ov.argmax()), ov.max()
    return arg, best


def _roi_pairs(rows, fg, gt_boxes, num_gt, num_classes):
    rows = np.asarray(rows, F32)
    arg, _ = roi_assignment(rows, gt_boxes, num_gt)
    img = np.clip(rows[:, 0].astype(np.int64), 0, len(num_gt) - 1)
    g = np.asarray(gt_boxes, F32)[img, np.maximum(arg, 0)]                                  # [R, 5]
    cls = g[:, 4].astype(np.int64)
    live = np.asarray(fg, bool) & (arg >= 0) & (g[:, 4] > 0) & (cls < num_classes)
    return rows, g, cls, live


def roi_targets_statement(rows, fg, gt_boxes, num_gt, num_classes, norm=None):
    """bbox_targets [R, 4 * num_classes] f32 of returned rows; fg [R] bool marks the rows sampled as foreground.  All
    f32: ew = (b2 - b0) + 1, ecx = b0 + 0.5 ew, the same of the gt; t0 = (gcx - ecx) / ew, t2 = f32(log(f64(gw / ew)));
    with norm = (means, stds) each f32((f64(t) - mean) / std).  Placed at 4 * cls of the row, zeros elsewhere; a row
    that is not foreground, or whose gt has class 0 or a class >= num_classes, is all zeros.
    A proposal that coincides with its gt gives gcx - ecx = +0.0 and log(1.0) = +0.0: t is +0.0, sign included."""
    rows, g, cls, live = _roi_pairs(rows, fg, gt_boxes, num_gt, num_classes)
    R = rows.shape[0]
    half, one = F32(0.5), F32(1.0)
    t = np.zeros((R, 4), F32)
    with np.errstate(all="ignore"):
        for a in (0, 1):
            es = (rows[:, 3 + a] - rows[:, 1 + a]) + one
            ecn = rows[:, 1 + a] + half * es
            gs = (g[:, 2 + a] - g[:, a]) + one
            gc = g[:, a] + half * gs
            q = gs / es
            assert q.dtype == F32 and gc.dtype == F32
            t[:, a] = (gc - ecn) / es
            t[:, a + 2] = np.log(q.astype(F64)).astype(F32)
        if norm is not None:
            mean, std = np.asarray(norm[0], F64), np.asarray(norm[1], F64)
            t = ((t.astype(F64) - mean[None]) / std[None]).astype(F32)
    out = np.zeros((R, 4 * num_classes), F32)
    for r in np.nonzero(live)[0]:
        out[r, 4 * cls[r]:4 * cls[r] + 4] = t[r]
    return out


def roi_targets_evaluate_f64(rows, fg, gt_boxes, num_gt, num_classes, norm=None):
    """(targets [R, 4 * num_classes] f64, bound, log_args [R, 2] f64; NaN on rows without targets).

    Both sides are f32 now, so the proposal's size and centre carry roundings too:
        ew  = (b2 - b0) + 1       eew = U |b2 - b0| + U |ew|               (the same for gw: egw)
        ecx = b0 + 0.5 ew         eec = 0.5 eew + U |ecx|                  (the same for gcx: egc)
        n   = gcx - ecx           en  = egc + eec + U |n|
        t0  = n / ew              e0  = en / ew + |t0| eew / ew + U |t0|
        q   = gw / ew             eq  = egw / ew + q eew / ew + U q
        t2  = fl32(log(q))        e2  = eq / q + U |t2|
    With normalisation t' = fl32((t - mean) / std): e' = e / std + U |t'| (the two f64 operations add < 2^-52 relative).
    Second-order terms: the factor 1.001.  log_args are the f64 values of the statement's f32 quotients gw / ew."""
    rows, g32, cls, live = _roi_pairs(rows, fg, gt_boxes, num_gt, num_classes)
    R = rows.shape[0]
    b, g = rows.astype(F64), g32.astype(F64)
    t, e = np.zeros((R, 4)), np.zeros((R, 4))
    largs = np.full((R, 2), np.nan)
    with np.errstate(all="ignore"):
        for a in (0, 1):
            de, dg = b[:, 3 + a] - b[:, 1 + a], g[:, 2 + a] - g[:, a]
            es, gs = de + 1.0, dg + 1.0
            ees, egs = U * np.abs(de) + U * np.abs(es), U * np.abs(dg) + U * np.abs(gs)
            ecn, gc = b[:, 1 + a] + 0.5 * es, g[:, a] + 0.5 * gs
            eec, egc = 0.5 * ees + U * np.abs(ecn), 0.5 * egs + U * np.abs(gc)
            n = gc - ecn
            en = egc + eec + U * np.abs(n)
            t0 = n / es
            q = gs / es
            eq = egs / np.abs(es) + np.abs(q) * ees / np.abs(es) + U * np.abs(q)
            t2 = np.log(q)
            t[:, a], e[:, a] = t0, en / np.abs(es) + np.abs(t0) * ees / np.abs(es) + U * np.abs(t0)
            t[:, a + 2], e[:, a + 2] = t2, eq / np.abs(q) + U * np.abs(t2)
            q32 = ((g32[:, 2 + a] - g32[:, a]) + F32(1.0)) / ((rows[:, 3 + a] - rows[:, 1 + a]) + F32(1.0))
            largs[:, a] = np.where(live, q32.astype(F64), np.nan)
        if norm is not None:
            mean, std = np.asarray(norm[0], F64), np.asarray(norm[1], F64)
            t = (t - mean[None]) / std[None]
            e = e / np.abs(std[None]) + U * np.abs(t)
    out, bound = np.zeros((R, 4 * num_classes)), np.zeros((R, 4 * num_classes))
    for r in np.nonzero(live)[0]:
        out[r, 4 * cls[r]:4 * cls[r] + 4] = t[r]
        bound[r, 4 * cls[r]:4 * cls[r] + 4] = 1.001 * e[r]
    return out, bound, largs


# ------------------------------------------------------------------------------------------------ the cases ---
# A builder that meets a value which fails its guard redraws that value; nothing is ever left out of a comparison.
# Every case records how many values it redrew ("redrawn") and how many it excludes ("excluded": always 0).

def _ordered(f):
    """the f32 value as an integer that orders like the value"""
    i = int(np.array(f, F32).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _unordered(o):
    return np.array(o if o >= 0 else ((-o) | 0x80000000), np.uint32).view(F32)[()]


def _one_anchor(anc32, a_idx, d, info_row, min_size):
    """the statement on one anchor of one image: (bw, bh, ms, valid) -- through _decode_axis, the arithmetic of
    proposal_statement itself"""
    one = F32(1.0)
    res = []
    with np.errstate(all="ignore"):
        for a in (0, 1):
            _, _, lo, hi = _decode_axis(anc32[a_idx, a], anc32[a_idx, a + 2], d[a], np.array(d[a + 2], F32), info_row[1 - a] - one)
            res.append((hi - lo) + one)
    ms = F32(min_size) * info_row[2]
    return res[0], res[1], ms, bool(res[0] >= ms and res[1] >= ms)


def _find_edge(anc32, a_idx, d, info_row, axis, min_size=16.0):
    """the smallest f32 size delta (column 2 + axis of d) at which the anchor passes the filter, by bisection over the
    ordered f32 values (every operation of the statement is monotone in it); None when [-8, 8] does not bracket it"""
    d = np.array(d, F32)

    def valid(o):
        d[2 + axis] = _unordered(o)
        return _one_anchor(anc32, a_idx, d, info_row, min_size)[3]
    lo, hi = _ordered(F32(-8.0)), _ordered(F32(8.0))
    if valid(lo) or not valid(hi):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if valid(mid):
            hi = mid
        else:
            lo = mid
    return hi                                                          # ordered integer of the smallest valid delta


EDGE_KINDS = ("at", "below", "above")


def _plant_edges(rs, pred, info, H, W, taken, want=9, min_size=16.0):
    """Filter-edge anchors, found on the host through the statement: for anchors spread over three places of every
    image -- its interior, its origin (the left / upper corner clipped to 0) and its right / lower border, where the
    box reaches the filter's edge only AFTER the clip -- the centre delta puts the box there, the other axis keeps the
    anchor's own size, and a bisection finds d*, the smallest f32 size delta that passes the filter.  Kinds:
        'at'    the delta is d* and bw == ms exactly (kept)
        'above' the delta is the smallest one with bw > ms (kept; one nextafter step of the delta down and bw <= ms)
        'below' the delta is nextafter(d*, -inf) (dropped; one step up and it is kept)
    A d* whose exp is unsafe is not used: the centre is redrawn.  Returns a list of dicts (image, anchor, axis, kind,
    place) and the number of redraws; writes the deltas into pred [N, M, 4]."""
    N, M = pred.shape[:2]
    anc32 = shifted_anchors(H, W).astype(F32)
    edges, redrawn = [], 0
    for n in range(N):
        im = (float(info[n, 1]), float(info[n, 0]))                    # (w, h)
        ms = float(F32(min_size) * info[n, 2])
        found = {k: 0 for k in EDGE_KINDS}
        n_found, tries = 0, 0
        places = ("interior", "origin", "border")
        while (n_found < want or min(found.values()) < 2) and tries < 600:
            place = places[tries % 3]
            axis = (tries // 3) % 2
            tries += 1
            i = int(rs.randint(M))
            if (n, i) in taken:
                continue
            aw = float(anc32[i, 2 + axis] - anc32[i, axis] + 1)
            ao = float(anc32[i, 3 - axis] - anc32[i, 1 - axis] + 1)
            c = float(anc32[i, axis]) + 0.5 * aw
            co = float(anc32[i, 1 - axis]) + 0.5 * ao
            if not (0.25 * im[1 - axis] < co < 0.75 * im[1 - axis]):   # the other axis: the anchor's own span, which
                continue                                               # must keep more than ms + 1 inside the image
            if place == "interior":
                target = rs.uniform(2.0 * ms, im[axis] - 2.0 * ms)
            elif place == "origin":
                target = rs.uniform(0.05, 0.4) * ms                    # the centre near 0: x1 is clipped to 0
            else:
                target = im[axis] - 1.0 + rs.uniform(0.2, 1.5) * ms    # the centre past the border: x2 is clipped
            d = np.zeros(4, F32)
            d[axis] = F32((target - c) / aw)
            o = _find_edge(anc32, i, d, info[n], axis, min_size)
            if o is None:
                continue
            d[2 + axis] = _unordered(o)
            b = _one_anchor(anc32, i, d, info[n], min_size)
            if b[1 - axis] < b[2] + F32(1.0):
                continue
            kind = min(EDGE_KINDS, key=lambda k: found[k])             # the kind this image has fewest of
            if kind == "at" and b[axis] != b[2]:
                kind = "above" if found["above"] <= found["below"] else "below"
            if kind == "below":
                d[2 + axis] = _unordered(o - 1)
            elif kind == "above":
                while b[axis] == b[2]:                                 # from 'at' up to the first delta with bw > ms
                    o += 1
                    d[2 + axis] = _unordered(o)
                    b = _one_anchor(anc32, i, d, info[n], min_size)
            if not bool(exp_is_safe(d[2:4]).all()):
                redrawn += 1
                continue
            pred[n, i] = d
            taken.add((n, i))
            found[kind] += 1
            n_found += 1
            edges.append(dict(image=n, anchor=i, axis=axis, kind=kind, place=place))
    return edges, redrawn


def _distinct_logits(rs, N, H, W, A):
    """scores [N, H, W, 2A] f32 whose fused-softmax outputs are pairwise distinct within an image and whose softmax
    arguments are all exp-safe: offending pairs are redrawn"""
    x = rs.normal(0.0, 1.5, (N, H, W, 2 * A)).astype(F32)
    redrawn = 0
    for _ in range(200):
        s = proposal_scores(x, A, True)
        t0, t1 = softmax_arguments(x, A)
        bad = ~(exp_is_safe(t0) & exp_is_safe(t1))
        for n in range(N):
            _, first = np.unique(s[n], return_index=True)
            dup = np.ones(s.shape[1], bool)
            dup[first] = False
            bad[n] |= dup
        if not bad.any():
            return x, redrawn
        redrawn += int(bad.sum())
        m = bad.reshape(N, H, W, A)
        fresh = rs.normal(0.0, 1.5, (N, H, W, 2 * A)).astype(F32)
        x[..., :A] = np.where(m, fresh[..., :A], x[..., :A])
        x[..., A:] = np.where(m, fresh[..., A:], x[..., A:])
    raise AssertionError("no distinct, safe scores after 200 rounds")


def _rank_first(x, A, edges, from_logits):
    """Give the filter-edge anchors of every image that image's highest scores, by exchanging their (bg, fg) channel
    pairs with those of the anchors that held them: the k edge anchors of an image then hold its k largest scores (the
    multiset of scores, their distinctness and every softmax argument stay what they were).  Whether the layer kept an
    anchor shows only in sorted_index, so an anchor is decided only where it would rank inside the pre-NMS cut: at the
    head of the order every one of them is, whatever the cut, and the kept ones reach the NMS and the rois as well."""
    N, H, W = x.shape[:3]
    for n in range(N):
        mine = [e["anchor"] for e in edges if e["image"] == n]
        bg, fg = x[n, :, :, :A].reshape(-1).copy(), x[n, :, :, A:].reshape(-1).copy()
        s = proposal_scores(x[n:n + 1], A, from_logits)[0].astype(F64)
        holder = np.argsort(-s, kind="stable")[:len(mine)]             # holder[j]: the anchor with the j-th largest score
        for j, e in enumerate(mine):
            t = int(holder[j])
            if t != e:
                for ch in (bg, fg):
                    ch[e], ch[t] = ch[t], ch[e]
                holder[holder == e] = t                                # (e held a later one of the largest: t holds it now)
                holder[j] = e
        x[n, :, :, :A], x[n, :, :, A:] = bg.reshape(H, W, A), fg.reshape(H, W, A)


def _proposal_case(name, seed, N, H, W, im_info, topn=None, n_overflow=6, edges=True):
    rs = np.random.RandomState(seed)
    A, M = 9, H * W * 9
    info = np.asarray(im_info, F32)
    prob = np.zeros((N, H, W, 2 * A), F32)
    for n in range(N):
        fg = ((rs.permutation(M) + 1).astype(F32) / F32(M + 1)).reshape(H, W, A)             # pairwise distinct
        prob[n, :, :, A:] = fg
        prob[n, :, :, :A] = F32(1.0) - fg
    logits, redrawn = _distinct_logits(rs, N, H, W, A)
    pred = np.empty((N, M, 4), F32)
    pred[:, :, 0:2] = rs.normal(0.0, 0.5, (N, M, 2))
    pred[:, :, 2:4] = rs.uniform(-4.0, 4.0, (N, M, 2))
    taken = set()
    for n in range(N):                                                 # exp overflows f32 to inf (exp(88.73) > f32 max)
        for k in range(min(n_overflow, M)):
            i = int(rs.randint(M))
            taken.add((n, i))
            pred[n, i, 2 + k % 2] = F32(rs.uniform(89.0, 120.0))
            if k % 3 == 2:
                pred[n, i, 2:4] = rs.uniform(89.0, 120.0, 2)
    edge_list = []
    if edges:
        edge_list, r = _plant_edges(rs, pred, info, H, W, taken)
        redrawn += r
        _rank_first(prob, A, edge_list, False)
        _rank_first(logits, A, edge_list, True)
    sizes = pred[:, :, 2:4]                                            # (a view: the redraws land in pred)
    big = sizes > 80.0
    for mask, draw in ((~big, lambda r, k: r.uniform(-4.0, 4.0, k)), (big, lambda r, k: r.uniform(89.0, 120.0, k))):
        while True:
            bad = mask & ~exp_is_safe(sizes)
            for e in edge_list:                                        # (the planted deltas were checked when planted)
                bad[e["image"], e["anchor"]] = False
            if not bad.any():
                break
            redrawn += int(bad.sum())
            sizes[bad] = draw(rs, int(bad.sum())).astype(F32)
    return dict(name=name, N=N, H=H, W=W, A=A, M=M, prob=prob, logits=logits, pred=pred.reshape(N, H, W, 4 * A),
                im_info=info, topn=topn, edges=edge_list, redrawn=redrawn, excluded=0)


def proposal_one_cell():
    """N = 1, a 1 x 1 map: M = 9, the smallest launch (no filter-edge anchors: nine anchors, all larger than the image).
    The layer decodes it in proposal_decode_kernel whatever topk_sort says: the sorted runs of the other kernel live
    in the suppression matrix, 8 * N * topn * 16 bytes here, and one run of one image needs 16384 -- with N = 1 that
    is M >= 128 (see proposal_small_run)."""
    return _proposal_case("one_cell", 8101, 1, 1, 1, [(40.0, 52.0, 1.0, 1.0)], n_overflow=2, edges=False)


def proposal_small_run():
    """N = 1, a 4 x 4 map: M = 144, a small launch that does reach proposal_decode_runs_kernel (one block, one run with
    144 live keys of 2048); no filter-edge anchors are asked of a case below M = 315"""
    return _proposal_case("small_run", 8104, 1, 4, 4, [(61.0, 59.0, 1.0, 1.0)], n_overflow=4, edges=False)


def proposal_below_one_run():
    """N = 2, a 5 x 7 map: M = 315, less than one sort run of 2048"""
    return _proposal_case("below_one_run", 8102, 2, 5, 7, [(75.0, 107.0, 1.0, 1.0), (77.0, 110.0, 0.6, 2.0)])


def proposal_over_one_run():
    """N = 3, a 16 x 15 map: M = 2160, a second run with 112 live keys; per-image im_info of scales 1.0, 0.6 and
    1.7777778 and image sizes that are no multiples of 16; its TRAIN runs have pre_nms_topN = 500, post_nms_topN = 40,
    so that the top-N cut falls inside the candidates, its TEST runs the defaults, which cut nothing: there the order
    of all the valid keys of both runs is compared"""
    return _proposal_case("over_one_run", 8103, 3, 16, 15,
                          [(250.0, 237.0, 1.0, 1.0), (243.0, 229.0, 0.6, 2.0), (254.0, 235.0, 1.7777778, 0.0)], topn=(500, 40))


def _gt_array(rows, max_gt=20):
    g = np.zeros((max_gt, 5), F32)
    g[:len(rows)] = np.asarray(rows, F32)
    return g


def _anchor_case(name, seed, H, W, scales, dataset, n_images, n_out, infos, gts, special=None):
    """gts: per supervised image a list of (x1, y1, x2, y2, cls) rows.  A gt box that leaves an unsafe logarithm for any
    inside anchor is redrawn (its corners jittered) until every logarithm the statement takes is safe.  special: the
    row indices (thin, big, dup) of the 1-px-wide gt, the gt larger than the image and the copy of row 0 in every
    supervised image; a jitter would undo 'thin' and 'dup', so the CPU test checks that these rows still are what
    they are called and which of them are some inside anchor's arg-max."""
    rs = np.random.RandomState(seed)
    gt = np.stack([_gt_array(g) for g in gts] + [np.zeros((20, 5), F32)] * (n_out - n_images))
    ng = np.array([len(g) for g in gts] + [0] * (n_out - n_images), np.int32)
    info = np.asarray(infos, F32)
    redrawn = 0
    for _ in range(100):
        _, _, largs = anchor_targets_evaluate_f64(gt, ng, info, n_images, n_out, H, W, dataset, STRIDE, scales)
        _, arg = anchor_assignment(gt, ng, info, n_images, H, W, dataset, STRIDE, scales)
        bad = ~np.isnan(largs) & ~log_is_safe(np.where(np.isnan(largs), 1.0, largs))
        if not bad.any():
            break
        for n, m in zip(*np.nonzero(bad.any(2))):
            gt[n, arg[n, m], :4] += rs.uniform(-0.5, 0.5, 4).astype(F32)
            redrawn += 1
    else:
        raise AssertionError("no safe ground truth after 100 rounds")
    return dict(name=name, H=H, W=W, scales=tuple(scales), dataset=dataset, n_images=n_images, n_out=n_out, gt_boxes=gt,
                num_gt=ng, im_info=info, seed=seed, redrawn=redrawn, excluded=0, special=special)


def _rand_gt(rs, n, w, h, cls):
    x1, y1 = rs.uniform(0, 0.6 * w, n), rs.uniform(0, 0.6 * h, n)
    return [(a, b, a + rs.uniform(10, 0.5 * w), b + rs.uniform(10, 0.5 * h), c) for a, b, c in zip(x1, y1, cls)]


def _anchor_rows(rs, w, h):
    """positives first: random boxes, a 1-px-wide box, a box larger than the image, a duplicated pair; then class-0 rows"""
    pos = _rand_gt(rs, 3, w, h, [1, 2, 1])
    pos.append((0.37 * w, 0.2 * h, 0.37 * w, 0.7 * h, 2))              # x2 == x1: one pixel wide
    pos.append((-20.5, -11.25, w + 30.0, h + 17.5, 1))                 # larger than the image
    pos.append(pos[0][:4] + (2,))                                      # a duplicate of row 0: the first maximum wins
    return pos, _rand_gt(rs, 2, w, h, [0, 0])


def anchor_cases():
    """the anchor-target cases, by name.

    The issue's maps are 1 x 1 (9 anchors, fewer than the 16 of one aligned load of the label recount; N = 2, so that
    image 1's label row starts at byte offset 9), 3 x 4 and 14 x 17, N = 3 joint.  With the workload's anchor scales
    (8, 16, 32) the smallest anchor is 88 x 176 px and starts at (-36, -80): no anchor of a 1 x 1 or 3 x 4 map lies
    inside any image.  The reference's layer raises there (an arg-max over zero inside anchors); the product's layer
    defines it -- anchor_label_kernel gives an outside anchor label -1 and no gt, anchor_targets_kernel then writes
    label -1 and zero targets and weights -- and the '*_outside' cases hold the layer to exactly that.  So that the
    same maps also run WITH targets, the '*_small' cases use anchor_scales (1, 2, 4) on them: 16 .. 64 px anchors, of
    which the 1 x 1 map has exactly one inside its image ((0, 0, 15, 15)).  14 x 17 has inside anchors at (8, 16, 32)."""
    rs = np.random.RandomState(8201)
    out = {}
    # 1 x 1, N = 2
    tiny = [(40.0, 44.0, 1.0, 1.0), (36.0, 41.0, 0.6, 2.0)]
    tiny_gt = [[(1.5, 2.25, 13.0, 17.5, 1), (0.0, 0.0, 15.0, 15.0, 2), (3.0, 3.0, 3.0, 30.0, 1), (5.0, 1.0, 30.0, 9.0, 0)],
               [(-4.0, -7.5, 50.0, 47.0, 2), (2.0, 1.0, 14.5, 12.0, 1), (2.0, 1.0, 14.5, 12.0, 2)]]
    out["1x1_outside"] = _anchor_case("1x1_outside", 8211, 1, 1, SCALES, "SNUBH", 2, 2, tiny, tiny_gt)
    out["1x1_small"] = _anchor_case("1x1_small", 8212, 1, 1, SMALL_SCALES, "SNUBH", 2, 2, tiny, tiny_gt)
    out["1x1_small_fg"] = _anchor_case("1x1_small_fg", 8213, 1, 1, SMALL_SCALES, "SNUBH_FG", 2, 2, tiny, tiny_gt)
    # 3 x 4 and 14 x 17: one supervised image + two weak ones (N = 3 joint), and three supervised ones
    for tag, H, W, scales in (("3x4_small", 3, 4, SMALL_SCALES), ("14x17", 14, 17, SCALES)):
        w, h = W * 16 - 5.0, H * 16 - 3.0
        infos = [(h, w, 1.0, 1.0), (h - 6.0, w - 9.0, 0.6, 2.0), (h - 2.0, w - 1.0, 1.7777778, 0.0)]
        rows = []
        for _ in range(3):
            pos, neg = _anchor_rows(rs, w, h)
            rows.append(pos + neg)
        out[tag + "_joint"] = _anchor_case(tag + "_joint", 8220 + H, H, W, scales, "SNUBH", 1, 3, infos, rows[:1], (3, 4, 5))
        out[tag + "_fg"] = _anchor_case(tag + "_fg", 8230 + H, H, W, scales, "SNUBH_FG", 3, 3, infos, rows, (3, 4, 5))
        mixed = [r[:2] + r[-1:] + r[2:-1] for r in rows]               # a class-0 row among the positives: every row counts
        out[tag + "_all"] = _anchor_case(tag + "_all", 8240 + H, H, W, scales, "ALL", 3, 3, infos, mixed, (4, 5, 6))
        if H == 14:
            # next to the larger-than-image gt the 1-px-wide row is no inside anchor's arg-max (the CPU test says so);
            # alone among the admitted rows it is every inside anchor's: gw = 1 against ew >= 88
            thin = [rows[0][3], rows[0][-1]]
            out[tag + "_thin"] = _anchor_case(tag + "_thin", 8260, H, W, scales, "SNUBH", 1, 1, infos[:1], [thin])
    out["3x4_outside"] = _anchor_case("3x4_outside", 8250, 3, 4, SCALES, "SNUBH", 1, 3,
                                      out["3x4_small_joint"]["im_info"], [[tuple(r) for r in out["3x4_small_joint"]["gt_boxes"][0, :8]]])
    return out


ROI_NORM = ((0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2))                # the means and stds of proposal_target_norm.npz
ROI_INSIDE_W = (0.1, 0.0, 2.0, -0.5)                                   # a zero and a negative entry


def _jitter(rs, box, rel):
    x1, y1, x2, y2 = box
    w, h = x2 - x1 + 1, y2 - y1 + 1
    return (x1 + rs.uniform(-rel, rel) * w, y1 + rs.uniform(-rel, rel) * h, x2 + rs.uniform(-rel, rel) * w, y2 + rs.uniform(-rel, rel) * h)


def _roi_case(name, seed, R, n_images, train, cfg):
    """R returned rows over n_images images, K = 3.  BATCH_SIZE is 4096 and the bands [FG_THRESH, 1] and [0, BG_THRESH_HI)
    cover every candidate, so the layer returns every candidate: the proposals and (train) the appended positive gt
    rows, which coincide with their gt.  The proposals: jittered copies of the positives (foreground), copies that
    coincide with a positive, random boxes (mostly background), and -- where FG_THRESH is lowered to 0.05 -- boxes of
    an eighth and of eight times a gt's width at the same centre.  A proposal that leaves an unsafe logarithm is redrawn."""
    rs = np.random.RandomState(seed)
    w, h = 400.0, 300.0
    gts = []
    for i in range(n_images):
        pos = _rand_gt(rs, 2 + i % 2, w, h, [1, 2, 1][:2 + i % 2])
        gts.append(pos + _rand_gt(rs, 1, w, h, [0]))
    gt = np.stack([_gt_array(g) for g in gts])
    ng = np.array([len(g) for g in gts], np.int32)
    n_pos = [len(g) - 1 for g in gts]
    n_in = R - (sum(n_pos) if train else 0)
    assert n_in >= 1
    wide = cfg.get("FG_THRESH", 0.5) < 0.1

    def draw(i, kind):
        g = gts[i][int(rs.randint(n_pos[i]))][:4]
        if kind == 0:
            return g                                                   # coincides with its gt
        if kind == 1:
            return _jitter(rs, g, 0.12)
        if kind == 2 and wide:
            cx, cy, gw, gh = 0.5 * (g[0] + g[2]), 0.5 * (g[1] + g[3]), g[2] - g[0] + 1, g[3] - g[1] + 1
            f = (0.125, 8.0)[int(rs.randint(2))]                       # gw / ew = 8 and 1 / 8, gh / eh the other way
            return (cx - 0.5 * gw * f, cy - 0.25 * gh / f ** 0.34, cx + 0.5 * gw * f, cy + 0.25 * gh / f ** 0.34)
        x1, y1 = rs.uniform(0, w - 40), rs.uniform(0, h - 40)
        return (x1, y1, x1 + rs.uniform(12, 200), y1 + rs.uniform(12, 150))
    rows = np.zeros((n_in, 5), F32)
    kinds = np.zeros(n_in, np.int64)
    for r in range(n_in):
        i = r * n_images // n_in                                       # grouped by image, ascending
        kinds[r] = 0 if r == 0 else int(rs.randint(4))
        rows[r] = (i,) + tuple(draw(i, kinds[r]))
    redrawn = 0
    for _ in range(100):
        arg, best = roi_assignment(rows, gt, ng)
        fg = best >= cfg.get("FG_THRESH", 0.5)
        _, _, largs = roi_targets_evaluate_f64(rows, fg, gt, ng, 3)
        bad = (~np.isnan(largs) & ~log_is_safe(np.where(np.isnan(largs), 1.0, largs))).any(1)
        if not bad.any():
            break
        for r in np.nonzero(bad)[0]:
            rows[r, 1:] = draw(int(rows[r, 0]), 1)
            redrawn += 1
    else:
        raise AssertionError("no safe proposals after 100 rounds")
    return dict(name=name, R=R, K=3, n_images=n_images, train=train, rois=rows, gt_boxes=gt, num_gt=ng, cfg=dict(cfg),
                seed=seed, redrawn=redrawn, excluded=0)


def roi_cases():
    """R in {1, 70, 257} returned rows (257: one past a 256-thread block) over 1, 2 and 3 images"""
    base = dict(BATCH_SIZE=4096, BBOX_INSIDE_WEIGHTS=ROI_INSIDE_W)
    return {"r1": _roi_case("r1", 8301, 1, 1, False, base),
            "r70": _roi_case("r70", 8302, 70, 2, True, dict(base, FG_THRESH=0.05, BG_THRESH_HI=0.05)),
            "r257": _roi_case("r257", 8303, 257, 3, True, base)}


PROPOSAL_BUILDERS = {"one_cell": proposal_one_cell, "small_run": proposal_small_run, "below_one_run": proposal_below_one_run,
                     "over_one_run": proposal_over_one_run}
PROPOSAL_CASES = tuple(PROPOSAL_BUILDERS)
EDGED_CASES = ("below_one_run", "over_one_run")                        # M >= 315: these carry filter-edge anchors
ANCHOR_CASES = ("1x1_outside", "1x1_small", "1x1_small_fg", "3x4_outside", "3x4_small_joint", "3x4_small_fg", "3x4_small_all",
                "14x17_joint", "14x17_fg", "14x17_all", "14x17_thin")
ROI_CASES = ("r1", "r70", "r257")
_built = {}


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def proposal_case(name):
    """the case, built once and shared (nobody writes into it)"""
    if ("p", name) not in _built:
        _built[("p", name)] = _frozen(PROPOSAL_BUILDERS[name]())
    return _built[("p", name)]


def anchor_case(name):
    if "anchor" not in _built:
        _built["anchor"] = {k: _frozen(v) for k, v in anchor_cases().items()}
    return _built["anchor"][name]


def roi_case(name):
    if "roi" not in _built:
        _built["roi"] = {k: _frozen(v) for k, v in roi_cases().items()}
    return _built["roi"][name]


_stated = {}


def proposal_stated(name, from_logits):
    """the statement of a proposal case, computed once and shared"""
    key = (name, bool(from_logits))
    if key not in _stated:
        c = proposal_case(name)
        st = proposal_statement(c["logits"] if from_logits else c["prob"], c["pred"], c["im_info"], from_logits=from_logits)
        _stated[key] = _frozen(st)
    return _stated[key]
