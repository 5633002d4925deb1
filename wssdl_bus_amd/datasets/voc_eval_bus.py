"""Detection evaluation: AP, CorLoc and the FROC counts (reference code/lib/datasets/voc_eval_bus.py and the 44
calls of code/lib/datasets/bus.py:_do_python_eval) from detections that stay on the GPU.

    eval_detections(dets, gt, num_classes, ...)      one pass for every class and every score threshold
    DetectionAccumulator                             add() batches of post_detections_batched_device, evaluate() once
    evaluate_detections(all_boxes | accumulator, gt_roidb, classes)      what _do_python_eval reports

GPU tensors go through the C ABI (wssdl_eval_detections, csrc/eval_detect.hip).  CPU tensors / numpy arrays take
the NumPy path below, which restates the same arithmetic and the same tie rule; it is the module's own host path
(small validation sets, machines without a GPU), not a fallback of the device op.

What is evaluated (as_result_file=True) is what the reference wrote to its result file and read back: the score
as '{:.3f}', every coordinate as '{:.1f}' of the f32 value x + 1 (bus.py:257-261) -- rint(double(s) * 1000.0) /
1000.0 and rint(double(x +f32 1.0f) * 10.0) / 10.0 are exactly the parsed doubles -- against ground-truth boxes in
the annotation's 1-based pixel values.  With as_result_file=False the f32 values are used as they are.

Order among equal scores: the reference's np.argsort(-confidence) is an unstable introsort, so its order among
detections of equal confidence -- and every curve value that depends on it -- is an accident of NumPy.  Here equal
scores keep their input order (image index, then rank within the image): a stable sort of the result file's
lines.  With pairwise distinct 3-decimal scores both give the same bits."""
import ctypes

import numpy as np
import torch

from .. import _lib

FROC_THRESHOLDS = np.arange(1.0, -0.01, -0.05)          # bus.py:369


def voc_ap(rec, prec, use_07_metric=False):
    """ap = voc_ap(rec, prec, [use_07_metric]): VOC AP from recall and precision, the 11-point metric of VOC07 or
    the area under the precision envelope.  Same call and same f64 arithmetic as the reference's function."""
    rec = np.asarray(rec, np.float64)
    prec = np.asarray(prec, np.float64)
    if use_07_metric:
        ap = 0.
        for i in range(11):
            above = rec >= i * 0.1
            p = prec[above].max() if above.any() else 0
            ap = ap + p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    envelope = np.maximum.accumulate(np.concatenate(([0.], prec, [0.]))[::-1])[::-1]
    step = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[step + 1] - mrec[step]) * envelope[step + 1])


def pack_gt(gt_roidb):
    """gt_roidb: list over the images of {'boxes' [n,4], 'gt_classes' [n], 'difficult' [n] (optional)} with the
    annotation's pixel values as they stand -> (boxes [G,4] f64, classes [G] i32, difficult [G] u8,
    image_offsets [n_images+1] i32), numpy."""
    boxes, cls, dif, off = [], [], [], [0]
    for r in gt_roidb:
        b = np.asarray(r['boxes'], np.float64).reshape(-1, 4)
        c = np.asarray(r['gt_classes'], np.int32).reshape(-1)
        d = np.asarray(r['difficult'] if r.get('difficult') is not None else np.zeros(len(c)), np.uint8).reshape(-1)
        if not (len(b) == len(c) == len(d)):
            raise ValueError("boxes, gt_classes and difficult of an image differ in length")
        boxes.append(b), cls.append(c), dif.append(d), off.append(off[-1] + len(c))
    return (np.concatenate(boxes, 0) if boxes else np.zeros((0, 4)), np.concatenate(cls) if cls else np.zeros(0, np.int32),
            np.concatenate(dif) if dif else np.zeros(0, np.uint8), np.asarray(off, np.int32))


def _np(x, dtype=None):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a if dtype is None else np.ascontiguousarray(a, dtype)


def _gt_arrays(gt):
    if isinstance(gt, (list, tuple)) and len(gt) == 4 and not isinstance(gt[0], dict):
        b, c, d, o = gt
    else:
        b, c, d, o = pack_gt(gt)
    b, c, d, o = _np(b, np.float64).reshape(-1, 4), _np(c, np.int32).ravel(), _np(d, np.uint8).ravel(), _np(o, np.int32).ravel()
    if len(o) < 1 or not (len(b) == len(c) == len(d)):
        raise ValueError("gt = (boxes [G,4], classes [G], difficult [G], image_offsets [n_images+1])")
    return b, c, d, o


def flatten_batched(dets, counts, first_image=0):
    """(dets [N,K-1,P,5], counts [N,K-1]) -> (boxes, scores, image, class, slot): the live rows in slot order
    ((i * (K-1) + j-1) * P + p, the input index the batched layout reports).  Host arrays."""
    d, n = _np(dets, np.float32), _np(counts, np.int64)
    N, K1, P = d.shape[0], d.shape[1], d.shape[2]
    live = np.arange(P)[None, None, :] < np.minimum(n, P)[:, :, None]
    i, j, p = np.nonzero(live)
    rows = d[i, j, p]
    return (rows[:, :4], rows[:, 4], (i + int(first_image)).astype(np.int32), (j + 1).astype(np.int32),
            ((i * K1 + j) * P + p).astype(np.int64))


def _eval_host(boxes, scores, image, cls, gt, K, ovthresh, thresholds, base, quantise, index=None, n_slots=None):
    """The NumPy path: same outputs as the device op for the flat layout (index: the input index to report in
    `order` for each row, default its position)."""
    gb, gc, gd, goff = gt
    n_images, G = len(goff) - 1, len(gc)
    boxes, scores = np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(scores, np.float32).ravel()
    image, cls = np.asarray(image, np.int64).ravel(), np.asarray(cls, np.int64).ravel()
    D, T = len(scores), len(thresholds)
    index = np.arange(D) if index is None else np.asarray(index, np.int64)
    n_slots = D if n_slots is None else int(n_slots)
    if quantise:
        q = np.rint(scores.astype(np.float64) * 1000.0)
        conf, skey = q / 1000.0, q
        bb = np.rint((boxes + np.float32(1.0)).astype(np.float64) * 10.0) / 10.0
    else:
        conf = scores.astype(np.float64)
        skey, bb = conf, boxes.astype(np.float64)
    valid = (image >= 0) & (image < n_images) & (cls >= 1) & (cls < K)
    gimg = np.repeat(np.arange(n_images), np.diff(goff))
    ovmax, jmax = np.full(D, -np.inf), np.full(D, -1, np.int64)
    # detections and boxes grouped by (image, class): one overlap matrix per group, voc_eval_bus.py:221-236
    vi = np.nonzero(valid)[0]
    if len(vi) and G:
        gkey = np.where((gc >= 1) & (gc < K), gimg * K + gc, -1)       # (boxes of unknown classes match nothing)
        gsort = np.argsort(gkey, kind='stable')
        dkey = image[vi] * K + cls[vi]
        dsort = vi[np.argsort(dkey, kind='stable')]
        ks, starts = np.unique(dkey[np.argsort(dkey, kind='stable')], return_index=True)
        ends = np.append(starts[1:], len(dsort))
        glo, ghi = np.searchsorted(gkey[gsort], ks, 'left'), np.searchsorted(gkey[gsort], ks, 'right')
        for a, b, g0, g1 in zip(starts, ends, glo, ghi):
            if g1 == g0:
                continue
            sel, g = dsort[a:b], gsort[g0:g1]
            B, Gt = bb[sel][:, None, :], gb[g][None, :, :]
            ixmin, iymin = np.maximum(Gt[..., 0], B[..., 0]), np.maximum(Gt[..., 1], B[..., 1])
            ixmax, iymax = np.minimum(Gt[..., 2], B[..., 2]), np.minimum(Gt[..., 3], B[..., 3])
            iw, ih = np.maximum(ixmax - ixmin + 1., 0.), np.maximum(iymax - iymin + 1., 0.)
            inters = iw * ih
            uni = ((B[..., 2] - B[..., 0] + 1.) * (B[..., 3] - B[..., 1] + 1.) +
                   (Gt[..., 2] - Gt[..., 0] + 1.) * (Gt[..., 3] - Gt[..., 1] + 1.) - inters)
            ov = inters / uni
            ovmax[sel], jmax[sel] = ov.max(1), g[ov.argmax(1)]
    hit = ovmax > ovthresh
    out = dict(order=np.full(n_slots, -1, np.int32), class_offsets=np.zeros(K, np.int32), tp=np.zeros(n_slots, np.int32),
               fp=np.zeros(n_slots, np.int32), rec=np.zeros(n_slots), prec=np.zeros(n_slots), ap07=np.zeros(K - 1),
               ap_area=np.zeros(K - 1), npos=np.zeros(K - 1, np.int32), ni=np.zeros(K - 1, np.int32),
               nok=np.zeros((K - 1, T), np.int32), num_all_fps=np.zeros((K - 1, T), np.int32),
               arr_ok=np.zeros((K - 1, n_images), bool), num_fp_per_img=np.zeros((K - 1, n_images), np.int32))
    off = 0
    for c in range(1, K):
        has = np.zeros(n_images, bool)
        has[gimg[gc == c]] = True
        npos = int(np.sum((gc == c) & (gd == 0)))
        out['npos'][c - 1], out['ni'][c - 1] = npos, int(has.sum())
        idx = np.nonzero(valid & (cls == c))[0]
        n = len(idx)
        out['class_offsets'][c] = off + n
        if n == 0:
            out['ap07'][c - 1] = out['ap_area'][c - 1] = -1.0            # the reference's sentinel (empty result file)
            continue
        order = idx[np.argsort(-skey[idx], kind='stable')]            # ties: input order
        h, g, rank = hit[order], jmax[order], np.arange(n)
        first = np.full(max(G, 1), n, np.int64)
        np.minimum.at(first, g[h], rank[h])
        easy = np.zeros(n, bool)
        easy[h] = gd[g[h]] == 0
        is_first = np.zeros(n, bool)
        is_first[h] = first[g[h]] == rank[h]
        tp = np.cumsum(h & easy & is_first)
        fp = np.cumsum(~h | (h & easy & ~is_first))
        with np.errstate(divide='ignore', invalid='ignore'):
            rec = tp.astype(np.float64) / float(npos)
        prec = tp.astype(np.float64) / np.maximum((tp + fp).astype(np.float64), np.finfo(np.float64).eps)
        seg = slice(off, off + n)
        out['order'][seg], out['tp'][seg], out['fp'][seg], out['rec'][seg], out['prec'][seg] = index[order], tp, fp, rec, prec
        out['ap07'][c - 1], out['ap_area'][c - 1] = voc_ap(rec, prec, True), voc_ap(rec, prec, False)
        best = np.full(n_images, -np.inf)
        np.maximum.at(best, image[idx][hit[idx]], conf[idx][hit[idx]])
        miss_conf, miss_img = conf[idx][~hit[idx]], image[idx][~hit[idx]]
        for t, thr in enumerate(thresholds):
            ok = has & (best >= thr)
            out['nok'][c - 1, t] = ok.sum()
            out['num_all_fps'][c - 1, t] = np.sum(miss_conf >= thr)
            if t == base:
                out['arr_ok'][c - 1] = ok
                out['num_fp_per_img'][c - 1] = np.bincount(miss_img[miss_conf >= thr], minlength=n_images)
        off += n
    return out


_BIG = ("order", "tp", "fp", "rec", "prec")


def _eval_device(layout, gt, K, ovthresh, thresholds, base, quantise):
    """One wssdl_eval_detections call.  layout = ('flat', boxes, scores, image, cls) or ('batched', dets, counts,
    first_image), GPU tensors.  The small outputs share one buffer and come back in ONE read-back; order / tp /
    fp / rec / prec stay on the device."""
    gb, gc, gd, goff = gt
    n_images, G, T = len(goff) - 1, len(gc), len(thresholds)
    L = _lib.lib()
    flags = _lib.EVAL_QUANTISE if quantise else 0
    if layout[0] == 'batched':
        dets, counts = layout[1].to(torch.float32).contiguous(), layout[2].to(torch.int32).contiguous()
        dev = dets.device
        N, P = int(dets.shape[0]), int(dets.shape[2])
        if dets.dim() != 4 or dets.shape[1] != K - 1 or dets.shape[3] != 5 or tuple(counts.shape) != (N, K - 1):
            raise ValueError("expected dets [N, K-1, P, 5] and counts [N, K-1] with K = num_classes")
        slots, first_image = N * (K - 1) * P, int(layout[3])
        flags |= _lib.EVAL_BATCHED
        flat = (None, None, None, None)
    else:
        boxes, scores = layout[1].to(torch.float32).contiguous(), layout[2].to(torch.float32).contiguous()
        dev = scores.device
        image, cls = layout[3].to(device=dev, dtype=torch.int32).contiguous(), layout[4].to(device=dev, dtype=torch.int32).contiguous()
        slots = int(scores.numel())
        if tuple(boxes.shape) != (slots, 4) or image.numel() != slots or cls.numel() != slots:
            raise ValueError("expected boxes [D,4], scores [D], image [D], class [D]")
        flat, dets, counts, N, P, first_image = (boxes, scores, image, cls), None, None, 0, 0, 0
    _lib.require_cuda(*(x for x in flat + (dets, counts)))
    with torch.cuda.device(dev):
        g_b, g_c = _lib.to_device(gb, torch.float64, dev), _lib.to_device(gc, torch.int32, dev)
        g_d, g_o = _lib.to_device(gd, torch.uint8, dev), _lib.to_device(goff, torch.int32, dev)
        thr = _lib.to_device(np.asarray(thresholds, np.float64), torch.float64, dev)
        # the small outputs, f64 first, then i32, then u8, in one buffer
        sizes = [("ap07", 8, K - 1), ("ap_area", 8, K - 1), ("class_offsets", 4, K), ("npos", 4, K - 1), ("ni", 4, K - 1),
                 ("nok", 4, (K - 1) * T), ("num_all_fps", 4, (K - 1) * T), ("num_fp_per_img", 4, (K - 1) * n_images),
                 ("arr_ok", 1, (K - 1) * n_images)]
        offs, total = {}, 0
        for name, width, n in sizes:
            offs[name] = (total, width, n)
            total += width * n
        small = torch.zeros((total + 8,), dtype=torch.uint8, device=dev)
        sp = lambda name: ctypes.c_void_p(small.data_ptr() + offs[name][0])
        big = dict(order=torch.empty((slots,), dtype=torch.int32, device=dev), tp=torch.empty((slots,), dtype=torch.int32, device=dev),
                   fp=torch.empty((slots,), dtype=torch.int32, device=dev), rec=torch.empty((slots,), dtype=torch.float64, device=dev),
                   prec=torch.empty((slots,), dtype=torch.float64, device=dev))
        n = L.wssdl_eval_detections_workspace_bytes(slots, G, n_images, K)
        if n == 0:
            raise _lib.HipCallError("wssdl_eval_detections: unsupported sizes (detections %d, classes %d)" % (slots, K))
        ws = torch.empty((n,), dtype=torch.uint8, device=dev)
        _lib.check(L.wssdl_eval_detections(
            flags, _lib.ptr(flat[0]), _lib.ptr(flat[1]), _lib.ptr(flat[2]), _lib.ptr(flat[3]), slots if layout[0] == 'flat' else 0,
            _lib.ptr(dets), _lib.ptr(counts), N, P, first_image, _lib.ptr(g_b), _lib.ptr(g_c), _lib.ptr(g_d), _lib.ptr(g_o), G,
            n_images, K, float(ovthresh), _lib.ptr(thr), T, int(base), _lib.ptr(big["order"]), sp("class_offsets"),
            _lib.ptr(big["tp"]), _lib.ptr(big["fp"]), _lib.ptr(big["rec"]), _lib.ptr(big["prec"]), sp("ap07"), sp("ap_area"),
            sp("npos"), sp("ni"), sp("nok"), sp("num_all_fps"), sp("arr_ok"), sp("num_fp_per_img"), _lib.ptr(ws), n,
            _lib.stream()), "wssdl_eval_detections")
        host = small.cpu().numpy()                      # the one read-back
    out = dict(big)
    kinds = {8: np.float64, 4: np.int32, 1: np.uint8}
    for name, (o, width, n) in offs.items():
        out[name] = host[o:o + width * n].view(kinds[width]).copy()
    for name in ("nok", "num_all_fps"):
        out[name] = out[name].reshape(K - 1, T)
    out["num_fp_per_img"] = out["num_fp_per_img"].reshape(K - 1, n_images)
    out["arr_ok"] = out["arr_ok"].reshape(K - 1, n_images).astype(bool)
    return out


def _finish(out, use_07_metric, thresholds, base):
    out["ap"] = out["ap07"] if use_07_metric else out["ap_area"]
    out["thresholds"], out["base_threshold"] = np.asarray(thresholds, np.float64), int(base)
    return out


def eval_detections(dets, gt, num_classes, ovthresh=0.5, score_thresh=(0.5,), use_07_metric=True, as_result_file=True):
    """voc_eval_bus for every class and every score threshold in one pass.

    dets   flat: (boxes [D,4], scores [D], image [D], class [D]) with classes 1 .. num_classes-1, the detections of
           one class in result-file order (image index, then rank); or batched: (dets [N,K-1,P,5], counts [N,K-1])
           or (dets, counts, first_image), the pair post_detections_batched_device returns.
    gt     (boxes [G,4], classes [G], difficult [G], image_offsets [n_images+1]) (pack_gt) or a gt_roidb list.
    score_thresh   the T thresholds of CorLoc / FROC (`conf >= t`); arr_ok and num_fp_per_img are those of the first.
    Returns a dict: order, tp, fp, rec, prec (per class segment class_offsets[j-1] : class_offsets[j]; device tensors
    for GPU inputs), class_offsets, ap07, ap_area, ap (the metric asked for), npos, ni, nok [K-1,T],
    num_all_fps [K-1,T], arr_ok [K-1,n_images], num_fp_per_img [K-1,n_images] (numpy).  ap = -1 for a class without
    detections.  GPU inputs: one device op and one read-back of the small outputs."""
    K = int(num_classes)
    thresholds = [float(t) for t in np.atleast_1d(np.asarray(score_thresh, np.float64))]
    if K < 2 or len(thresholds) < 1:
        raise ValueError("num_classes >= 2 and at least one score threshold")
    g = _gt_arrays(gt)
    dets = tuple(dets)
    if len(dets) == 4:
        layout = ('flat',) + dets
    elif len(dets) in (2, 3):
        layout = ('batched', dets[0], dets[1], int(dets[2]) if len(dets) == 3 else 0)
    else:
        raise ValueError("dets = (boxes, scores, image, class) or (dets, counts[, first_image])")
    if isinstance(layout[1], torch.Tensor) and layout[1].is_cuda:
        return _finish(_eval_device(layout, g, K, ovthresh, thresholds, 0, as_result_file), use_07_metric, thresholds, 0)
    if layout[0] == 'batched':
        d = _np(layout[1])
        if d.ndim != 4 or d.shape[1] != K - 1 or d.shape[3] != 5:
            raise ValueError("expected dets [N, K-1, P, 5] with K = num_classes")
        b, s, i, c, slot = flatten_batched(layout[1], layout[2], layout[3])
        out = _eval_host(b, s, i, c, g, K, ovthresh, thresholds, 0, as_result_file, index=slot, n_slots=d.shape[0] * d.shape[1] * d.shape[2])
    else:
        out = _eval_host(_np(layout[1]), _np(layout[2]), _np(layout[3]), _np(layout[4]), g, K, ovthresh, thresholds, 0, as_result_file)
    return _finish(out, use_07_metric, thresholds, 0)


class DetectionAccumulator(object):
    """Collects the (dets, counts) batches of post_detections_batched_device where they are (no read-back) and
    evaluates them in one op:

        acc = DetectionAccumulator(num_classes)
        for every batch:  acc.add(dets, counts, first_image)
        result = acc.evaluate(gt_roidb)
    """

    def __init__(self, num_classes):
        self.num_classes = int(num_classes)
        self.batches = []

    def add(self, dets, counts, first_image):
        if dets.dim() != 4 or dets.shape[1] != self.num_classes - 1 or dets.shape[3] != 5 or \
                tuple(counts.shape) != (dets.shape[0], self.num_classes - 1):
            raise ValueError("expected dets [N, K-1, P, 5] and counts [N, K-1] with K = num_classes")
        self.batches.append((dets, counts, int(first_image)))

    def gathered(self, n_images):
        """(dets [n_images, K-1, P, 5], counts [n_images, K-1]) of all batches, on their device (images nobody
        added have no detections; an image flagged with counts[i, 0] = -1 raises at evaluation time only through
        its missing detections -- detect with postprocess_detections_batch when that matters)."""
        K1 = self.num_classes - 1
        if not self.batches:
            return torch.zeros((n_images, K1, 1, 5)), torch.zeros((n_images, K1), dtype=torch.int32)
        dev = self.batches[0][0].device
        P = max(int(d.shape[2]) for d, _, _ in self.batches)
        dets = torch.zeros((n_images, K1, P, 5), dtype=torch.float32, device=dev)
        counts = torch.zeros((n_images, K1), dtype=torch.int32, device=dev)
        for d, c, first in self.batches:
            n = int(d.shape[0])
            if first < 0 or first + n > n_images:
                raise ValueError("batch of images %d .. %d outside the %d images of the ground truth" % (first, first + n - 1, n_images))
            dets[first:first + n, :, :d.shape[2]] = d.to(device=dev, dtype=torch.float32)
            counts[first:first + n] = c.to(device=dev, dtype=torch.int32).clamp_min(0)
        return dets, counts

    def evaluate(self, gt, ovthresh=0.5, score_thresh=(0.5,), use_07_metric=True, as_result_file=True):
        g = _gt_arrays(gt)
        dets, counts = self.gathered(len(g[3]) - 1)
        return eval_detections((dets, counts, 0), g, self.num_classes, ovthresh, score_thresh, use_07_metric, as_result_file)


def _flat_from_all_boxes(all_boxes, K):
    boxes, scores, image, cls = [], [], [], []
    for j in range(1, K):
        for i, d in enumerate(all_boxes[j]):
            if d is None or len(d) == 0:
                continue
            d = _np(d, np.float32).reshape(-1, 5)
            boxes.append(d[:, :4]), scores.append(d[:, 4])
            image.append(np.full(len(d), i, np.int32)), cls.append(np.full(len(d), j, np.int32))
    if not boxes:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(boxes), np.concatenate(scores), np.concatenate(image), np.concatenate(cls)


def evaluate_detections(all_boxes_or_accumulator, gt_roidb, classes, ovthresh=0.5, score_thresh=0.5, use_07_metric=True):
    """What bus.py:_do_python_eval reports, without files, XML or plots.  all_boxes[j][i] = [n,5] detections of class
    j >= 1 in image i (detect_images), or a DetectionAccumulator; gt_roidb as for pack_gt; classes the class names
    with '__background__' first.  Returns a dict:
      aps, mean_ap                 per class (bus.py:332, use_07_metric as there) and their mean
      corloc_list                  nok / ni per class, then sum(nok) / sum(ni) (bus.py:342, :349); NaN where ni == 0
      froc_curve_pts               [all, class 1, class 2, ...] of (num_all_fps / ni, nok / ni) over
                                   np.arange(1.0, -0.01, -0.05); 'all' the mean of the class points (bus.py:368-381)
      all_arr_ok                   the classes' arr_ok, concatenated (bus.py:343): entry k of a class = its k-th image
                                   with a box of the class, 200 entries per class as in the reference (more if needed)
      num_fp_per_img               false positives at score_thresh per image, summed over the classes (bus.py:315-316)
      result                       eval_detections' dict (thresholds: score_thresh first, then the FROC thresholds)."""
    K = len(classes)
    g = _gt_arrays(gt_roidb)
    thresholds = [float(score_thresh)] + [float(t) for t in FROC_THRESHOLDS]
    if isinstance(all_boxes_or_accumulator, DetectionAccumulator):
        r = all_boxes_or_accumulator.evaluate(g, ovthresh, thresholds, use_07_metric)
    else:
        r = eval_detections(_flat_from_all_boxes(all_boxes_or_accumulator, K), g, K, ovthresh, thresholds, use_07_metric)
    ni, nok, fps = r["ni"].astype(np.float64), r["nok"].astype(np.float64), r["num_all_fps"].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        corloc = list(nok[:, 0] / ni) + [np.sum(nok[:, 0]) / np.sum(ni)]
        pts = [[(fps[c, t] / ni[c], nok[c, t] / ni[c]) for t in range(1, len(thresholds))] for c in range(K - 1)]
    mean_pts = [(sum(p[t][0] for p in pts) / (K - 1), sum(p[t][1] for p in pts) / (K - 1)) for t in range(len(thresholds) - 1)]
    gimg = np.repeat(np.arange(len(g[3]) - 1), np.diff(g[3]))
    arr = []
    for c in range(1, K):
        has = np.zeros(len(g[3]) - 1, bool)
        has[gimg[g[1] == c]] = True
        a = np.zeros(max(200, int(has.sum())))
        a[:int(has.sum())] = r["arr_ok"][c - 1][has]
        arr.append(a)
    aps = [float(a) for a in r["ap"]]
    return dict(aps=aps, mean_ap=float(np.mean(aps)), corloc_list=[float(x) for x in corloc], froc_curve_pts=[mean_pts] + pts,
                all_arr_ok=np.concatenate(arr) if arr else np.zeros((0,)), num_fp_per_img=r["num_fp_per_img"].sum(0), result=r)
