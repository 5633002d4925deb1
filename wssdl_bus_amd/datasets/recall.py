"""RPN proposal recall (reference code/lib/datasets/imdb.py:125-213, evaluate_recall): the greedy matching of
candidate boxes to ground-truth boxes, recall per IoU threshold and average recall, per object-area range and per
proposal budget (`limit`).

    pack_recall_gt(roidb)                         the ground truth the matching sees, packed once
    evaluate_recall_table(candidates, gt, ...)    every (area, limit) cell of the table from ONE device op
    evaluate_recall_host(candidates, gt, ...)     the same semantics in NumPy

evaluate_recall_table goes through the C ABI (wssdl_proposal_recall, csrc/proposal_recall.hip): the f64 IoU matrix
of every image is computed once, every cell masks its columns (area) and cuts its rows (limit).  The reference
recomputes everything per cell.  evaluate_recall_host is this module's own restatement of the reference's loop for
machines without a GPU and for the tests; it is not a fallback of the device op, which raises when it cannot run.

Both return {(area, limit): cell} with
    ar            recalls.mean()
    recalls       hits / float(num_pos) per threshold (nan for a cell without positives, like the reference)
    thresholds    np.arange(0.5, 0.95 + 1e-5, 0.05) unless given
    gt_overlaps   np.sort of the recorded overlaps
    num_pos       valid ground-truth boxes over ALL images (images without boxes included)
    hits          recorded overlaps >= threshold, per threshold
    matches       (return_matches) dict(image, gt, box, overlap): one row per round, images ascending, rounds in the
                  reference's order; `gt` indexes the image's packed ground-truth rows, `box` the image's candidates.
Where the reference's assert(gt_ovr >= 0) fires -- an image with fewer usable boxes than valid ground-truth boxes --
both raise AssertionError and name the image."""
import ctypes

import numpy as np

AREAS = {'all': 0, 'small': 1, 'medium': 2, 'large': 3, '96-128': 4, '128-256': 5, '256-512': 6, '512-inf': 7}
AREA_RANGES = [[0 ** 2, 1e5 ** 2],      # all
               [0 ** 2, 32 ** 2],       # small
               [32 ** 2, 96 ** 2],      # medium
               [96 ** 2, 1e5 ** 2],     # large
               [96 ** 2, 128 ** 2],     # 96-128
               [128 ** 2, 256 ** 2],    # 128-256
               [256 ** 2, 512 ** 2],    # 256-512
               [512 ** 2, 1e5 ** 2]]    # 512-inf
ALL_EIGHT = tuple(sorted(AREAS, key=AREAS.get))


def default_thresholds():
    return np.arange(0.5, 0.95 + 1e-5, 0.05)                 # imdb.py:204-205


def _area_range(area):
    assert area in AREAS, 'unknown area range: {}'.format(area)      # imdb.py:149
    return AREA_RANGES[AREAS[area]]


def pack_recall_gt(roidb):
    """imdb.py:156-160 for every entry: the boxes with gt_classes > 0 and max gt_overlaps == 1 (no crowd boxes) and
    their seg_areas.  Returns dict(boxes [G,4] f64, areas [G] f64, offsets [n_images+1] i32).  An entry without
    'seg_areas' -- the flipped twins of append_flipped_images -- raises KeyError, as the reference does."""
    boxes, areas, offsets = [], [], [0]
    for entry in roidb:
        ov = entry['gt_overlaps']
        ov = ov.toarray() if hasattr(ov, 'toarray') else np.asarray(ov)
        max_gt_overlaps = ov.max(axis=1)
        gt_inds = np.where((np.asarray(entry['gt_classes']) > 0) & (max_gt_overlaps == 1))[0]
        b = np.asarray(entry['boxes'])[gt_inds, :]
        a = np.asarray(entry['seg_areas'])[gt_inds]
        boxes.append(b.astype(np.float64).reshape(-1, 4))
        areas.append(a.astype(np.float64).reshape(-1))
        offsets.append(offsets[-1] + len(gt_inds))
    return dict(boxes=np.concatenate(boxes, 0) if boxes else np.zeros((0, 4), np.float64),
                areas=np.concatenate(areas, 0) if areas else np.zeros((0,), np.float64),
                offsets=np.asarray(offsets, np.int32))


def non_gt_boxes(roidb):
    """imdb.py:166-170: the candidates of evaluate_recall(candidate_boxes=None), the roidb's gt_classes == 0 rows."""
    return [np.asarray(e['boxes'])[np.where(np.asarray(e['gt_classes']) == 0)[0], :] for e in roidb]


def _gt(gt):
    if not isinstance(gt, dict):
        gt = pack_recall_gt(gt)
    boxes = np.ascontiguousarray(gt['boxes'], np.float64).reshape(-1, 4)
    areas = np.ascontiguousarray(gt['areas'], np.float64).reshape(-1)
    offsets = np.ascontiguousarray(gt['offsets'], np.int32).reshape(-1)
    if len(offsets) < 1 or offsets[0] != 0 or offsets[-1] != len(boxes) or len(areas) != len(boxes) or (np.diff(offsets) < 0).any():
        raise ValueError("gt: offsets [n_images+1] must start at 0, not decrease and end at len(boxes) == len(areas)")
    return boxes, areas, offsets


def _cells(areas, limits):
    if isinstance(areas, str):
        areas = (areas,)
    areas, limits = list(areas), list(limits)
    if not areas or not limits:
        raise ValueError("at least one area and one limit")
    ranges = np.array([_area_range(a) for a in areas], np.float64).reshape(-1, 2)
    lim = np.array([0 if l is None else int(l) for l in limits], np.int32)
    return areas, limits, ranges, lim


def overlaps_host(boxes, query):
    """utils/bbox.pyx:15-55 in NumPy, f64, the same operations in the same order (each rounded on its own), so the
    values are those of the Cython kernel bit for bit: [n, k]."""
    b = np.asarray(boxes, np.float64).reshape(-1, 1, 4)
    q = np.asarray(query, np.float64).reshape(1, -1, 4)
    qarea = (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1)
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + 1
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + 1
    with np.errstate(all='ignore'):
        ua = (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1) + qarea - iw * ih
        ov = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), ov, 0.0)


def _finish(cell_ov, num_pos, hits, thresholds):
    gt_overlaps = np.sort(cell_ov)
    recalls = np.zeros_like(thresholds)
    with np.errstate(all='ignore'):
        for i in range(len(thresholds)):
            recalls[i] = np.int64(hits[i]) / float(num_pos) if num_pos else np.float64(hits[i]) / np.float64(0.0)
    return {'ar': recalls.mean(), 'recalls': recalls, 'thresholds': thresholds, 'gt_overlaps': gt_overlaps,
            'num_pos': int(num_pos), 'hits': np.asarray(hits, np.int64)}


def _no_box_message(image, area, limit, n_boxes, n_gt):
    return ("evaluate_recall: image %d has %d usable box(es) for %d ground-truth box(es) (area '%s', limit %s): "
            "the reference's assert(gt_ovr >= 0)" % (image, n_boxes, n_gt, area, limit))


def evaluate_recall_host(candidates, gt, areas=ALL_EIGHT, limits=(None,), thresholds=None, return_matches=False):
    """evaluate_recall_table's semantics in NumPy: the reference's loop (imdb.py:151-213) per cell.  `candidates` is
    the reference's list of [n_i, 4] arrays, one per image."""
    gt_boxes_all, gt_areas_all, offsets = _gt(gt)
    areas, limits, ranges, lim = _cells(areas, limits)
    thresholds = default_thresholds() if thresholds is None else np.asarray(thresholds, np.float64)
    n_images = len(offsets) - 1
    if len(candidates) != n_images:
        raise ValueError("one candidate array per image: got %d for %d images" % (len(candidates), n_images))
    out = {}
    for ai, area in enumerate(areas):
        lo, hi = ranges[ai]
        for li, limit in enumerate(limits):
            rec_img, rec_gt, rec_box, rec_ov = [], [], [], []
            num_pos = 0
            for i in range(n_images):
                g_areas = gt_areas_all[offsets[i]:offsets[i + 1]]
                valid = np.where((g_areas >= lo) & (g_areas <= hi))[0]
                g_boxes = gt_boxes_all[offsets[i]:offsets[i + 1]][valid, :]
                num_pos += len(valid)
                boxes = np.asarray(candidates[i]).reshape(-1, 4)
                if boxes.shape[0] == 0:
                    continue
                if lim[li] > 0 and boxes.shape[0] > lim[li]:
                    boxes = boxes[:lim[li], :]
                overlaps = overlaps_host(boxes.astype(np.float64), g_boxes)
                for _ in range(g_boxes.shape[0]):
                    argmax_overlaps = overlaps.argmax(axis=0)
                    max_overlaps = overlaps.max(axis=0)
                    gt_ind = max_overlaps.argmax()
                    gt_ovr = max_overlaps.max()
                    assert gt_ovr >= 0, _no_box_message(i, area, limit, boxes.shape[0], g_boxes.shape[0])
                    box_ind = argmax_overlaps[gt_ind]
                    rec_img.append(i), rec_gt.append(valid[gt_ind]), rec_box.append(box_ind), rec_ov.append(overlaps[box_ind, gt_ind])
                    overlaps[box_ind, :] = -1
                    overlaps[:, gt_ind] = -1
            ov = np.asarray(rec_ov, np.float64)
            hits = [(ov >= t).sum() for t in thresholds]
            cell = _finish(ov, num_pos, hits, thresholds)
            if return_matches:
                cell['matches'] = dict(image=np.asarray(rec_img, np.int32), gt=np.asarray(rec_gt, np.int32),
                                       box=np.asarray(rec_box, np.int32), overlap=ov)
            out[(area, limit)] = cell
    return out


def _device_candidates(candidates, n_images):
    """-> (f32 tensor | None, scale tensor | None, f64 tensor | None, pointer of the first coordinate, row stride,
    counts tensor, P)."""
    import torch
    from .. import _lib
    if isinstance(candidates, tuple) and len(candidates) == 3 and isinstance(candidates[0], torch.Tensor):
        rois, counts, scales = candidates
        _lib.require_cuda(rois, counts, scales)
        if rois.dim() != 3 or rois.shape[2] not in (4, 5) or rois.shape[0] != n_images:
            raise ValueError("expected rois_padded [n_images, P, 5 or 4]")
        rois = rois.to(torch.float32).contiguous()
        counts = counts.to(device=rois.device, dtype=torch.int32).contiguous()
        if counts.shape != (n_images,):
            raise ValueError("expected counts [n_images]")
        if scales is not None:
            scales = scales.to(device=rois.device, dtype=torch.float32).contiguous()
            if scales.shape != (n_images,):
                raise ValueError("expected scales [n_images]")
        stride = int(rois.shape[2])
        first = ctypes.c_void_p(rois.data_ptr() + 4 * (stride - 4)) if rois.numel() else None
        return rois, scales, None, first, stride, counts, int(rois.shape[1])
    if len(candidates) != n_images:
        raise ValueError("one candidate array per image: got %d for %d images" % (len(candidates), n_images))
    arrays = [np.asarray(c).reshape(-1, 4).astype(np.float64) for c in candidates]       # boxes.astype(np.float)
    counts = np.array([len(a) for a in arrays], np.int32)
    P = int(counts.max()) if n_images else 0
    padded = np.zeros((n_images, P, 4), np.float64)
    for i, a in enumerate(arrays):
        padded[i, :len(a)] = a
    boxes = torch.from_numpy(padded).cuda()
    return None, None, boxes, (_lib.ptr(boxes) if boxes.numel() else None), 4, torch.from_numpy(counts).cuda(), P


def evaluate_recall_table(candidates, gt, areas=ALL_EIGHT, limits=(None,), thresholds=None, return_matches=False):
    """Every (area, limit) cell of the recall table from one device op (wssdl_proposal_recall).

    candidates   the reference's list of [n_i, 4] arrays (uploaded as f64, boxes.astype(np.float)), or the device
                 triple (rois_padded [N, P, 5] f32, counts [N] i32, scales [N] f32 | None) that
                 rpn_msr.generate.rpn_proposals_batch and im_info[:, 2] give: the op divides by the scale in f32 and
                 widens, which is im_proposals' arithmetic, so nothing is read back or repacked.
    gt           pack_recall_gt(roidb), or the roidb itself.
    areas        names of AREAS; limits: None (or <= 0) for no limit.
    One read-back of the summary (hits, num_pos, flags), one of the overlaps the cells' gt_overlaps are sorted from;
    the (gt, box) columns of the match table are read back only with return_matches."""
    import torch
    from .. import _lib
    gt_boxes, gt_areas, offsets = _gt(gt)
    areas, limits, ranges, lim = _cells(areas, limits)
    thresholds = default_thresholds() if thresholds is None else np.asarray(thresholds, np.float64)
    if thresholds.ndim != 1 or len(thresholds) < 1:
        raise ValueError("at least one threshold")
    N, Gtot, A, Ln, T = len(offsets) - 1, len(gt_boxes), len(areas), len(limits), len(thresholds)
    if N and int(np.diff(offsets).max()) > _lib.RECALL_MAX_GT:
        raise ValueError("more than WSSDL_RECALL_MAX_GT = %d ground-truth boxes in one image" % _lib.RECALL_MAX_GT)
    f32, scales, f64, first, stride, counts, P = _device_candidates(candidates, N)
    if P > _lib.RECALL_MAX_BOXES:
        raise ValueError("more than WSSDL_RECALL_MAX_BOXES = %d candidate rows per image" % _lib.RECALL_MAX_BOXES)
    dev = counts.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_gt, d_ar, d_rng, d_lim, d_thr = up(gt_boxes), up(gt_areas), up(ranges), up(lim), up(thresholds)
        summary = torch.empty((A * Ln * (T + 2),), dtype=torch.int32, device=dev)
        hits, num_pos, flags = summary[:A * Ln * T], summary[A * Ln * T:A * Ln * (T + 1)], summary[A * Ln * (T + 1):]
        m_ov = torch.empty((A * Ln, Gtot), dtype=torch.float64, device=dev)
        m_gt = torch.empty((A * Ln, Gtot), dtype=torch.int32, device=dev) if return_matches else None
        m_box = torch.empty((A * Ln, Gtot), dtype=torch.int32, device=dev) if return_matches else None
        n = L.wssdl_proposal_recall_workspace_bytes(N, P, Gtot)
        ws = torch.empty((max(n, 1),), dtype=torch.uint8, device=dev)
        with _lib.timed("proposal_recall", dict(N=N, P=P, G=Gtot, A=A, L=Ln, T=T)):
            _lib.check(L.wssdl_proposal_recall(first if f32 is not None else None, _lib.ptr(scales),
                                               first if f64 is not None else None, stride, _lib.ptr(counts), N, P,
                                               _lib.ptr(d_gt), _lib.ptr(d_ar), _lib.host_ptr(offsets), Gtot, _lib.ptr(d_rng), A,
                                               _lib.ptr(d_lim), Ln, _lib.ptr(d_thr), T, _lib.ptr(hits), _lib.ptr(num_pos),
                                               _lib.ptr(flags), _lib.ptr(m_gt), _lib.ptr(m_box), _lib.ptr(m_ov), _lib.ptr(ws), n,
                                               _lib.stream()), "wssdl_proposal_recall")
        host = summary.cpu().numpy()                      # the small read-back
    h_hits = host[:A * Ln * T].reshape(A, Ln, T)
    h_pos = host[A * Ln * T:A * Ln * (T + 1)].reshape(A, Ln)
    h_flags = host[A * Ln * (T + 1):].reshape(A, Ln)
    if h_flags.any():
        ai, li = [int(v[0]) for v in np.nonzero(h_flags)]
        c = np.clip(counts.cpu().numpy(), 0, P)
        for i in range(N):
            ar = gt_areas[offsets[i]:offsets[i + 1]]
            nv = int(((ar >= ranges[ai, 0]) & (ar <= ranges[ai, 1])).sum())
            nb = int(min(c[i], lim[li]) if lim[li] > 0 else c[i])
            if 0 < nb < nv:
                raise AssertionError(_no_box_message(i, areas[ai], limits[li], nb, nv))
        raise AssertionError("evaluate_recall: the device op flagged cell (%s, %s)" % (areas[ai], limits[li]))
    ov = m_ov.cpu().numpy().reshape(A, Ln, Gtot)
    if return_matches:
        mg, mb = m_gt.cpu().numpy().reshape(A, Ln, Gtot), m_box.cpu().numpy().reshape(A, Ln, Gtot)
        image_of = np.repeat(np.arange(N, dtype=np.int32), np.diff(offsets))
    out = {}
    for ai, area in enumerate(areas):
        for li, limit in enumerate(limits):
            rec = ov[ai, li] != -1.0                       # (slots the rounds did not fill hold -1)
            cell = _finish(ov[ai, li][rec], h_pos[ai, li], h_hits[ai, li], thresholds)
            if return_matches:
                cell['matches'] = dict(image=image_of[rec], gt=mg[ai, li][rec], box=mb[ai, li][rec], overlap=ov[ai, li][rec])
            out[(area, limit)] = cell
    return out
