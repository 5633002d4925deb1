"""Batched test-time detection: the detection half of test_net (reference code/lib/fast_rcnn/test_bus.py:300-401)
at N images per forward.

The reference detects one image per forward (test_bus.py:208); so does ``test_bus.im_detect``.  Here
get_test_blobs builds the blob of N images, im_detect_batch decodes every RoI with its own image's scale and
bounds, postprocess_detections_batch runs the per-class NMS, the class-agnostic pass (cfg.TEST.CLS_AGNOSTIC_NMS) and
the max_per_image cap of all images as ONE device op (wssdl_post_detections_batched or its _agnostic_ twin) with one
read-back, and detect_images strings them together.  Every image's
detections are bit for bit those of the single-image arithmetic (test_bus.im_detect's decode / clip,
test_bus.postprocess_detections, of which post_detections.postprocess_detections is the form with a device op
under the flag) on that image's rows of the same network outputs.

Test-time augmentation (an addition; cfg.TEST.FLIP_AUG, BBOX_VOTE, BBOX_VOTE_THRESH, all off by default and read at every
call): get_test_blobs(flip_aug=True) adds a mirrored view of every image to the blob, post_detections_views_device
(wssdl_post_detections_views) brings the views' rows into the image's own frame, runs one NMS over them and votes the
surviving boxes, and postprocess_detections_batch(views=, flip_width=) routes to it."""
import numpy as np
import torch

from .bbox_transform import bbox_transform_inv
from .config import cfg
from .post_detections import device_post_detections_fit, postprocess_detections


def get_test_blobs(planes, net_name, flip_aug=None):
    """test_bus.py:28-64 (_get_image_blob) for a list of grey planes of any sizes, one scale
    (cfg.TEST.SCALES[0], cfg.TEST.MAX_SIZE): returns (data [N, Hmax, Wmax, 3] f32, zero-padded like
    im_list_to_blob, and im_info [N, 3] f32 = (h_i, w_i, scale_i) of each resized image), both on the GPU.
    For one image (h, w) are the blob's own dimensions, as in the reference (test_bus.py:176-179).

    flip_aug (None reads cfg.TEST.FLIP_AUG): the blob of 2n images, image 2i = plane i and image 2i+1 = plane i read
    mirrored (prep_im_for_blob(..., flipped=True): no copy of the plane), and a third result flip_width [2n] f32 on the
    GPU: -1 for the plain views, the plane's width for the mirrored ones -- (data, im_info [2n,3], flip_width), the
    source-image order wssdl_post_detections_views takes with views = 2.  Without it the result is the pair above."""
    from ..utils.blob import PIXEL_MEANS, PIXEL_STDS, im_list_to_blob, prep_im_for_blob
    if len(planes) == 0:
        raise ValueError("get_test_blobs needs at least one image")
    if flip_aug is None:
        flip_aug = bool(cfg.TEST.FLIP_AUG)
    ims, info, width = [], [], []
    for g in planes:
        for flipped in ((False, True) if flip_aug else (False,)):
            if flipped:
                im, s = prep_im_for_blob(g, net_name, PIXEL_MEANS, PIXEL_STDS, cfg.TEST.SCALES[0], cfg.TEST.MAX_SIZE,
                                         is_training=False, flipped=True)
            else:
                im, s = prep_im_for_blob(g, net_name, PIXEL_MEANS, PIXEL_STDS, cfg.TEST.SCALES[0], cfg.TEST.MAX_SIZE,
                                         is_training=False)
            ims.append(im)
            info.append((int(im.shape[0]), int(im.shape[1]), s))
            width.append(float(g.shape[1]) if flipped else -1.0)
    data = im_list_to_blob(ims)
    im_info = torch.tensor(info, dtype=torch.float32, device=data.device)
    if not flip_aug:
        return data, im_info
    return data, im_info, torch.tensor(width, dtype=torch.float32, device=data.device)


@torch.no_grad()
def im_detect_batch(net, data, im_info):
    """im_detect for N images in one forward: data [N,H,W,3] NHWC, im_info [N,>=3] (h, w, scale, ...) per
    image.  Returns (scores [R,K], pred_boxes [R,4K], rois [R,5]) for the RoI blob the network fed to RoI
    pooling; row r belongs to image rois[r, 0] and is decoded with that image's scale and clipped to that
    image's bounds.  Under cfg.PADDED_ROIS the blob has dead rows (batch index -1) whose values are
    meaningless, and nothing here reads the device back.

    Image i's rows are bit for bit what im_detect's arithmetic gives on them: its Python-scalar operations
    are restated with per-row tensors that hold the same f32 values --
      rois / scale        (GPU: PyTorch multiplies by the f32 reciprocal of a Python scalar divisor)
                          -> rois * fl32(1 / fl32(scale)) on the GPU, rois / fl32(scale) on the CPU;
      clamp(max=w/scale - 1)  (the bound computed in double, rounded to f32 by clamp)
                          -> minimum with the f32-rounded double bound."""
    was_training = net.training
    net.eval()
    try:
        layers = net(data, im_info, None, None, is_training=False, is_ws=False, test_net=True)
    finally:
        net.train(was_training)
    rois = layers['rpn_rois']
    scores = layers['cls_prob']
    n = int(data.shape[0])
    from .. import _lib
    info = _lib.to_device(im_info, torch.float64, rois.device)       # exact for an f32 or f64 im_info
    if info.dim() != 2 or info.shape[0] != n or info.shape[1] < 3:
        raise ValueError("im_info must be [N, >=3] for N = data.shape[0]")
    img = rois[:, 0].to(torch.int64).clamp_(0, n - 1)                 # dead rows (-1): any image, ignored later
    scale = info[:, 2].to(torch.float32)
    if rois.is_cuda:
        boxes = rois[:, 1:5] * torch.reciprocal(scale)[img].unsqueeze(1)
    else:
        boxes = rois[:, 1:5] / scale[img].unsqueeze(1)
    if cfg.TEST.BBOX_REG:
        pred = bbox_transform_inv(boxes, layers['bbox_pred'])
        # test_bus._clip_boxes with (h / scale, w / scale) per row
        xmax = (info[:, 1] / info[:, 2] - 1.0).to(torch.float32)[img].unsqueeze(1)
        ymax = (info[:, 0] / info[:, 2] - 1.0).to(torch.float32)[img].unsqueeze(1)
        pred[:, 0::4] = pred[:, 0::4].clamp_min(0)
        pred[:, 1::4] = pred[:, 1::4].clamp_min(0)
        pred[:, 2::4] = torch.minimum(pred[:, 2::4], xmax)
        pred[:, 3::4] = torch.minimum(pred[:, 3::4], ymax)
    else:
        pred = boxes.repeat(1, scores.shape[1])
    return scores, pred, rois


def _rows_pitch(max_rows_per_image=None):
    """P of the batched op: max_rows_per_image, default cfg.TEST.RPN_POST_NMS_TOP_N (<= 0: the largest image)."""
    return int(max_rows_per_image if max_rows_per_image is not None else cfg.TEST.RPN_POST_NMS_TOP_N)


def _device_post_detections_apply(scores, num_classes):
    # (a pitch <= 0 is the largest image of the blob: never more than its rows)
    P = _rows_pitch()
    return scores.is_cuda and scores.shape[1] == num_classes and \
        device_post_detections_fit(num_classes, P if P > 0 else scores.shape[0])


@torch.no_grad()
def post_detections_batched_device(scores, boxes, rois, n_images, num_classes, thresh=0.05, max_per_image=300,
                                   max_rows_per_image=None, agnostic=None):
    """The post-detection step of N images as one C-ABI call (wssdl_post_detections_batched, or
    wssdl_post_detections_agnostic_batched for the class-agnostic variant; agnostic=None reads
    cfg.TEST.CLS_AGNOSTIC_NMS: one set of launches, no read-back).
    rois [R,5] is the blob behind scores [R,K] / boxes [R,4K]; only its batch
    column is read.  Returns (dets [N, K-1, P, 5] f32, counts [N, K-1] i32) on the GPU with
    P = max_rows_per_image (default cfg.TEST.RPN_POST_NMS_TOP_N, or the largest image when that is <= 0);
    dets[i, j-1, :counts[i, j-1]] are image i's class-j detections, best first; counts[i, 0] == -1 flags an
    image with more than P rows."""
    from .. import _lib
    if agnostic is None:
        agnostic = bool(cfg.TEST.CLS_AGNOSTIC_NMS)
    name = "wssdl_post_detections_agnostic_batched" if agnostic else "wssdl_post_detections_batched"
    s = scores.to(torch.float32).contiguous()
    b = boxes.to(torch.float32).contiguous()
    r = rois.to(torch.float32).contiguous()
    R, K = s.shape
    N = int(n_images)
    if K != num_classes or b.shape != (R, 4 * K) or r.shape != (R, 5):
        raise ValueError("expected scores [R,K], boxes [R,4K], rois [R,5] with K = num_classes")
    P = _rows_pitch(max_rows_per_image)
    if P <= 0:
        live = r[:, 0][(r[:, 0] >= 0) & (r[:, 0] < N)].to(torch.int64)
        P = int(torch.bincount(live, minlength=1).max()) if live.numel() else 1
    if agnostic and (K - 1) * P > _lib.POST_AGNOSTIC_MAX_UNION:
        raise ValueError("class-agnostic NMS on the device: (K-1) * max_rows_per_image = %d exceeds "
                         "WSSDL_POST_AGNOSTIC_MAX_UNION = %d" % ((K - 1) * P, _lib.POST_AGNOSTIC_MAX_UNION))
    L = _lib.lib()
    dets = torch.empty((N, K - 1, max(P, 1), 5), dtype=torch.float32, device=s.device)
    counts = torch.empty((N, K - 1), dtype=torch.int32, device=s.device)
    with torch.cuda.device(s.device):
        n = getattr(L, name + "_workspace_bytes")(N, P, K)
        ws = torch.empty((n,), dtype=torch.uint8, device=s.device)
        _lib.check(getattr(L, name)(_lib.ptr(r), _lib.ptr(s), _lib.ptr(b), R, N, P, K, float(thresh), float(cfg.TEST.NMS),
                                    int(max_per_image), _lib.ptr(dets), _lib.ptr(counts), _lib.ptr(ws), n,
                                    _lib.stream()), name)
    return dets, counts


def _vote_thresh(vote_thresh=None):
    """vote_thresh of the views op: cfg.TEST.BBOX_VOTE_THRESH under cfg.TEST.BBOX_VOTE, else 0 (no voting)"""
    if vote_thresh is not None:
        return float(vote_thresh)
    return float(cfg.TEST.BBOX_VOTE_THRESH) if cfg.TEST.BBOX_VOTE else 0.0


@torch.no_grad()
def post_detections_views_device(scores, boxes, rois, n_images, views, flip_width, num_classes, thresh=0.05,
                                 max_per_image=300, max_rows_per_image=None, agnostic=None, vote_thresh=None):
    """Test-time augmentation as one C-ABI call (wssdl_post_detections_views: one set of launches, no read-back): the
    blob behind scores [R,K] / boxes [R,4K] / rois [R,5] holds n_images * views source images, source s = view
    s % views of output image s // views; flip_width [n_images * views] f32 (GPU tensor, or None) holds the original
    width of every mirrored source and -1 for the others.  The views' rows are brought into the image's own frame,
    go through one NMS (class-agnostic pass: agnostic, None reads cfg.TEST.CLS_AGNOSTIC_NMS) and the cap, and with
    vote_thresh > 0 (None: cfg.TEST.BBOX_VOTE_THRESH under cfg.TEST.BBOX_VOTE, else 0) every surviving box becomes
    the score-weighted mean of its class's candidates that overlap it by at least vote_thresh.
    Returns (dets [N, K-1, P, 5] f32, counts [N, K-1] i32) on the GPU like post_detections_batched_device, with
    P = max_rows_per_image (default views * cfg.TEST.RPN_POST_NMS_TOP_N, or the longest image when that is <= 0);
    counts[i, 0] == -1 flags an image whose views span more than P rows."""
    from .. import _lib
    if agnostic is None:
        agnostic = bool(cfg.TEST.CLS_AGNOSTIC_NMS)
    vt = _vote_thresh(vote_thresh)
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
    P = int(max_rows_per_image) if max_rows_per_image is not None else V * int(cfg.TEST.RPN_POST_NMS_TOP_N)
    if P <= 0:
        col = r[:, 0]
        live = torch.nonzero((col >= 0) & (col < N * V)).reshape(-1)
        P = 1
        if live.numel():
            img = torch.div(col[live].to(torch.int64), V, rounding_mode="floor")
            lo = torch.full((N,), R, dtype=torch.int64, device=s.device).scatter_reduce(0, img, live, "amin")
            hi = torch.full((N,), -1, dtype=torch.int64, device=s.device).scatter_reduce(0, img, live, "amax")
            P = max(int((hi - lo + 1).max()), 1)
    if agnostic and (K - 1) * P > _lib.POST_AGNOSTIC_MAX_UNION:
        raise ValueError("class-agnostic NMS on the device: (K-1) * max_rows_per_image = %d exceeds "
                         "WSSDL_POST_AGNOSTIC_MAX_UNION = %d" % ((K - 1) * P, _lib.POST_AGNOSTIC_MAX_UNION))
    L = _lib.lib()
    dets = torch.empty((N, K - 1, max(P, 1), 5), dtype=torch.float32, device=s.device)
    counts = torch.empty((N, K - 1), dtype=torch.int32, device=s.device)
    with torch.cuda.device(s.device):
        n = L.wssdl_post_detections_views_workspace_bytes(N, V, P, K)
        ws = torch.empty((n,), dtype=torch.uint8, device=s.device)
        _lib.check(L.wssdl_post_detections_views(_lib.ptr(r), _lib.ptr(s), _lib.ptr(b), R, N, V,
                                                 _lib.ptr(fw) if fw is not None else None, P, K, float(thresh),
                                                 float(cfg.TEST.NMS), int(bool(agnostic)), vt, int(max_per_image),
                                                 _lib.ptr(dets), _lib.ptr(counts), _lib.ptr(ws), n, _lib.stream()),
                   "wssdl_post_detections_views")
    return dets, counts


def unmirror_boxes(boxes, rois, n_images, views, flip_width):
    """Step 1 of the views statement with torch ops, every operation rounded to f32 on its own: for the rows of a
    mirrored source (flip_width[source] = w >= 0) every class's x1' = max((w - x2) - 1, 0), x2' = (w - x1) - 1.
    Returns (boxes' [R,4K] f32 -- a copy --, image [R] int64: the output image of every row, -1 for dead rows)."""
    b = boxes.to(torch.float32).clone()
    col = rois[:, 0]
    live = (col >= 0) & (col < n_images * views)
    src = torch.where(live, col, torch.zeros_like(col)).to(torch.int64)
    image = torch.where(live, torch.div(src, views, rounding_mode="floor"), torch.full_like(src, -1))
    if flip_width is not None:
        fw = torch.as_tensor(flip_width, dtype=torch.float32).to(b.device)
        w = fw[src]
        rows = torch.nonzero(live & (w >= 0)).reshape(-1)
        if rows.numel():
            wr = w[rows].unsqueeze(1)
            x1, x2 = b[rows, 0::4], b[rows, 2::4]
            b[rows, 0::4] = ((wr - x2) - 1.0).clamp_min(0.0)
            b[rows, 2::4] = (wr - x1) - 1.0
    return b, image


def vote_boxes_host(dets, cands, vote_thresh):
    """Step 5 of the views statement for one class of one image on the host: dets [n,5] (after NMS and cap), cands [m,5]
    (the class's rows above the score threshold, un-mirrored, ascending row order), both f32 NumPy.  The overlap is
    utils/bbox.pyx's in f64 (candidate = box, detection = query); the sums run serially in row order in f64
    (np.cumsum), one division, one rounding to f32.  Returns the voted dets [n,5] f32."""
    out = np.array(dets, dtype=np.float32, copy=True)
    c = np.asarray(cands, np.float64)
    for i in range(out.shape[0]):
        q = out[i].astype(np.float64)
        qarea = (q[2] - q[0] + 1) * (q[3] - q[1] + 1)
        iw = np.minimum(c[:, 2], q[2]) - np.maximum(c[:, 0], q[0]) + 1
        ih = np.minimum(c[:, 3], q[3]) - np.maximum(c[:, 1], q[1]) + 1
        inter = iw * ih
        ua = (c[:, 2] - c[:, 0] + 1) * (c[:, 3] - c[:, 1] + 1) + qarea - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            ov = np.where((iw > 0) & (ih > 0), inter / ua, 0.0)
        m = c[ov >= vote_thresh]
        if len(m) == 0:
            continue
        sw = np.cumsum(m[:, 4])[-1]
        if not sw > 0:
            continue
        for k in range(4):
            out[i, k] = np.float32(np.cumsum(m[:, 4] * m[:, k])[-1] / sw)
    return out


@torch.no_grad()
def _postprocess_views(scores, boxes, rois, n_images, num_classes, thresh, max_per_image, views, flip_width):
    """postprocess_detections_batch under test-time augmentation (views > 1 or cfg.TEST.BBOX_VOTE): the device op
    (post_detections_views_device, one read-back of the counts) for GPU tensors it takes; else the same statement step
    by step on the host with equal bits: unmirror_boxes, postprocess_detections on every output image's rows,
    vote_boxes_host."""
    vt = _vote_thresh()
    if vt > 1.0 or (vt > 0.0 and thresh < 0):
        raise ValueError("box voting needs BBOX_VOTE_THRESH <= 1 and a score threshold >= 0")
    top = int(cfg.TEST.RPN_POST_NMS_TOP_N)
    if scores.is_cuda and scores.shape[1] == num_classes and 1 <= views <= 8 and \
            device_post_detections_fit(num_classes, views * top if top > 0 else scores.shape[0]):
        dets, counts = post_detections_views_device(scores, boxes, rois, n_images, views, flip_width, num_classes, thresh,
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
        s_i, b_i = scores[rows].to(torch.float32), ub[rows]
        d = postprocess_detections(s_i, b_i, num_classes, thresh, max_per_image)
        if vt > 0.0:
            s_np, b_np = s_i.cpu().numpy(), b_i.cpu().numpy()
            for j in range(1, num_classes):
                if d[j].shape[0] == 0:
                    continue
                inds = np.where(s_np[:, j] > thresh)[0]
                cands = np.hstack((b_np[inds, 4 * j:4 * j + 4], s_np[inds, j:j + 1])).astype(np.float32)
                voted = vote_boxes_host(d[j].cpu().numpy(), cands, vt)
                d[j] = torch.from_numpy(voted).to(d[j].device)
        out.append(d)
    return out


@torch.no_grad()
def postprocess_detections_batch(scores, boxes, rois, n_images, num_classes, thresh=0.05, max_per_image=300, views=1,
                                 flip_width=None):
    """postprocess_detections for every image of a batch: rows r of scores [R,K] / boxes [R,4K] belong to
    image rois[r, 0] (rows with a negative index are dead and ignored).  Returns a list of n_images dicts
    {j: dets [n,5]}, each equal to postprocess_detections on that image's rows.  On the GPU: one device op
    (post_detections_batched_device), class-agnostic or not, and ONE read-back of the counts [N, K-1] for the
    whole batch; CPU tensors, more than 64 classes, a class-agnostic union (K-1) * RPN_POST_NMS_TOP_N beyond
    WSSDL_POST_AGNOSTIC_MAX_UNION and FUSED_POST_DETECTIONS off loop over the images with
    postprocess_detections.

    Test-time augmentation: with views > 1 (the blob holds n_images * views source images, source s = view s % views of
    output image s // views; flip_width [n_images * views] marks the mirrored ones with their original width, -1
    otherwise) or under cfg.TEST.BBOX_VOTE the call goes to wssdl_post_detections_views (_postprocess_views), whose
    fallback is the same statement step by step on the host.

    Under cfg.TEST.SOFT_NMS = 'linear' | 'gaussian' the call goes to soft_nms.postprocess_soft_batch
    (wssdl_post_detections_soft, or the host path of the same statement), with or without views."""
    n_images = int(n_images)
    if cfg.TEST.SOFT_NMS != 'off':
        from .soft_nms import postprocess_soft_batch
        return postprocess_soft_batch(scores, boxes, rois, n_images, num_classes, thresh, max_per_image, int(views),
                                      flip_width)
    if int(views) > 1 or flip_width is not None or cfg.TEST.BBOX_VOTE:
        return _postprocess_views(scores, boxes, rois, n_images, num_classes, thresh, max_per_image, int(views), flip_width)
    if _device_post_detections_apply(scores, num_classes):
        dets, counts = post_detections_batched_device(scores, boxes, rois, n_images, num_classes, thresh, max_per_image)
        n = counts.cpu().tolist()
        over = [i for i in range(n_images) if n[i][0] < 0]
        if over:
            raise ValueError("image(s) %s have more RoI rows than max_rows_per_image = %d (cfg.TEST.RPN_POST_NMS_TOP_N)"
                             % (over, dets.shape[2]))
        return [{j: dets[i, j - 1, :n[i][j - 1]] for j in range(1, num_classes)} for i in range(n_images)]
    img = rois[:, 0]
    out = []
    for i in range(n_images):
        rows = torch.nonzero(img == i).reshape(-1)
        out.append(postprocess_detections(scores[rows], boxes[rows], num_classes, thresh, max_per_image))
    return out


def detect_images(net, planes, net_name, batch_size=8, thresh=0.05, max_per_image=300):
    """The detection half of test_net (test_bus.py:300-401) at `batch_size` images per forward: returns
    all_boxes[j][i] = numpy [n,5] (x1, y1, x2, y2, score) of image i, class j >= 1, in original-image
    coordinates -- the structure the reference pickles (all_boxes[0] stays a list of empty lists).
    Under cfg.TEST.FLIP_AUG every image is also detected mirrored: batch_size still counts original images, the
    forward sees 2 * batch_size, and the two views' rows go through one NMS in the image's own frame;
    cfg.TEST.BBOX_VOTE votes the surviving boxes (wssdl_post_detections_views, one device op for the batch)."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    all_boxes = None
    for b0 in range(0, len(planes), batch_size):
        chunk = planes[b0:b0 + batch_size]
        flip_width = None
        if cfg.TEST.FLIP_AUG:
            data, info, flip_width = get_test_blobs(chunk, net_name, flip_aug=True)
        else:
            data, info = get_test_blobs(chunk, net_name)
        scores, boxes, rois = im_detect_batch(net, data, info)
        K = int(scores.shape[1])
        if all_boxes is None:
            all_boxes = [[[] for _ in range(len(planes))] for _ in range(K)]
        if flip_width is not None:
            dets = postprocess_detections_batch(scores, boxes, rois, len(chunk), K, thresh, max_per_image, views=2,
                                                flip_width=flip_width)
        else:
            dets = postprocess_detections_batch(scores, boxes, rois, data.shape[0], K, thresh, max_per_image)
        # one read-back per batch
        parts = [d[j] for d in dets for j in range(1, K)]
        host = torch.cat(parts, 0).cpu().numpy() if parts else np.zeros((0, 5), np.float32)
        off = 0
        for i, d in enumerate(dets):
            for j in range(1, K):
                m = int(d[j].shape[0])
                all_boxes[j][b0 + i] = host[off:off + m]
                off += m
    return all_boxes if all_boxes is not None else []
