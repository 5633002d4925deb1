"""The four supervised loss terms as ONE device op with its own backward.

Reference: code/lib/fast_rcnn/train_bus.py:186-235 (alternating mode) == :605-647 (combined
mode, where the RPN box term covers the first IMS_PER_BATCH images): ~40 TF element-wise and
reduction ops; here one forward launch (+ a one-workgroup finish) and one backward launch of
`csrc/loss.hip`.  The op takes the layers as the network produces them -- `rpn_cls_score`
[N,H,W,2A] instead of its `rpn_cls_score_reshape` view (network.py:283-291 is an index map) -- so
neither the reshape nor the NCHW -> NHWC permutes of the targets are materialised.

`multi_task_loss_per_image` gives the same four terms for each image of a batch, forward only: what a
validation pass averages (the reference evaluates them one validation image per step, :427-534 / :792-899).
"""
import torch

from .. import _lib

TERMS = ("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box")


def _i32(t):
    return t if t.dtype == torch.int32 else t.to(torch.int32)


class _MultiTaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_labels, rpn_tg, rpn_inw, rpn_outw,
                labels, tg, inw, outw, n_box_images):
        _lib.require_cuda(rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_labels, rpn_tg, rpn_inw, rpn_outw,
                          labels, tg, inw, outw)
        L = _lib.lib()
        N, H, W, A2 = rpn_cls_score.shape
        A = A2 // 2
        if tuple(rpn_bbox_pred.shape) != (N, H, W, 4 * A):
            raise _lib.HipCallError("rpn_bbox_pred %s does not match rpn_cls_score %s" %
                                    (tuple(rpn_bbox_pred.shape), tuple(rpn_cls_score.shape)))
        if rpn_labels.numel() != N * A * H * W or tuple(rpn_tg.shape) != (N, 4 * A, H, W):
            raise _lib.HipCallError("rpn-data shapes do not match the score map")
        K = cls_score.shape[1]
        n_rows = labels.numel()
        if n_rows > cls_score.shape[0] or tuple(tg.shape) != (n_rows, 4 * K) or bbox_pred.shape[1] != 4 * K:
            raise _lib.HipCallError("roi-data shapes do not match the head outputs")
        f32 = torch.float32
        t = [x.contiguous() if x.dtype == f32 else x.to(f32).contiguous()
             for x in (rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_tg, rpn_inw, rpn_outw, tg, inw, outw)]
        rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_tg, rpn_inw, rpn_outw, tg, inw, outw = t
        rpn_labels = _i32(rpn_labels).contiguous()
        labels = _i32(labels).reshape(-1).contiguous()
        dev = rpn_cls_score.device
        nb = int(n_box_images) if n_box_images is not None else N
        ws = torch.empty((L.wssdl_multi_task_loss_workspace_bytes(N, H, W, A),), dtype=torch.uint8, device=dev)
        losses = torch.empty((4,), dtype=f32, device=dev)
        with torch.cuda.device(dev), _lib.timed("multi_task_loss", dict(N=N, H=H, W=W, A=A, rows=n_rows)):
            _lib.check(L.wssdl_multi_task_loss_forward(
                _lib.ptr(rpn_cls_score), _lib.ptr(rpn_labels), _lib.ptr(rpn_bbox_pred), _lib.ptr(rpn_tg),
                _lib.ptr(rpn_inw), _lib.ptr(rpn_outw), N, nb, H, W, A, _lib.ptr(cls_score), _lib.ptr(labels),
                _lib.ptr(bbox_pred), _lib.ptr(tg), _lib.ptr(inw), _lib.ptr(outw), n_rows, K, _lib.ptr(losses),
                _lib.ptr(ws), ws.numel(), _lib.stream()), "wssdl_multi_task_loss_forward")
        ctx.save_for_backward(rpn_cls_score, rpn_labels, rpn_bbox_pred, rpn_tg, rpn_inw, rpn_outw, cls_score, labels,
                              bbox_pred, tg, inw, outw, ws)
        ctx.dims = (N, nb, H, W, A, n_rows, K)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        (rpn_cls_score, rpn_labels, rpn_bbox_pred, rpn_tg, rpn_inw, rpn_outw, cls_score, labels, bbox_pred, tg, inw,
         outw, ws) = ctx.saved_tensors
        N, nb, H, W, A, n_rows, K = ctx.dims
        L = _lib.lib()
        gl = grad_losses.to(torch.float32).contiguous()
        g_rpn_cls = torch.empty_like(rpn_cls_score)
        g_rpn_box = torch.empty_like(rpn_bbox_pred)
        g_cls = torch.empty_like(cls_score)
        g_box = torch.empty_like(bbox_pred)
        with torch.cuda.device(gl.device), _lib.timed("multi_task_loss_backward", dict(N=N, H=H, W=W, A=A, rows=n_rows)):
            _lib.check(L.wssdl_multi_task_loss_backward(
                _lib.ptr(rpn_cls_score), _lib.ptr(rpn_labels), _lib.ptr(rpn_bbox_pred), _lib.ptr(rpn_tg),
                _lib.ptr(rpn_inw), _lib.ptr(rpn_outw), N, nb, H, W, A, _lib.ptr(cls_score), _lib.ptr(labels),
                _lib.ptr(bbox_pred), _lib.ptr(tg), _lib.ptr(inw), _lib.ptr(outw), n_rows, cls_score.shape[0], K,
                _lib.ptr(gl), _lib.ptr(ws), _lib.ptr(g_rpn_cls), _lib.ptr(g_rpn_box), _lib.ptr(g_cls),
                _lib.ptr(g_box), _lib.stream()), "wssdl_multi_task_loss_backward")
        return (g_rpn_cls, g_rpn_box, g_cls, g_box) + (None,) * 9


def multi_task_loss(rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_data, roi_data, n_box_images=None):
    """-> tensor [4]: rpn_cross_entropy, rpn_loss_box, cross_entropy, loss_box (TERMS).
    rpn_data = (labels, targets, inside_w, outside_w) of the anchor-target layer, roi_data =
    (rois, labels, targets, inside_w, outside_w) of the proposal-target layer."""
    return _MultiTaskLoss.apply(rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_data[0], rpn_data[1],
                                rpn_data[2], rpn_data[3], roi_data[1], roi_data[2], roi_data[3], roi_data[4],
                                n_box_images)


def _per_image_torch(rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_data, roi_data, n_images):
    """The per-image terms with the torch chain of train_bus.py on each image's slice (CPU tensors, a head wider
    than the device op takes, cfg.FUSED_LOSS off).  The slices are handed over in f64 and each value is rounded to
    f32 once, so this path is itself inside the error bounds counted for the device op (tests/loss_reference.py)
    and can stand in for it in tests without a GPU."""
    from . import train_bus as T
    f64 = torch.float64
    rois, labels = roi_data[0], roi_data[1].reshape(-1)
    n_rows = labels.numel()
    img = rois[:n_rows, 0]
    N, H, W, A2 = rpn_cls_score.shape
    # network.py:283-291 as an index map: [N,H,W,2A] -> [N, A*H, W, 2]
    reshaped = rpn_cls_score.permute(0, 3, 1, 2).reshape(N, 2, (A2 // 2) * H, W).permute(0, 2, 3, 1)
    dev = rpn_cls_score.device
    losses = torch.empty((n_images, 4), dtype=f64, device=dev)
    counts = torch.empty((n_images, 2), dtype=torch.float32, device=dev)
    for i in range(n_images):
        # rows of image i that carry a label in [0, K): padding and out-of-range labels contribute to nothing
        keep = ((img == i) & (labels >= 0) & (labels < cls_score.shape[1])).nonzero().reshape(-1)
        data_i = (rpn_data[0][i:i + 1],) + tuple(t[i:i + 1].to(f64) for t in rpn_data[1:4])
        roi_i = (rois[keep], labels[keep]) + tuple(t[keep].to(f64) for t in roi_data[2:5])
        losses[i, 0] = T.rpn_cls_loss(reshaped[i:i + 1].to(f64), data_i[0])
        losses[i, 1] = T.rpn_box_loss(rpn_bbox_pred[i:i + 1].to(f64), data_i)
        losses[i, 2] = T.rcnn_cls_loss(cls_score[keep].to(f64), roi_i[1])
        losses[i, 3] = T.rcnn_box_loss(bbox_pred[keep].to(f64), roi_i)
        counts[i, 0] = (data_i[0] != -1).sum()
        counts[i, 1] = keep.numel()
    losses = losses.to(torch.float32)
    return losses, counts


def multi_task_loss_per_image(rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_data, roi_data, n_images):
    """-> (losses [n_images, 4] f32: TERMS of each image, counts [n_images, 2] f32: its labelled anchors and rows).
    Row i is what multi_task_loss gives for a batch that holds image i alone -- rpn_* and rpn_data sliced on
    dimension 0, the rows r of the head outputs and of roi_data with roi_data[0][r, 0] == i -- except that loss_box
    sums the rows with a label in [0, K) only.  Rows need not be grouped by image; an image without labelled anchors
    or rows has NaN for that cross-entropy.  Forward only, no autograd: one device launch (and its finish) for all
    images, nothing read back.  CPU tensors, K outside 2..32 and cfg.FUSED_LOSS = False take the torch chain of
    train_bus.py image by image."""
    from .config import cfg
    tensors = (rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred) + tuple(rpn_data[:4]) + tuple(roi_data[:5])
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError("multi_task_loss_per_image has no backward: call it under torch.no_grad() or on detached tensors")
    N, H, W, A2 = rpn_cls_score.shape
    A = A2 // 2
    n_images = int(n_images)
    if n_images < 1 or n_images > N:
        raise ValueError("n_images = %d for a score map of %d image(s)" % (n_images, N))
    K = cls_score.shape[1]
    if not (rpn_cls_score.is_cuda and cfg.get('FUSED_LOSS', True) and 2 <= K <= 32):
        with torch.no_grad():
            return _per_image_torch(rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_data, roi_data, n_images)
    rois, labels, tg, inw, outw = roi_data[:5]
    rpn_labels, rpn_tg, rpn_inw, rpn_outw = rpn_data[:4]
    _lib.require_cuda(*tensors)
    L = _lib.lib()
    n_rows = labels.numel()
    if tuple(rpn_bbox_pred.shape) != (N, H, W, 4 * A):
        raise _lib.HipCallError("rpn_bbox_pred %s does not match rpn_cls_score %s" %
                                (tuple(rpn_bbox_pred.shape), tuple(rpn_cls_score.shape)))
    if rpn_labels.numel() != N * A * H * W or tuple(rpn_tg.shape) != (N, 4 * A, H, W):
        raise _lib.HipCallError("rpn-data shapes do not match the score map")
    if n_rows > cls_score.shape[0] or tuple(tg.shape) != (n_rows, 4 * K) or bbox_pred.shape[1] != 4 * K \
            or rois.dim() != 2 or rois.shape[0] < n_rows:
        raise _lib.HipCallError("roi-data shapes do not match the head outputs")
    f32 = torch.float32
    t = [x.contiguous() if x.dtype == f32 else x.to(f32).contiguous()
         for x in (rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_tg, rpn_inw, rpn_outw, tg, inw, outw, rois)]
    rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_tg, rpn_inw, rpn_outw, tg, inw, outw, rois = t
    rpn_labels = _i32(rpn_labels).contiguous()
    labels = _i32(labels).reshape(-1).contiguous()
    dev = rpn_cls_score.device
    ws = torch.empty((L.wssdl_multi_task_loss_per_image_workspace_bytes(n_images, H, W, A),), dtype=torch.uint8, device=dev)
    losses = torch.empty((n_images, 4), dtype=f32, device=dev)
    counts = torch.empty((n_images, 2), dtype=f32, device=dev)
    with torch.cuda.device(dev), _lib.timed("multi_task_loss_per_image", dict(N=n_images, H=H, W=W, A=A, rows=n_rows)):
        _lib.check(L.wssdl_multi_task_loss_per_image(
            _lib.ptr(rpn_cls_score), _lib.ptr(rpn_labels), _lib.ptr(rpn_bbox_pred), _lib.ptr(rpn_tg), _lib.ptr(rpn_inw),
            _lib.ptr(rpn_outw), n_images, H, W, A, _lib.ptr(cls_score), _lib.ptr(labels), _lib.ptr(bbox_pred),
            _lib.ptr(tg), _lib.ptr(inw), _lib.ptr(outw), n_rows, K, _lib.ptr(rois), int(rois.shape[1]),
            _lib.ptr(losses), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream()),
            "wssdl_multi_task_loss_per_image")
    return losses, counts
