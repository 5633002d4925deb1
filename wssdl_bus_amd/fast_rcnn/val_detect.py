"""The detection half of the reference's validation pass (code/lib/fast_rcnn/train_bus.py:445-514 alternating,
:810-879 combined): detections of the N images of ONE eval forward of the training wiring, from the `layers` that
forward already produced -- no second forward through the test wiring.

The reference takes cls_prob, bbox_pred and roi-data[0] out of the same sess.run that yields the losses, divides the
sampled RoIs by the image's scale, decodes the class-wise deltas, clips to the original image (:456-457) and runs
the per-class NMS, the class-agnostic pass and the max_per_image cap (:479-514).  Here the first three steps are one
device launch (wssdl_decode_detections, csrc/decode_detect.hip) and the rest is post_detections_batched_device;
nothing is read back.  detect_batch.im_detect_batch keeps its own chain of torch ops for the test protocol."""
import torch

from .config import cfg
from .detect_batch import post_detections_batched_device


@torch.no_grad()
def decode_detections_device(rois, deltas, im_info, n_images, bounds=None):
    """wssdl_decode_detections: rois [R,5] (batch index, box in the scaled image), deltas [R,4K], im_info
    [n_images, >=3] rows (h, w, scale, ...) -> boxes [R,4K] f32 in original-image pixels, clipped to bounds
    [n_images,2] = (xmax, ymax) per image, or, without bounds, to (w / scale - 1, h / scale - 1) computed in double.
    Rows whose batch index is outside [0, n_images) come out as zeros.  One launch, no read-back; GPU tensors only."""
    from .. import _lib
    _lib.require_cuda(rois, deltas)
    r = rois.to(torch.float32).contiguous()
    d = deltas.to(torch.float32).contiguous()
    info = _lib.to_device(im_info, torch.float32, r.device)
    n = int(n_images)
    R = int(r.shape[0])
    if r.dim() != 2 or r.shape[1] != 5 or d.dim() != 2 or d.shape[0] != R or d.shape[1] % 4 != 0:
        raise ValueError("expected rois [R,5] and deltas [R,4K]")
    if info.dim() != 2 or info.shape[0] < n or info.shape[1] < 3:
        raise ValueError("im_info must be [>= n_images, >= 3]")
    b = None
    if bounds is not None:
        b = _lib.to_device(bounds, torch.float32, r.device)
        if tuple(b.shape) != (n, 2):
            raise ValueError("bounds must be [n_images, 2] = (xmax, ymax) per image")
    boxes = torch.empty_like(d)
    with torch.cuda.device(r.device):
        _lib.check(_lib.lib().wssdl_decode_detections(_lib.ptr(r), _lib.ptr(d), R, int(d.shape[1]) // 4, _lib.ptr(info),
                                                      int(info.shape[1]), n, _lib.ptr(b), _lib.ptr(boxes), _lib.stream()),
                   "wssdl_decode_detections")
    return boxes


@torch.no_grad()
def validation_detections(layers, im_info, n_images, thresh=0.05, max_per_image=300, im_shapes=None, agnostic=None):
    """The detections of the n_images images of one eval forward of the training wiring: a pure function of its
    `layers`.  scores = layers['cls_prob'], deltas = layers['bbox_pred'], rois = layers['roi-data'][0] (the sampled
    RoIs, ground truth among them), the first two cut to the rois' row count.  As in the reference's validation loop
    bbox_pred is used as the network emits it (no un-normalisation under BBOX_NORMALIZE_TARGETS_PRECOMPUTED).
    im_shapes: the original (H, W) of every image, to clip to as the reference does (im.shape); without it the bounds
    are (w / scale - 1, h / scale - 1) of im_info.  agnostic=None reads cfg.TEST.CLS_AGNOSTIC_NMS.
    -> (dets [N, K-1, P, 5] f32, counts [N, K-1] i32) on the GPU in post_detections_batched_device's layout, with
    P = cfg.TRAIN.BATCH_SIZE (the sampler never emits more rows per image); nothing is read back.
    With im_shapes the bounds go up in a blocking copy from the host, which synchronises it; without them nothing does."""
    n = int(n_images)
    rois = layers['roi-data'][0]
    R = int(rois.shape[0])
    scores = layers['cls_prob'][:R]
    deltas = layers['bbox_pred'][:R]
    bounds = None
    if im_shapes is not None:
        if len(im_shapes) != n:
            raise ValueError("im_shapes names %d images, the forward holds %d" % (len(im_shapes), n))
        # clip_boxes(boxes, im.shape): (W - 1, H - 1) of the original image
        bounds = torch.tensor([(float(s[1]) - 1.0, float(s[0]) - 1.0) for s in im_shapes], dtype=torch.float32,
                              device=rois.device).reshape(n, 2)
    boxes = decode_detections_device(rois, deltas, im_info, n, bounds)
    if cfg.TEST.SOFT_NMS != 'off':                  # (addition) Soft-NMS in place of the hard one, the same layout
        from .soft_nms import post_detections_soft_device
        if agnostic:
            raise ValueError("cfg.TEST.SOFT_NMS cannot be combined with a class-agnostic pass")
        return post_detections_soft_device(scores, boxes, rois, n, 1, None, int(scores.shape[1]), thresh, max_per_image,
                                           max_rows_per_image=int(cfg.TRAIN.BATCH_SIZE))
    return post_detections_batched_device(scores, boxes, rois, n, int(scores.shape[1]), thresh, max_per_image,
                                          max_rows_per_image=int(cfg.TRAIN.BATCH_SIZE), agnostic=agnostic)
