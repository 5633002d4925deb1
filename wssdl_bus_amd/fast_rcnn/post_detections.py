"""The post-detection step of one image on the device, class-agnostic or not (reference
code/lib/fast_rcnn/test_bus.py:360-401).

``test_bus.postprocess_detections`` takes the per-class device op and, under cfg.TEST.CLS_AGNOSTIC_NMS, the
step-by-step form (a hip_nms per class, a concatenation, one more hip_nms, boolean masks).  Here the flag has a
device form too: wssdl_post_detections_agnostic runs the per-class step, the second NMS over the classes' kept rows
together (:371-384) and the max_per_image cap as one C-ABI call, with one read-back of the per-class counts.  The
result equals the step-by-step form's bit for bit.  The batched path (detect_batch.py) and the validation pass
(eval_batch.py) go through this module; whatever the device op does not take falls through to
``test_bus.postprocess_detections``."""
import torch

from . import test_bus
from .config import cfg


def device_post_detections_fit(num_classes, rows_per_image):
    """Whether the device op takes this shape under the current switches: at most 64 object classes, the fused
    form not switched off, and -- for the class-agnostic variant, whose union of one image is one NMS segment --
    (K-1) * rows_per_image within the library's WSSDL_POST_AGNOSTIC_MAX_UNION."""
    from .. import _lib
    if not (2 <= num_classes <= 65 and cfg.TEST.get("FUSED_POST_DETECTIONS", True)):
        return False
    return not cfg.TEST.CLS_AGNOSTIC_NMS or (num_classes - 1) * int(rows_per_image) <= _lib.POST_AGNOSTIC_MAX_UNION


@torch.no_grad()
def post_detections_device(scores, boxes, num_classes, thresh=0.05, max_per_image=300, agnostic=None):
    """The whole post-detection step as one C-ABI call (wssdl_post_detections, or wssdl_post_detections_agnostic
    for the class-agnostic variant: one set of launches for all classes, no read-back): returns
    (dets [K-1, R, 5] f32, counts [K-1] i32) on the GPU; rows dets[j-1, :counts[j-1]] are class j's detections in
    descending score order.  agnostic=None reads cfg.TEST.CLS_AGNOSTIC_NMS."""
    from .. import _lib
    if agnostic is None:
        agnostic = bool(cfg.TEST.CLS_AGNOSTIC_NMS)
    if not agnostic:
        return test_bus.post_detections_device(scores, boxes, num_classes, thresh, max_per_image)
    s = scores.to(torch.float32).contiguous()
    b = boxes.to(torch.float32).contiguous()
    R, K = s.shape
    L = _lib.lib()
    dets = torch.empty((K - 1, max(R, 1), 5), dtype=torch.float32, device=s.device)
    counts = torch.empty((K - 1,), dtype=torch.int32, device=s.device)
    with torch.cuda.device(s.device):
        n = L.wssdl_post_detections_agnostic_workspace_bytes(R, K)
        ws = torch.empty((n,), dtype=torch.uint8, device=s.device)
        _lib.check(L.wssdl_post_detections_agnostic(_lib.ptr(s), _lib.ptr(b), R, K, float(thresh), float(cfg.TEST.NMS),
                                                    int(max_per_image), _lib.ptr(dets), _lib.ptr(counts), _lib.ptr(ws),
                                                    n, _lib.stream()), "wssdl_post_detections_agnostic")
    return dets, counts


@torch.no_grad()
def postprocess_detections(scores, boxes, num_classes, thresh=0.05, max_per_image=300):
    """test_bus.postprocess_detections with a device form of cfg.TEST.CLS_AGNOSTIC_NMS: under the flag, GPU tensors
    whose union (K-1) * R is within WSSDL_POST_AGNOSTIC_MAX_UNION take wssdl_post_detections_agnostic and ONE
    read-back of the per-class counts.  Everything else -- flag off, CPU tensors, more than 64 classes, a longer
    union, FUSED_POST_DETECTIONS off -- is test_bus.postprocess_detections as it stands (its step-by-step form
    under the flag).  Returns {j: dets [n,5]} (GPU).
    Under cfg.TEST.SOFT_NMS = 'linear' | 'gaussian': soft_nms.postprocess_soft (wssdl_post_detections_soft on the image
    as a batch of one, or the host path of the same statement)."""
    if cfg.TEST.SOFT_NMS != 'off':
        from .soft_nms import postprocess_soft
        return postprocess_soft(scores, boxes, num_classes, thresh, max_per_image)
    if cfg.TEST.CLS_AGNOSTIC_NMS and scores.is_cuda and scores.shape[1] == num_classes and \
            device_post_detections_fit(num_classes, scores.shape[0]):
        dets, counts = post_detections_device(scores, boxes, num_classes, thresh, max_per_image, agnostic=True)
        n = counts.cpu().tolist()
        return {j: dets[j - 1, :n[j - 1]] for j in range(1, num_classes)}
    return test_bus.postprocess_detections(scores, boxes, num_classes, thresh, max_per_image)
