"""Mini-batch blobs from roidb entries (reference roi_data_layer/minibatch_bus.py:15-56, 96-139, 259-318).

Each of get_minibatch / get_minibatch_joint is two steps:
  1. plan_minibatch[_joint]: host only, NumPy only.  EVERY random draw of the reference, in its order -- first
     npr.randint(0, len(cfg.TRAIN.SCALES), size=num_images) (:19, :102), then image by image what prep_im_for_blob draws
     (utils.blob.draw_prep_params: angle and crop of a weak image, brightness and contrast when training) -- and
     everything that follows from the draws without touching a pixel: shapes, im_scales, gt_boxes, num_gt_boxes, im_info.
  2. utils.blob.image_batch_blob(plan, planes): the image blob of the whole batch in one device op.  With the
     environment variable WSSDL_IMAGE_BATCH=0 the per-image functions build it instead (utils.blob.image_blob_per_image:
     the same bits, a chain of launches per image) -- for A/B runs and as a fallback.
The result is a dict of device tensors with synthetic.make_batch's keys, dtypes and layouts.

A roidb entry carries 'image' (a path, decoded on the host by utils.blob.imread) or 'plane' (a decoded [h, w] u8 array),
'flipped', 'boxes', 'gt_classes' and 'birads_diag'.  Only the cfg.TRAIN.HAS_RPN branch exists."""
import os

import numpy as np
import torch

from ..fast_rcnn.config import cfg
from ..utils import blob as B


class ImagePlan(object):
    """One image of a planned mini-batch: the draws and what follows from them."""
    __slots__ = ("flipped", "is_ws", "target_size", "max_size", "angle", "crop", "delta", "factor", "pre_shape",
                 "resize_shape", "im_scale")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


class MinibatchPlan(object):
    """images: [ImagePlan]; blob_shape = (Hmax, Wmax); im_scales; gt_boxes [N, MAX_GT_PER_IMAGE, 5] f32;
    num_gt_boxes [N] i32; im_info [N, 4] f32 (blob H, blob W, im_scale, birads_diag)."""

    def __init__(self, net_name, images, gt_boxes, num_gt_boxes, im_info):
        self.net_name = net_name
        self.images = images
        self.blob_shape = (max(im.resize_shape[0] for im in images), max(im.resize_shape[1] for im in images))
        self.im_scales = [im.im_scale for im in images]
        self.pre_shapes = [im.pre_shape for im in images]
        self.resize_shapes = [im.resize_shape for im in images]
        self.gt_boxes, self.num_gt_boxes, self.im_info = gt_boxes, num_gt_boxes, im_info


def entry_plane(entry):
    """The decoded grey plane [h, w] u8 of a roidb entry."""
    if entry.get("plane") is not None:
        return np.ascontiguousarray(entry["plane"], dtype=np.uint8)
    return B.imread(entry["image"])


def _plan_images(entries, ws_flags, shapes, is_training, rng):
    rng = np.random if rng is None else rng
    scale_inds = rng.randint(0, high=len(cfg.TRAIN.SCALES), size=len(entries))
    images = []
    for e, ws, shape, si in zip(entries, ws_flags, shapes, scale_inds):
        h, w = int(shape[0]), int(shape[1])
        angle, crop, delta, factor = B.draw_prep_params((h, w), is_training, ws, rng)
        if factor is not None and not np.isfinite(factor):
            raise ValueError("contrast factor %r" % (factor,))
        pre = (h, w) if crop is None else (h - crop[0] - crop[1], w - crop[2] - crop[3])
        if pre[0] < 1 or pre[1] < 1:
            raise ValueError("crop %s leaves nothing of a %d x %d image" % (crop, h, w))
        target = cfg.TRAIN.SCALES[int(si)]
        im_scale, shape_out = B.prep_im_scale(pre, target, cfg.TRAIN.MAX_SIZE)
        images.append(ImagePlan(flipped=bool(e.get("flipped", False)), is_ws=bool(ws), target_size=target,
                                max_size=cfg.TRAIN.MAX_SIZE, angle=angle, crop=crop, delta=delta, factor=factor,
                                pre_shape=pre, resize_shape=shape_out, im_scale=im_scale))
    return images


def _plan(entries, ws_flags, gt_flags, net_name, is_training, rng, planes):
    if not cfg.TRAIN.HAS_RPN:
        raise NotImplementedError("only the cfg.TRAIN.HAS_RPN branch of the data layers exists")
    if not entries:
        raise ValueError("empty mini-batch")
    if planes is None:
        planes = [entry_plane(e) for e in entries]
    images = _plan_images(entries, ws_flags, [p.shape for p in planes], is_training, rng)
    n = len(entries)
    gt_boxes = np.zeros((n, cfg.TRAIN.MAX_GT_PER_IMAGE, 5), dtype=np.float32)
    num_gt = np.zeros((n,), dtype=np.int32)
    im_info = np.zeros((n, 4), dtype=np.float32)
    plan = MinibatchPlan(net_name, images, gt_boxes, num_gt, im_info)
    for i, (e, im, with_gt) in enumerate(zip(entries, images, gt_flags)):
        if with_gt:                                             # minibatch_bus.py:38-45, 117-123
            k = len(e["gt_classes"])
            g = np.empty((k, 5), dtype=np.float32)
            g[:, 0:4] = np.asarray(e["boxes"])[:k, :] * im.im_scale        # f64 product, stored as f32
            g[:, 4] = e["gt_classes"]
            gt_boxes[i, :k, :] = g
            num_gt[i] = k
        im_info[i, :] = [plan.blob_shape[0], plan.blob_shape[1], im.im_scale, e["birads_diag"]]
    plan.planes = planes
    return plan


def plan_minibatch(roidb, net_name, num_classes, is_training, is_ws, rng=None, planes=None):
    """Step 1 of get_minibatch.  `rng`: a RandomState (default: NumPy's global legacy stream, like the reference);
    `planes`: the entries' decoded planes when the caller has them already."""
    ws = bool(is_ws)
    return _plan(list(roidb), [ws] * len(roidb), [not ws] * len(roidb), net_name, is_training, rng, planes)


def plan_minibatch_joint(roidb_s, roidb_ws, net_name, num_classes, is_training, rng=None, planes=None):
    """Step 1 of get_minibatch_joint: the supervised entries first, then the weak ones, one stream through both."""
    ns, nw = len(roidb_s), len(roidb_ws)
    return _plan(list(roidb_s) + list(roidb_ws), [False] * ns + [True] * nw, [True] * ns + [False] * nw, net_name,
                 is_training, rng, planes)


def use_image_batch():
    return os.environ.get("WSSDL_IMAGE_BATCH", "1") != "0"


def plan_blobs(plan, device=None):
    """Step 2: the device blobs of a plan."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        if use_image_batch():
            data = B.image_batch_blob(plan, plan.planes, dev)
        else:
            data = B.image_blob_per_image(plan, plan.planes, dev)
    return dict(data=data, im_info=torch.from_numpy(plan.im_info).to(dev),
                gt_boxes=torch.from_numpy(plan.gt_boxes).to(dev), num_gt_boxes=torch.from_numpy(plan.num_gt_boxes).to(dev))


def get_minibatch(roidb, net_name, num_classes, is_training, is_ws, rng=None):
    """The device blobs of the mini-batch made of `roidb`'s entries, all supervised or all weak (is_ws): plan, then build."""
    return plan_blobs(plan_minibatch(roidb, net_name, num_classes, is_training, is_ws, rng=rng))


def get_minibatch_joint(roidb_s, roidb_ws, net_name, num_classes, is_training, rng=None):
    """The device blobs of the joint mini-batch: `roidb_s`'s entries first, then `roidb_ws`'s: plan, then build."""
    return plan_blobs(plan_minibatch_joint(roidb_s, roidb_ws, net_name, num_classes, is_training, rng=rng))
