"""RPN-only proposals (reference code/lib/rpn_msr/generate.py:82-117, im_proposals / imdb_proposals): the boxes that
imdb.evaluate_recall consumes, at N images per forward.

    rpn_proposals_batch(net, data, im_info)     trunk -> rpn_conv -> rpn_cls_score / rpn_bbox_pred -> proposal layer
                                                (TEST settings); no RoI pooling, no head, nothing read back
    im_proposals(net, plane, net_name)          boxes [n, 4] of one grey plane in original-image pixels
    imdb_proposals(net, imdb, batch_size=8)     the reference's list of per-image box arrays

(rois_padded, counts) of rpn_proposals_batch with im_info[:, 2] as scales is the device triple
datasets.recall.evaluate_recall_table takes as it is.

Out of scope: the reference's `scores` return value and imdb_proposals_det.  The proposal op does not export the
scores of the boxes it keeps, and nothing on the recall path reads them: im_proposals returns the boxes alone."""
import numpy as np
import torch

from ..fast_rcnn.config import cfg
from ..networks.network import Network
from ..networks.Resnet_train_bus import _feat_stride, anchor_scales
from .proposal_layer_tf_bus import proposal_layer_padded


@torch.no_grad()
def rpn_proposals_batch(net, data, im_info):
    """The RPN half of the test network's forward for data [N,H,W,3] NHWC and im_info [N,>=3] (h, w, scale, ...):
    returns (rois_padded [N, P, 5] f32, counts [N] i32) on the device, P = cfg.TEST.RPN_POST_NMS_TOP_N, rows
    (batch index, x1, y1, x2, y2) in network-input pixels -- image i's first counts[i] rows are its rows of
    layers['rpn_rois'] of net(..., test_net=True), bit for bit (the same modules, the same proposal op, under
    cfg.FUSED_RPN_SOFTMAX and cfg.USE_GPU_NMS like the networks' forward).  Works for Resnet_train_bus and
    VGGnet_train_bus alike (trunk, rpn_conv, rpn_cls_score, rpn_bbox_pred).  Eval mode for the call; the training
    flag is restored.  A count of -1 marks an image whose NMS sweep timed out (see proposal_layer_tf_bus)."""
    was_training = net.training
    net.eval()
    try:
        x = data.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        rpn = net.rpn_conv(net.trunk(x))
        score = net.rpn_cls_score(rpn).permute(0, 2, 3, 1).contiguous()
        pred = net.rpn_bbox_pred(rpn).permute(0, 2, 3, 1).contiguous()
        if cfg.FUSED_RPN_SOFTMAX:
            return proposal_layer_padded(score, pred, im_info, False, _feat_stride, anchor_scales, from_logits=True)
        # reshape_layer(2) -> softmax -> reshape_layer(2A), the layers' own arithmetic without registering them
        reshape = Network.reshape_layer.__wrapped__
        prob = torch.softmax(reshape(net, score, 2, name='rpn_cls_score_reshape'), dim=-1)
        prob = reshape(net, prob, len(anchor_scales) * 3 * 2, name='rpn_cls_prob_reshape')
        return proposal_layer_padded(prob, pred, im_info, False, _feat_stride, anchor_scales)
    finally:
        net.train(was_training)


def _boxes_of_batch(net, planes, net_name):
    """Per-image boxes of one batch: one forward, ONE read-back (rois, counts and scales in one buffer)."""
    from ..fast_rcnn.detect_batch import get_test_blobs
    data, info = get_test_blobs(planes, net_name)
    rois, counts = rpn_proposals_batch(net, data, info)
    N, P = int(rois.shape[0]), int(rois.shape[1])
    # (a count is at most P < 2^24: exact in f32)
    host = torch.cat((rois.reshape(N, P * 5), counts.to(torch.float32).reshape(N, 1), info[:, 2:3].to(torch.float32)), 1).cpu().numpy()
    out = []
    for i in range(N):
        n, scale = int(host[i, P * 5]), np.float32(host[i, P * 5 + 1])
        if n < 0:
            from .. import _lib
            raise _lib.HipCallError("im_proposals: the NMS sweep of image %d of the batch timed out (roi count -1)" % i)
        r = host[i, :P * 5].reshape(P, 5)[:n, 1:]
        # generate.py:93 under the NumPy it was written for: an f32 array over a scalar stays f32 (NumPy 2 would
        # promote an f64 scalar's quotient to f64), so both operands are f32 here and the division is IEEE f32
        out.append(r.astype(np.float32) / np.float32(scale))
    return out


def im_proposals(net, plane, net_name):
    """generate.py:82-95 for one grey plane [h, w]: boxes [n, 4] f32 in original-image pixels, rois[:, 1:] / scale
    in f32.  (The reference's second return value, the scores, is out of scope: see the module docstring.)"""
    return _boxes_of_batch(net, [plane], net_name)[0]


def imdb_proposals(net, imdb, batch_size=8, net_name=None):
    """generate.py:97-117: the list of per-image box arrays of imdb.image_path_at(i), i = 0 .. num_images-1, at
    `batch_size` images per forward (get_test_blobs per batch, one read-back per batch).  net_name defaults to the
    network's class name (its first six letters select the input normalisation)."""
    from ..utils.blob import imread
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    net_name = type(net).__name__ if net_name is None else net_name
    imdb_boxes = [[] for _ in range(imdb.num_images)]
    for b0 in range(0, imdb.num_images, batch_size):
        idx = range(b0, min(b0 + batch_size, imdb.num_images))
        for i, boxes in zip(idx, _boxes_of_batch(net, [imread(imdb.image_path_at(i)) for i in idx], net_name)):
            imdb_boxes[i] = boxes
    return imdb_boxes
