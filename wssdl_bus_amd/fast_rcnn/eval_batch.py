"""Batched validation: detect N images per forward and score the detections where they are (the validation pass of
reference code/lib/fast_rcnn/train_bus.py:485-534 / :850-899 and test_net's evaluate_detections, without result
files): get_test_blobs -> im_detect_batch -> post_detections_batched_device -> DetectionAccumulator -> one
evaluation op.  No detection is read back; the summary is."""
from ..datasets.voc_eval_bus import DetectionAccumulator, evaluate_detections
from .config import cfg
from .detect_batch import get_test_blobs, im_detect_batch, post_detections_batched_device, post_detections_views_device


def accumulate_images(net, planes, net_name, batch_size=8, thresh=0.05, max_per_image=300):
    """The detections of `planes` at `batch_size` images per forward, kept on the GPU: a DetectionAccumulator.
    cfg.TEST.CLS_AGNOSTIC_NMS is honoured (post_detections_batched_device reads it); a class-agnostic union the
    device op does not take (post_detections_batched_device) raises -- per-class detections are never scored in its
    place.  cfg.TEST.FLIP_AUG (every image also detected mirrored: the forward sees 2 * batch_size images) and
    cfg.TEST.BBOX_VOTE / BBOX_VOTE_THRESH are honoured too: under either the batch goes through
    post_detections_views_device, whose output the accumulator takes as it stands.  So it does that of
    post_detections_soft_device under cfg.TEST.SOFT_NMS = 'linear' | 'gaussian' (with or without FLIP_AUG)."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    acc = None
    for b0 in range(0, len(planes), batch_size):
        chunk = planes[b0:b0 + batch_size]
        flip_width = None
        if cfg.TEST.FLIP_AUG:
            data, info, flip_width = get_test_blobs(chunk, net_name, flip_aug=True)
        else:
            data, info = get_test_blobs(chunk, net_name)
        scores, boxes, rois = im_detect_batch(net, data, info)
        K = int(scores.shape[1])
        if acc is None:
            acc = DetectionAccumulator(K)
        if cfg.TEST.SOFT_NMS != 'off':
            from .soft_nms import post_detections_soft_device
            dets, counts = post_detections_soft_device(scores, boxes, rois, len(chunk), 1 if flip_width is None else 2,
                                                       flip_width, K, thresh, max_per_image)
        elif flip_width is not None or cfg.TEST.BBOX_VOTE:
            dets, counts = post_detections_views_device(scores, boxes, rois, len(chunk), 1 if flip_width is None else 2,
                                                        flip_width, K, thresh, max_per_image)
        else:
            dets, counts = post_detections_batched_device(scores, boxes, rois, data.shape[0], K, thresh, max_per_image)
        acc.add(dets, counts, b0)
    return acc


def evaluate_images(net, planes, gt_roidb, net_name, batch_size=8, classes=None, thresh=0.05, max_per_image=300,
                    ovthresh=0.5, score_thresh=0.5, use_07_metric=True, vis_dir=None, image_paths=None):
    """evaluate_detections (datasets/voc_eval_bus.py) of the network's detections on `planes` against gt_roidb
    (one entry per plane).  classes: the class names, '__background__' first (default: numbered).
    vis_dir: also draw ground truth and detections over every plane on the device (fast_rcnn/vis.py: one op for all
    images, one read-back) and write <vis_dir>/<image basename>.png -- the reference's test_net(vis=True),
    test_bus.py:337-390; image_paths names the images (default: their index, six digits).  None (the default) draws
    nothing and changes nothing."""
    if len(planes) != len(gt_roidb):
        raise ValueError("one gt_roidb entry per image")
    acc = accumulate_images(net, planes, net_name, batch_size, thresh, max_per_image)
    if acc is None:
        raise ValueError("evaluate_images needs at least one image")
    if classes is None:
        classes = ['__background__'] + ['class_%d' % j for j in range(1, acc.num_classes)]
    if len(classes) != acc.num_classes:
        raise ValueError("the network scores %d classes, `classes` names %d" % (acc.num_classes, len(classes)))
    if vis_dir is not None:
        from . import vis
        names = image_paths if image_paths is not None else ['%06d' % i for i in range(len(planes))]
        if len(names) != len(planes):
            raise ValueError("one image path per plane")
        vis.save_qualitative(vis.draw_detections(planes, gt_roidb, acc, classes), vis.qualitative_paths(vis_dir, names))
    return evaluate_detections(acc, gt_roidb, classes, ovthresh, score_thresh, use_07_metric)
