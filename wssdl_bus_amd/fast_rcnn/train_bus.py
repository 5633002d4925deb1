"""Multi-task loss and train steps (combined and alternating) on PyTorch-ROCm.

Reference: code/lib/fast_rcnn/train_bus.py:184-270 (alternating losses), :603-678 (combined
losses), :286-301 / :694-705 (optimisers and the per-variable sum of the two gradient sets),
:334-394 (one alternating iteration = a supervised step then a weak step).  Only what drives
the hot path's backward is restated here, with the optimisers and
learning-rate schedules of fast_rcnn/optim.py.  The program around the steps -- train_net / train_net_alter
(:1055-1087) -- is at the end of this module: thin entry points over fast_rcnn/train_loop.py (the loops, log.txt,
summary.jsonl), fast_rcnn/snapshot.py (snapshots and resume) and fast_rcnn/vis.py (qualitative results drawn on the
device); the data layers are roi_data_layer/.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from ..mil import core as mil_core
from ..networks import _plumbing
from ..roi_pooling_layer import roi_pooling_op
from . import optim
from .config import cfg


# ----------------------------------------------------------------- losses ---

def rpn_cls_loss(rpn_cls_score_reshape, rpn_labels):
    """train_bus.py:186-192 / :605-610: CE over anchors whose label != -1.
    rpn_cls_score_reshape [N, A*H, W, 2]; rpn_labels [N, 1, A*H, W] int."""
    score = rpn_cls_score_reshape.reshape(-1, 2)
    label = rpn_labels.reshape(-1).to(torch.int64)
    # mean CE over the anchors whose label != -1 (tf.gather of the kept rows in the reference);
    # ignore_index does the same without materialising the kept rows (no host sync)
    return F.cross_entropy(score, label, ignore_index=-1)


def rpn_box_loss(rpn_bbox_pred, rpn_data, n_images=None):
    """train_bus.py:203-210 / :613-620.  The 'smooth L1' switches at |d| < 1 while using the
    sigma = 3 pieces (0.5*(3*in_w*d)^2 and |d| - 0.5/9): the reference's formula, kept as is.
    rpn_bbox_pred [N,H,W,4A]; rpn_data = (labels, targets, inside_w, outside_w) [N,4A,H,W]."""
    tg, inw, outw = (t.permute(0, 2, 3, 1) for t in rpn_data[1:4])
    pred = rpn_bbox_pred
    if n_images is not None:                       # combined mode slices the supervised images
        pred, tg, inw, outw = pred[:n_images], tg[:n_images], inw[:n_images], outw[:n_images]
    d = pred - tg
    sign = (d.abs() < 1).to(pred.dtype)
    per = outw * (0.5 * (inw * d * 3) ** 2 * sign + (d.abs() - 0.5 / 9.0) * (sign - 1).abs())
    return per.sum(dim=(1, 2)).mean() * 10


def rcnn_cls_loss(cls_score, labels):
    """train_bus.py:218 / :623-630: CE over the first len(labels) rows."""
    label = labels.reshape(-1).to(torch.int64)
    # label -1 = padding row of a fixed-shape RoI list (an image short of candidates): not a row of
    # the reference's blob, so it is left out of the mean
    return F.cross_entropy(cls_score[:label.numel()], label, ignore_index=-1)


def rcnn_box_loss(bbox_pred, roi_data):
    """train_bus.py:231-235 / :641-647: plain L1, mean over rows of the weighted row sums."""
    tg, inw, outw = roi_data[2], roi_data[3], roi_data[4]
    pred = bbox_pred[:tg.shape[0]]
    per_row = (outw * (inw * (pred - tg).abs())).sum(dim=1)
    # mean over the rows of the reference's blob: padding rows (label -1, zero weights) do not count
    n_rows = (roi_data[1].reshape(-1) >= 0).sum().clamp_min(1)
    return per_row.sum() / n_rows


def mil_loss(cls_score_ws, batch_inds, mil_label, n_bags, global_step, funcs, counts_host=None):
    """train_bus.py:239-260 / :650-671: bag logits -> CE weighted by the class prior
    [0, WS_MAL_PCT, 1-WS_MAL_PCT] and by 1 - 0.99*0.9^floor(step/2000) (or a constant).
    On the GPU the bag selection is the HIP op (no host round trip); on CPU tensors (tests) the
    host-side restatement of mil/core.py runs."""
    scale = _mil_scale(global_step)
    # (the fused MIL op takes 3..8 classes, the reference has 3; anything else: selection op + torch CE)
    if cls_score_ws.is_cuda and cfg.get('FUSED_LOSS', True) and 3 <= cls_score_ws.shape[1] <= 8:
        # selection + weighted CE + mean as one device op with its own backward (f1)
        prior = [0.0, float(cfg.TRAIN.WS_MAL_PCT), 1.0 - float(cfg.TRAIN.WS_MAL_PCT)]
        return mil_core.mil_loss_device(cls_score_ws, batch_inds, 0.0, mil_label, n_bags, funcs, prior, scale)
    valid = None
    if cls_score_ws.is_cuda:
        bag_logits, _, valid = mil_core.get_bag_logit_device(cls_score_ws, batch_inds, 0.0, mil_label,
                                                             n_bags, funcs, return_valid=True)
    else:
        bag_logits, _ = mil_core.get_bag_logit(cls_score_ws, batch_inds, 3, mil_label, n_bags,
                                               funcs, counts_host)
    label = mil_label.reshape(-1).to(torch.int64)
    w = _class_prior(bag_logits)[label]
    if valid is not None:                          # an empty bag (no proposals) carries no loss
        w = w * valid.to(w.dtype)
    ce = F.cross_entropy(bag_logits, label, reduction='none')
    return (scale * (w * ce)).mean()


def _mil_scale(global_step):
    if cfg.TRAIN.WS_LOSS_USE_ADAPTIVE_SCALE_FACTOR:
        return 1.0 - 0.99 * (0.9 ** (int(global_step) // 2000))       # exponential_decay, staircase
    return cfg.TRAIN.WS_LOSS_SCALE_FACTOR


_prior_cache = {}


def _class_prior(like):
    """[0, WS_MAL_PCT, 1 - WS_MAL_PCT] on like's device (train_bus.py:252,664), built once: a tensor
    made from a Python list is a blocking host->device copy."""
    key = (float(cfg.TRAIN.WS_MAL_PCT), str(like.device), like.dtype)
    t = _prior_cache.get(key)
    if t is None:
        t = torch.tensor([0.0, key[0], 1 - key[0]], dtype=like.dtype, device=like.device)
        _prior_cache[key] = t
    return t


def l2_weight_decay(params):
    """train_bus.py:268-270: sum(l2_loss(w)) * WEIGHT_DECAY over '*weights' variables."""
    if not params:
        return 0.0
    k = 0.5 * cfg.TRAIN.WEIGHT_DECAY
    if _plumbing.l2decay_usable(params):
        # every parameter in one device op (csrc/plumbing/l2decay.hip): same gradients bit for bit, the value an
        # f64 sum rounded once
        return _plumbing.l2_decay(params, k)
    return torch.stack([(p * p).sum() for p in params]).sum() * k


def supervised_loss(layers, params, n_sup=None):
    # (the device op takes 2 <= K <= 32 classes; wider heads take the torch chain)
    if cfg.get('FUSED_LOSS', True) and layers['cls_score'].is_cuda and 'rpn_cls_score' in layers \
            and 2 <= layers['cls_score'].shape[1] <= 32:
        # the four terms and their gradients as one device op (csrc/loss.hip)
        from .loss_op import multi_task_loss, TERMS
        terms = multi_task_loss(layers['rpn_cls_score'], layers['rpn_bbox_pred'], layers['cls_score'],
                                layers['bbox_pred'], layers['rpn-data'], layers['roi-data'], n_sup)
        l = {name: terms[i] for i, name in enumerate(TERMS)}
    else:
        l = dict(
            rpn_cross_entropy=rpn_cls_loss(layers['rpn_cls_score_reshape'], layers['rpn-data'][0]),
            rpn_loss_box=rpn_box_loss(layers['rpn_bbox_pred'], layers['rpn-data'], n_sup),
            cross_entropy=rcnn_cls_loss(layers['cls_score'], layers['roi-data'][1]),
            loss_box=rcnn_box_loss(layers['bbox_pred'], layers['roi-data']),
        )
    l['weight_decay'] = l2_weight_decay(params)
    l['loss'] = (l['cross_entropy'] + l['loss_box'] + l['rpn_cross_entropy'] + l['rpn_loss_box']
                 + l['weight_decay'])
    return l


# ------------------------------------------------------------- validation ---

# the reference's test_loss vector (train_bus.py:519-520): the total first
VAL_TERMS = ('total', 'rpn_cross_entropy', 'rpn_loss_box', 'cross_entropy', 'loss_box', 'mil_cross_entropy')


def _mil_per_image(cls_score, image_column, mil_label, n_images, global_step, funcs):
    """[n_images]: mil_loss of every image as ONE bag of its own rows (n_bags = 1 each)."""
    scale = _mil_scale(global_step)
    if cls_score.is_cuda and cfg.get('FUSED_LOSS', True) and 3 <= cls_score.shape[1] <= 8:
        # one call of the fused op with bags = images; its per-bag output times the scale, rounded as the op's
        # own finish rounds a mean over one bag: (f32)((f64)(f32)scale * bag_loss)
        prior = [0.0, float(cfg.TRAIN.WS_MAL_PCT), 1.0 - float(cfg.TRAIN.WS_MAL_PCT)]
        bag = mil_core.mil_bag_losses_device(cls_score, image_column, 0.0, mil_label, n_images, funcs, prior)
        return (bag.double() * float(np.float32(scale))).float()
    out = []
    for i in range(n_images):
        rows = (image_column == i).nonzero().reshape(-1)
        if rows.numel() == 0:                          # an empty bag carries no loss (as in the fused op)
            out.append(cls_score.new_zeros(()))
            continue
        out.append(mil_loss(cls_score[rows], cls_score.new_zeros((rows.numel(),)), mil_label[i:i + 1], 1, global_step,
                            funcs, counts_host=[int(rows.numel())]))
    return torch.stack(out).float()


def default_mil_funcs(alter):
    """The reference's own pair (for bags labelled 1, for the others): [mass-max, mal-max] in the alternating wiring
    (train_bus.py:241), [mal-max, mal-max] in the combined one (:655)."""
    return [mil_core.get_mass_max_logit, mil_core.get_mal_max_logit] if alter \
        else [mil_core.get_mal_max_logit, mil_core.get_mal_max_logit]


@torch.no_grad()
def validation_losses(layers, im_info, n_images, global_step, alter, funcs=None):
    """The loss half of the reference's validation pass (train_bus.py:427-534 alternating, :792-899 combined) for
    the N = n_images images of ONE forward: a pure function of that forward's `layers` (run with
    is_training=False, is_ws=False).  -> dict of [N] f32 tensors on the layers' device, nothing read back:

      rpn_cross_entropy, rpn_loss_box, cross_entropy, loss_box
                          image i's four supervised terms, as supervised_loss gives them for a batch holding that
                          image alone (loss_op.multi_task_loss_per_image: one device launch for all images);
      total               their sum, the reference's test_loss[0] (:519): no weight decay, no MIL term -- what the
                          plateau schedule is fed;
      mil_cross_entropy   mil_loss of image i as one bag of its own roi-data rows, bag label im_info[i, 3], class
                          prior and scale factor of mil_loss at `global_step`, selectors [get_mass_max_logit,
                          get_mal_max_logit] when `alter` else [get_mal_max_logit, get_mal_max_logit] -- or the
                          pair `funcs` (for bags labelled 1, for the others) of mil.core's bag functions.

    For the alternating wiring the MIL slot is the reference's value (:239-260 under the feed of :436-438).  For the
    combined wiring it is UNPINNED: the reference's graph slices the rows past len(label) (:650-653), of which a
    validation batch has none, and what TensorFlow then yields for an arg-max over no rows could not be observed;
    the slot holds the per-image bag loss defined above instead."""
    from .loss_op import multi_task_loss_per_image, TERMS
    n = int(n_images)
    losses, _ = multi_task_loss_per_image(layers['rpn_cls_score'], layers['rpn_bbox_pred'], layers['cls_score'],
                                          layers['bbox_pred'], layers['rpn-data'], layers['roi-data'], n)
    out = {name: losses[:, i] for i, name in enumerate(TERMS)}
    out['total'] = out['rpn_cross_entropy'] + out['rpn_loss_box'] + out['cross_entropy'] + out['loss_box']   # :519
    rois = layers['roi-data'][0]
    if funcs is None:
        funcs = default_mil_funcs(alter)
    out['mil_cross_entropy'] = _mil_per_image(layers['cls_score'][:rois.shape[0]], rois[:, 0],
                                              im_info[:n, 3].to(torch.int32), n, global_step, funcs)
    return out


# ------------------------------------------------------------ train steps ---

class SolverWrapper(object):
    """The part of the reference's SolverWrapper (train_bus.py:97-131) that a step needs: the network, the
    optimiser, the learning-rate schedule, the global step, and -- new in this implementation -- gradient
    averaging across data-parallel ranks.

    opt: None (the default) is torch.optim.Adam(lr, eps=0.1).  That is NOT the reference's Adam: torch adds eps to
    sqrt(v) / sqrt(1 - b2^t), TensorFlow to sqrt(v), and with eps = 0.1 above most gradients torch's first step is
    about 30 times TF's (fast_rcnn/optim.py).  It stays the default because the benchmark and every golden step
    measure it; flipping it is a separate decision.  'adam', 'amsgrad' and 'sgd' are the reference's `--opt`
    choices (:286-294, :694-697) in TF's arithmetic, one HIP launch per step (optim.ReferenceOptimizer); 'sgd'
    reads cfg.TRAIN.MOMENTUM.  'amsgrad' is UNPINNED: the reference's module is not in its tree.

    lr_scheduling: 'const'; 'pc', 0.1 * lr once the global step has passed int(0.75 * max_iters) (:276-279; needs
    max_iters); 'rop', optim.ReduceLROnPlateau fed by on_val_end(val_loss) (:281).  The current rate is written
    into whichever optimiser takes the step, right before it.

    Alternating mode under 'sgd': the reference's supervised op is minimize(loss, global_step=global_step) (:293),
    so BOTH halves of an iteration count the global step (two per iteration); under the other optimisers only the
    weak half does.  The MIL scale factor 1 - 0.99 * 0.9^floor(step / 2000) and the 'pc' schedule read that count,
    so this is reproduced.

    mil_funcs: the bag functions of the MIL term, a pair (for bags labelled 1, for the others) like the reference's
    `funcs` (:241, :655), each one of mil.core's five functions or its name in mil.core.MIL_FUNCS ('mal_max',
    'ben_max', 'mass_max', 'disc_max', 'mean_ben').  None keeps the reference's wiring-specific pairs: [mass_max,
    mal_max] in the weak half of an alternating iteration, [mal_max, mal_max] in a combined step, and the matching
    one in validate.  A given pair is used by joint_backward, weak_backward and validate alike.  It is a constructor
    argument like `opt`: snapshots do not store it, a resumed run passes it again."""

    OPTS = (None, 'adam', 'amsgrad', 'sgd')
    SCHEDULES = ('const', 'pc', 'rop')

    def __init__(self, network, lr=None, dist_ctx=None, opt=None, lr_scheduling='const', max_iters=None, *,
                 mil_funcs=None):
        if opt not in self.OPTS:
            raise ValueError("opt=%r: one of %r" % (opt, self.OPTS))
        if lr_scheduling not in self.SCHEDULES:
            raise ValueError("lr_scheduling=%r: one of %r" % (lr_scheduling, self.SCHEDULES))
        if lr_scheduling == 'pc' and max_iters is None:
            raise ValueError("lr_scheduling='pc' needs max_iters")
        self.mil_funcs = None if mil_funcs is None else mil_core.resolve_funcs(mil_funcs)
        self.net = network
        self.lr = cfg.TRAIN.get('LEARNING_RATE', 0.0005) if lr is None else lr
        self.opt, self.lr_scheduling, self.max_iters = opt, lr_scheduling, max_iters
        self.rop = None
        if lr_scheduling == 'rop':
            self.rop = optim.ReduceLROnPlateau(self.lr, factor=0.5, patience=5, mode='min', epsilon=1e-3,
                                               cooldown=0, min_lr=0)
        self.params = [p for p in network.parameters() if p.requires_grad]
        # combined mode: ONE Adam applies the summed gradients and counts the global step
        # (:694-705).  Alternating mode: the supervised op is Adam.minimize(loss) WITHOUT a
        # global step, the weak op a SECOND Adam whose apply_gradients counts it (:286-301);
        # the two keep their own moments and bias-correction powers.  (Likewise for every `opt`.)
        self.optimizer = self._make_optimizer()
        self.optimizer_ws = None                  # created by the first alternating iteration
        self.global_step = 0
        self.dist = dist_ctx
        if dist_ctx is not None and dist_ctx.enabled:
            # seed per rank = seed + rank, for the device samplers too; a single
            # process keeps the DEVICE_RNG_SEED its caller set
            if getattr(dist_ctx, "_device_seed_base", None) is None:
                dist_ctx._device_seed_base = int(cfg.DEVICE_RNG_SEED)      # a second solver on this context
            cfg.DEVICE_RNG_SEED = dist_ctx.seed(dist_ctx._device_seed_base)   # does not add the rank again
        # data parallel: bucketed gradient all-reduce overlapped with backward
        self.overlap = dist_ctx.overlap(self.params) if (dist_ctx is not None and dist_ctx.enabled) else None

    def _adam(self):
        # plumbing: on the GPU ask for the multi-tensor ("fused") implementation -- the per-parameter
        # loop is ~7 small launches for each of ~160 parameters per step
        fused = bool(self.params) and all(p.is_cuda for p in self.params) and os.environ.get("WSSDL_ADAM_FUSED", "1") != "0"
        return torch.optim.Adam(self.params, lr=self.lr, eps=0.1, fused=True) if fused \
            else torch.optim.Adam(self.params, lr=self.lr, eps=0.1)

    def _make_optimizer(self):
        return self._adam() if self.opt is None else optim.make(self.opt, self.params, self.lr)

    def current_lr(self):
        """The learning rate of the step about to be taken (train_bus.py:338-344, :739-745)."""
        if self.lr_scheduling == 'pc':
            return optim.piecewise_lr(self.lr, self.global_step, self.max_iters)
        if self.lr_scheduling == 'rop':
            return self.rop.get_cur_lr()
        return self.lr

    def on_val_end(self, val_loss):
        """After a validation pass: feeds the 'rop' schedule (train_bus.py:70-91); nothing under the others."""
        if self.rop is not None:
            self.rop.on_val_end(val_loss)

    def validate(self, blobs_iter, feed_schedule=True, *, gt_roidb=None, classes=None, im_shapes=None, thresh=0.05,
                 max_per_image=300, ovthresh=0.5, score_thresh=0.5):
        """The loss half of the reference's validation pass (train_bus.py:427-534 / :792-899): the training wiring
        on validation images with is_training=False, their six loss values averaged over the set and the total
        handed to the plateau schedule (:519-534).  The reference runs one image per step; here every element of
        `blobs_iter` -- a blob dict as the train steps take them: data [n,H,W,3], im_info [n,4], gt_boxes,
        num_gt_boxes, any n >= 1, not the same for every element -- is ONE forward in eval mode under no_grad, and
        validation_losses gives the per-image values of its n images.  They stay on the device; the single
        read-back comes at the end of the pass.

        -> dict: the means over all images under VAL_TERMS' names ('total' first, the order of :519-520),
        'n_images', and 'per_image', a [n_images, 6] numpy array in that column order.  With feed_schedule the
        mean total goes to on_val_end: under 'rop' the next current_lr() follows the plateau rule, under the
        other schedules nothing happens.

        Nothing else moves: optimisers, parameters, running statistics, renorm state and global_step are as
        before (eval mode updates no buffer), the network's training flag is restored, and so is
        cfg.TRAIN.IMS_PER_BATCH, which the combined wiring's target layers read and which is therefore set to
        each element's n during its forward -- both also when a forward raises.  Under cfg.SAMPLING_RNG =
        'reference' the target layers draw from the global NumPy stream exactly as the reference's own
        validation forward does (they sample under is_training=False too): per forward all anchor subsamples,
        image by image, then all RoI samples; a caller who needs the training draws unchanged saves and
        restores np.random's state around the pass.  The deferred device flags are polled at the end, as after a
        train step.

        The reference also scores CorLoc on the sampled RoIs of the same forward (:445-527 / :810-892).  With
        gt_roidb=None (the default) that half does not run: arguments, return value, launches and RNG draws are
        those of the loss half alone.  With a gt_roidb -- one entry per validation image in pass order, in
        original-image pixels, in datasets.voc_eval_bus.pack_gt's format -- every forward's layers also go through
        val_detect.validation_detections (decode and clip of the sampled RoIs in one launch, then the batched
        post-detection op under `thresh`, cfg.TEST.NMS, cfg.TEST.CLS_AGNOSTIC_NMS and `max_per_image`), the result is
        added to a DetectionAccumulator at the running image index, and after the loss read-back ONE
        evaluate_detections call (ovthresh, score_thresh; classes: the names, '__background__' first, default
        numbered) scores the whole pass: two read-backs in total.  The dict then also holds 'corloc_list', 'aps',
        'mean_ap', 'froc_curve_pts' (evaluate_detections) and 'detections', the accumulator.  im_shapes: the
        original (H, W) of every image in pass order, to clip to as the reference does (im.shape); without it boxes
        are clipped to (w / scale - 1, h / scale - 1) of im_info.  A gt_roidb or im_shapes whose length is not the
        pass's image count raises ValueError.  The detection half draws nothing from any RNG and changes no state.
        eval_batch.evaluate_images remains the test protocol (a forward of its own, 300 proposals).
        The MIL column of the combined wiring is UNPINNED (validation_losses)."""
        alter = bool(getattr(self.net, 'alter', False))
        chunks = []
        detect = gt_roidb is not None
        acc, seen = None, 0
        if detect:
            from ..datasets.voc_eval_bus import DetectionAccumulator, evaluate_detections
            from .val_detect import validation_detections
        was_training = self.net.training
        ims_per_batch = cfg.TRAIN.IMS_PER_BATCH
        try:
            self.net.eval()
            with torch.no_grad():
                for blobs in blobs_iter:
                    n = int(blobs['data'].shape[0])
                    cfg.TRAIN.IMS_PER_BATCH = n
                    layers = self.net(blobs['data'], blobs['im_info'], blobs['gt_boxes'], blobs['num_gt_boxes'],
                                      is_training=False, is_ws=False)
                    v = validation_losses(layers, blobs['im_info'], n, self.global_step, alter, self.mil_funcs)
                    chunks.append(torch.stack([v[name] for name in VAL_TERMS], dim=1))
                    if detect:
                        shapes = None
                        if im_shapes is not None:
                            shapes = im_shapes[seen:seen + n]
                            if len(shapes) != n:
                                raise ValueError("validate: im_shapes names %d images, the pass holds more" % len(im_shapes))
                        dets, counts = validation_detections(layers, blobs['im_info'], n, thresh, max_per_image, shapes)
                        if acc is None:
                            acc = DetectionAccumulator(int(dets.shape[1]) + 1)
                        acc.add(dets, counts, seen)
                    seen += n
        finally:
            cfg.TRAIN.IMS_PER_BATCH = ims_per_batch
            self.net.train(was_training)
        if not chunks:
            raise ValueError("validate: no validation images")
        per_image = torch.cat(chunks, dim=0).cpu().numpy()             # the one read-back of the pass
        roi_pooling_op.poll_flags()
        means = per_image.astype(np.float64).mean(axis=0)
        out = {name: float(means[i]) for i, name in enumerate(VAL_TERMS)}
        out['n_images'] = int(per_image.shape[0])
        out['per_image'] = per_image
        if detect:
            if len(gt_roidb) != seen:
                raise ValueError("validate: gt_roidb has %d entries, the pass held %d images" % (len(gt_roidb), seen))
            if im_shapes is not None and len(im_shapes) != seen:
                raise ValueError("validate: im_shapes names %d images, the pass held %d" % (len(im_shapes), seen))
            if classes is None:
                classes = ['__background__'] + ['class_%d' % j for j in range(1, acc.num_classes)]
            if len(classes) != acc.num_classes:
                raise ValueError("the network scores %d classes, `classes` names %d" % (acc.num_classes, len(classes)))
            ev = evaluate_detections(acc, gt_roidb, classes, ovthresh, score_thresh)
            for name in ('corloc_list', 'aps', 'mean_ap', 'froc_curve_pts'):
                out[name] = ev[name]
            out['detections'] = acc
        if feed_schedule:
            self.on_val_end(out['total'])
        return out

    def _apply(self, optimizer=None, count_step=True):
        optimizer = optimizer or self.optimizer
        if self.lr_scheduling != 'const':
            for group in optimizer.param_groups:
                group['lr'] = self.current_lr()
        if self.overlap is not None:
            self.overlap.finish()
        elif self.dist is not None:
            self.dist.allreduce_gradients(self.params)
        roi_pooling_op.poll_flags()               # deferred error flags of the RoI-pool pair: no read-back
        optimizer.step()                          # parameters whose grad is None are skipped,
        self.optimizer.zero_grad(set_to_none=True)  # like apply_gradients with a None gradient
        if count_step:
            self.global_step += 1

    def check_flags(self):
        """Synchronising look at the deferred device flags (RoI-pool overflow, NMS time-out).  The poll in
        _apply runs one step late -- by the time it raises, the optimiser has already applied the step before
        it, so the parameters of that step are tainted -- and it never sees the last step.  The package calls this
        before every snapshot (snapshot.save_snapshot: a raised flag means no file is written) and at the end of
        training (train_loop); a caller who saves parameters by other means calls it first."""
        roi_pooling_op.check_flags()

    def joint_backward(self, blobs):
        """Forward + backward of one combined mini-batch (train_bus.py:732-764): supervised images
        first, weak images after; the supervised and MIL gradients are summed per variable
        (:701-705), which is the gradient of (loss + mil_cross_entropy).  Gradients are left in
        .grad (and, under data parallelism, their all-reduce is in flight)."""
        n_s = int(cfg.TRAIN.IMS_PER_BATCH)
        n_ws = int(cfg.TRAIN.WS_IMS_PER_BATCH)
        layers = self.net(blobs['data'], blobs['im_info'], blobs['gt_boxes'], blobs['num_gt_boxes'],
                          is_training=True, is_ws=False)
        losses = supervised_loss(layers, self.net.weight_decay_params(), n_s)
        n_valid = layers['roi-data'][1].numel()                       # len(label), :624-628
        cls_ws = layers['cls_score'][n_valid:]
        batch_inds = layers['roi-data'][0][n_valid:, 0] - n_s         # :653
        mil_label = blobs['im_info'][n_s:, 3].to(torch.int32)         # image-level labels, :654
        funcs = self.mil_funcs or default_mil_funcs(False)            # :655
        losses['mil_cross_entropy'] = mil_loss(cls_ws, batch_inds, mil_label, n_ws,
                                               self.global_step, funcs)
        (losses['loss'] + losses['mil_cross_entropy']).backward()
        return losses

    def train_step_joint(self, blobs):
        """One combined optimiser step: joint_backward, then Adam on the (averaged) gradients."""
        losses = self.joint_backward(blobs)
        self._apply()
        return losses

    def supervised_backward(self, blobs_s):
        """The supervised half of an alternating iteration (train_bus.py:334-360)."""
        layers = self.net(blobs_s['data'], blobs_s['im_info'], blobs_s['gt_boxes'],
                          blobs_s['num_gt_boxes'], is_training=True, is_ws=False)
        losses = supervised_loss(layers, self.net.weight_decay_params())
        losses['loss'].backward()
        return losses

    def weak_backward(self, blobs_ws):
        """The weak half (train_bus.py:362-394): the MIL loss alone, with is_ws=True."""
        layers = self.net(blobs_ws['data'], blobs_ws['im_info'], blobs_ws['gt_boxes'],
                          blobs_ws['num_gt_boxes'], is_training=True, is_ws=True)
        batch_inds = layers['roi-data'][0][:, 0]                      # :239
        mil_label = blobs_ws['im_info'][:, 3].to(torch.int32)         # :240
        funcs = self.mil_funcs or default_mil_funcs(True)             # :241
        mil = mil_loss(layers['cls_score'], batch_inds, mil_label, blobs_ws['data'].shape[0],
                       self.global_step, funcs)
        mil.backward()
        return mil

    def train_step_alter(self, blobs_s, blobs_ws):
        """One alternating iteration (train_bus.py:334-394): a supervised step on `loss`, then
        a weak step on the MIL loss alone with is_ws=True."""
        losses = self.supervised_backward(blobs_s)
        # train_op_s: no global_step -- except under 'sgd', whose minimize() is given it (:293)
        self._apply(self.optimizer, count_step=self.opt == 'sgd')
        losses['mil_cross_entropy'] = self.weak_backward(blobs_ws)
        if self.optimizer_ws is None:
            self.optimizer_ws = self._make_optimizer()
        self._apply(self.optimizer_ws, count_step=True)            # train_op_ws counts the step
        return losses


def get_training_roidb(imdb):
    """imdb.roidb made ready for the data layers: the mirrored twins appended when cfg.TRAIN.USE_FLIPPED, then the keys
    of roi_data_layer.roidb.prepare_roidb."""
    from ..roi_data_layer import roidb as rdl_roidb
    if cfg.TRAIN.USE_FLIPPED:
        imdb.append_flipped_images()
    if cfg.TRAIN.HAS_RPN and cfg.IS_MULTISCALE:
        raise NotImplementedError
    rdl_roidb.prepare_roidb(imdb)
    return imdb.roidb


def get_test_roidb(imdb):
    """imdb.roidb for the validation / test pass (reference fast_rcnn/test_bus.py:416-430): prepare_roidb's keys, no
    mirrored twins."""
    from ..roi_data_layer import roidb as rdl_roidb
    if cfg.TRAIN.HAS_RPN and cfg.IS_MULTISCALE:
        raise NotImplementedError
    rdl_roidb.prepare_roidb(imdb)
    return imdb.roidb


def get_data_layer(roidbs, net_name, num_classes, is_training, is_ws=False, is_joint=False):
    """RoIDataLayerJoint over roidbs = (roidb_s, roidb_ws) when is_joint, else RoIDataLayer over the one roidb."""
    from ..roi_data_layer.layer_bus import RoIDataLayer
    from ..roi_data_layer.layer_bus_joint import RoIDataLayerJoint
    if not cfg.TRAIN.HAS_RPN:
        raise NotImplementedError("only the cfg.TRAIN.HAS_RPN branch of the data layers exists")
    if cfg.IS_MULTISCALE:
        raise NotImplementedError
    if is_joint:
        return RoIDataLayerJoint(roidbs[0], roidbs[1], net_name, num_classes, is_training)
    return RoIDataLayer(roidbs, net_name, num_classes, is_training, is_ws)


def train_net(network, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test, output_dir,
              pretrained_model=None, max_iters=80000, s_start_iter=0, s_end_iter=80000, ws_start_iter=0, ws_end_iter=80000,
              opt='adam', lr=5e-4, lr_scheduling='const', vis=False, *, resume=None, dist_ctx=None, val_ims_per_batch=1,
              max_per_image=300, thresh=0.05, mil_funcs=None):
    """Train a Faster R-CNN using combined mini-batches from supervised and weakly supervised sets (train_bus.py:1073-1087,
    without the TensorFlow session): SolverWrapper(network, lr, dist_ctx, opt, lr_scheduling, max_iters), then
    train_loop.train_model.  opt='adam' is the reference's TF-form Adam, as its command line has it (SolverWrapper's own
    default opt=None is another optimiser).  pretrained_model: a snapshot written by this package or a torch state_dict
    file, loaded non-strictly before the first step, the missing names printed; the reference's .npy layout of
    TensorFlow variables is out of scope.  resume: a snapshot to continue from (fast_rcnn/snapshot.py).  vis: the
    validation pass's pictures go to <output_dir>/test (fast_rcnn/vis.py).  val_ims_per_batch: images per validation
    forward.  mil_funcs: the MIL term's pair of bag functions or names (SolverWrapper; None: the reference's pair; not
    stored in snapshots).  Returns train_loop's history dict."""
    from . import train_loop
    return train_loop._train(False, network, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test,
                             output_dir, pretrained_model, max_iters, (s_start_iter, s_end_iter, ws_start_iter, ws_end_iter), opt, lr,
                             lr_scheduling, vis, resume, dist_ctx, val_ims_per_batch, max_per_image, thresh, mil_funcs)


def train_net_alter(network, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test, output_dir,
                    pretrained_model=None, max_iters=80000, s_start_iter=0, s_end_iter=80000, ws_start_iter=0, ws_end_iter=80000,
                    opt='adam', lr=5e-4, lr_scheduling='const', vis=False, *, resume=None, dist_ctx=None, val_ims_per_batch=1,
                    max_per_image=300, thresh=0.05, mil_funcs=None):
    """Train a Faster R-CNN using alternating mini-batches each from supervised and weakly supervised sets
    (train_bus.py:1055-1069): as train_net, over train_loop.train_model_alter."""
    from . import train_loop
    return train_loop._train(True, network, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test,
                             output_dir, pretrained_model, max_iters, (s_start_iter, s_end_iter, ws_start_iter, ws_end_iter), opt, lr,
                             lr_scheduling, vis, resume, dist_ctx, val_ims_per_batch, max_per_image, thresh, mil_funcs)
