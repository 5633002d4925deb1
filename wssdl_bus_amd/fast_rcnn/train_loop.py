"""The training loops: the reference's SolverWrapper.train_model (joint, fast_rcnn/train_bus.py:595-958) and
train_model_alter (alternating, :175-593) over this package's data layers, train steps, validation pass, snapshots
(fast_rcnn/snapshot.py) and device-drawn qualitative results (fast_rcnn/vis.py).

Per iteration, in the reference's order: the train step(s); the running training losses; every cfg.TRAIN.DISPLAY
iterations the three status lines (:415-421); every cfg.TRAIN.SNAPSHOT_ITERS a snapshot; every cfg.TRAIN.TEST_ITERS one
validation pass over the whole test roidb (SolverWrapper.validate with gt_roidb: losses, CorLoc, AP and FROC from one
forward per batch), the record appended to <output_dir>/log.txt (the text of :573-583) and, as one JSON line holding
the reference's summary tags plus 'iter', to <output_dir>/summary.jsonl -- there is no TensorBoard writer here -- and
with `vis` the pass's pictures to <output_dir>/test/<image basename>.png.  One more snapshot at the end if the last
iteration took none (:589).

Running training losses: the six values (total = the sum of the four supervised terms, rpn_cls, rpn_box, cls, box,
mil) are summed in f64 ON THE DEVICE, one small op per iteration and no read-back; they come back to the host only at
a DISPLAY, TEST_ITERS or final boundary.  At a TEST_ITERS boundary they are divided by cfg.TRAIN.TEST_ITERS (:529),
reported and zeroed.  A half of an alternating iteration that is skipped contributes the reference's stand-in values
(:362-366, :395-399): the previous interval's means, or -log(1 / num_classes) while the previous MIL mean is 0; being
host constants they are summed on the host and joined at the boundary.

log.txt: the reference writes str() of NumPy f64 scalars under Python 2 (12 significant digits); here the same lines
carry Python 3's str(float), the shortest text that reads back to the same f64.

Multi-rank runs (dist_ctx): only rank 0 writes files, validates and renders; every rank takes the same number of
steps.  A resumed multi-rank run restores the shared state on every rank; the data cursors and generators of
ranks > 0 restart from seed + rank (fast_rcnn/snapshot.py).
"""
import json
import os
import time

import numpy as np
import torch

from . import snapshot as snap
from .config import cfg

TRAIN_TAGS = ('training_loss_total', 'training_loss_rpn_loss_cls', 'training_loss_rpn_loss_box', 'training_loss_loss_cls',
              'training_loss_loss_box', 'training_loss_mil_loss_cls')
TEST_TAGS = ('test_loss_total', 'test_loss_rpn_loss_cls', 'test_loss_rpn_loss_box', 'test_loss_loss_cls',
             'test_loss_loss_box', 'test_loss_mil_loss_cls')
CORLOC_TAGS = ('corloc for benign', 'corloc for malignant', 'corloc')
SUP_TERMS = ('rpn_cross_entropy', 'rpn_loss_box', 'cross_entropy', 'loss_box')


def log_record(iteration, max_iters, training_loss, test_loss, cur_lr):
    """The text train_bus.py:573-583 appends to log.txt for one validation (iteration 0-based)."""
    tr, te = [float(v) for v in training_loss], [float(v) for v in test_loss]

    def block(v):
        return ('total_loss: ' + str(v[0]) + '\n' + 'rpn_loss_cls: ' + str(v[1]) + '\trpn_loss_box: ' + str(v[2]) + '\tloss_cls: ' +
                str(v[3]) + '\tloss_box: ' + str(v[4]) + '\n' + 'mil_loss_cls: ' + str(v[5]) + '\n')
    return ('iter: ' + str(iteration + 1) + ' / ' + str(max_iters) + '\n' + 'training loss' + '\n' + block(tr) + 'test loss' + '\n' +
            block(te) + 'lr: ' + str(float(cur_lr)) + '\n')


def summary_record(iteration, training_loss, test_loss, corloc_list, cur_lr):
    """The reference's summary tags (:537-552) as one dict, plus 'iter'."""
    rec = {'iter': int(iteration) + 1}
    rec.update({k: float(v) for k, v in zip(TRAIN_TAGS, training_loss)})
    rec.update({k: float(v) for k, v in zip(TEST_TAGS, test_loss)})
    rec.update({k: float(v) for k, v in zip(CORLOC_TAGS, corloc_list)})
    rec['lr'] = float(cur_lr)
    return rec


class RunningLosses(object):
    """The loop's six running sums.  add() takes device scalars (or None for a skipped part, with its host stand-in)
    and reads nothing back; sums() is the one read-back."""

    def __init__(self):
        self.device_sums = None             # [6] f64 on the losses' device
        self.host_sums = np.zeros(6, np.float64)
        self.last = None                    # the last iteration's six values: ([6] device tensor or None, [6] host)
        self.old_means = np.zeros(6, np.float64)

    def add(self, sup_terms, mil, standins):
        """sup_terms: the four supervised device scalars or None; mil: the MIL device scalar or None; standins [6]:
        host values used where a part is None."""
        host = np.zeros(6, np.float64)
        parts = []
        like = sup_terms[0] if sup_terms is not None else mil
        if sup_terms is not None:
            four = torch.stack([t.detach().reshape(()) for t in sup_terms]).double()
            parts = [(four[0] + four[1] + four[2] + four[3]).reshape(1), four]     # the reference's a + b + c + d, in f64
        else:
            host[1:5] = standins[1:5]
            host[0] = standins[1] + standins[2] + standins[3] + standins[4]
        if mil is None:
            host[5] = standins[5]
        dev = None
        if like is not None:
            zero4 = like.detach().new_zeros((5,), dtype=torch.float64)
            head = torch.cat(parts) if sup_terms is not None else zero4
            tail = mil.detach().reshape(1).double() if mil is not None else like.detach().new_zeros((1,), dtype=torch.float64)
            dev = torch.cat([head, tail])
            self.device_sums = dev if self.device_sums is None else self.device_sums + dev
        self.host_sums += host
        self.last = (dev, host)

    def sums(self):
        out = self.host_sums.copy()
        if self.device_sums is not None:
            out += self.device_sums.cpu().numpy()
        return out

    def last_values(self):
        dev, host = self.last
        return host + (dev.cpu().numpy() if dev is not None else 0.0)

    def close_interval(self, n):
        """The means over the interval (sums / n), kept as the next interval's stand-ins; the sums start again."""
        means = self.sums() / n
        self.old_means = means
        self.device_sums, self.host_sums = None, np.zeros(6, np.float64)
        return means

    def standins(self, num_classes):
        s = self.old_means.copy()
        if s[5] == 0:
            s[5] = -np.log(1. / num_classes)
        return s

    def state_dict(self):
        return dict(sums=self.sums(), old_means=self.old_means.copy())

    def load_state_dict(self, state):
        self.device_sums, self.host_sums = None, np.array(state['sums'], dtype=np.float64)
        self.old_means = np.array(state['old_means'], dtype=np.float64)


def _is_writer(solver):
    d = getattr(solver, 'dist', None)
    return d is None or not getattr(d, 'enabled', False) or d.rank == 0


def _test_pass(solver, imdb_test, roidb_test, net_name, val_ims_per_batch, thresh, max_per_image, vis, output_dir):
    """One validation pass over the whole test roidb: the blobs of val_ims_per_batch images per forward, gt_roidb and
    im_shapes from the roidb in pass order (what a RoIDataLayer with is_training=False hands out -- arange order, no
    draws -- without its wrap-around, so the last forward may hold fewer images).  With `vis` the detections are drawn
    on the device and written as PNGs."""
    from ..roi_data_layer.minibatch_bus import entry_plane, plan_blobs, plan_minibatch
    n = len(roidb_test)
    planes = [entry_plane(e) for e in roidb_test] if vis else None

    def blobs_iter():
        for b0 in range(0, n, val_ims_per_batch):
            entries = roidb_test[b0:b0 + val_ims_per_batch]
            pl = planes[b0:b0 + val_ims_per_batch] if planes is not None else None
            yield plan_blobs(plan_minibatch(entries, net_name, imdb_test.num_classes, False, False, planes=pl))
    gt_roidb = [dict(boxes=e['boxes'], gt_classes=e['gt_classes']) for e in roidb_test]
    im_shapes = [(int(e['height']), int(e['width'])) for e in roidb_test]
    result = solver.validate(blobs_iter(), gt_roidb=gt_roidb, classes=imdb_test.classes, im_shapes=im_shapes, thresh=thresh,
                             max_per_image=max_per_image)
    if vis:
        from . import vis as V
        images = V.draw_detections(planes, gt_roidb, result['detections'], imdb_test.classes)
        paths = V.qualitative_paths(os.path.join(output_dir, 'test'), [imdb_test.image_path_at(i) for i in range(n)])
        V.save_qualitative(images, paths)
    return result


def _print_validation(iteration, max_iters, tr, te, corloc, cur_lr):
    print('iter: %d / %d' % (iteration + 1, max_iters))
    print('training loss')
    print('total_loss: %.4f' % tr[0])
    print('rpn_loss_cls: %.4f, rpn_loss_box: %.4f, loss_cls: %.4f, loss_box: %.4f, mil_loss_cls: %.4f' % tuple(tr[1:6]))
    print('test loss')
    print('total_loss: %.4f' % te[0])
    print('rpn_loss_cls: %.4f, rpn_loss_box: %.4f, loss_cls: %.4f, loss_box: %.4f, mil_loss_cls: %.4f' % tuple(te[1:6]))
    print('corloc for benign: %.4f, corloc for malignant: %.4f, corloc: %.4f' % tuple(corloc[:3]))
    print('lr: %.8f' % cur_lr)


def _run(solver, alter, layers, imdb_train_ws, imdb_test, roidb_test, output_dir, net_name, max_iters, windows, vis, resume,
         val_ims_per_batch, max_per_image, thresh, test_pass=None):
    s_start, s_end, ws_start, ws_end = windows
    writer = _is_writer(solver)
    test_pass = test_pass or _test_pass
    running = RunningLosses()
    history = dict(validations=[], snapshots=[], final_losses=None)
    start_iter, elapsed, timed = 0, 0.0, 0
    if resume is not None:
        start_iter, loop = snap.restore(resume, solver, layers, rank_local=writer)
        running.load_state_dict(loop['running'])
        elapsed, timed = float(loop.get('elapsed', 0.0)), int(loop.get('timed', 0))
    if writer:
        os.makedirs(output_dir, exist_ok=True)
        if vis:
            os.makedirs(os.path.join(output_dir, 'test'), exist_ok=True)
        f_log = open(os.path.join(output_dir, 'log.txt'), 'a' if resume is not None else 'w')
        f_sum = open(os.path.join(output_dir, 'summary.jsonl'), 'a' if resume is not None else 'w')
    last_snapshot_iter, it, cur_lr = start_iter - 1, start_iter - 1, solver.current_lr()
    pending = False
    if resume is not None:
        cur_lr, pending = float(loop.get('cur_lr', cur_lr)), bool(loop.get('pending_validation', False))

    def take_snapshot(iteration, validating):
        if writer:
            # a snapshot taken at a validating iteration precedes the pass, as in the reference (:423-427): it says so,
            # and a run resumed from it validates first
            state = dict(running=running.state_dict(), elapsed=elapsed, timed=timed, cur_lr=float(cur_lr),
                         pending_validation=bool(validating))
            history['snapshots'].append(snap.save_snapshot(solver, output_dir, net_name, iteration, state, layers))

    def validate_at(iteration):                                                      # :427-587
        tr = running.close_interval(cfg.TRAIN.TEST_ITERS)                            # :529
        total = 0.0
        if writer:
            result = test_pass(solver, imdb_test, roidb_test, net_name, val_ims_per_batch, thresh, max_per_image, vis, output_dir)
            total = result['total']
            te = [result['total'], result['rpn_cross_entropy'], result['rpn_loss_box'], result['cross_entropy'],
                  result['loss_box'], result['mil_cross_entropy'] if alter else 0]   # joint: :885 writes 0
            corloc = list(result['corloc_list'])
            _print_validation(iteration, max_iters, tr, te, corloc, cur_lr)
            f_log.write(log_record(iteration, max_iters, tr, te, cur_lr))
            f_log.flush()
            f_sum.write(json.dumps(summary_record(iteration, tr, te, corloc[:3], cur_lr)) + '\n')
            f_sum.flush()
            history['validations'].append(dict(iter=iteration + 1, training_loss=[float(v) for v in tr], result=result,
                                               lr=float(cur_lr)))
        d = getattr(solver, 'dist', None)
        if d is not None and getattr(d, 'enabled', False):
            # rank 0 validated (and fed its own schedule inside validate): the other ranks feed theirs the same value
            total = d.sum_over_ranks(total)
            if not writer:
                solver.on_val_end(total)
    try:
        if pending:
            validate_at(start_iter - 1)
        for it in range(start_iter, max_iters):
            t0 = time.time()
            standins = running.standins(imdb_train_ws.num_classes)
            if alter:
                sup = mil = None
                if s_start <= it <= s_end:                                          # :334
                    cur_lr = solver.current_lr()
                    losses = solver.supervised_backward(layers['train_s'].forward())
                    # train_op_s: no global_step -- except under 'sgd' (SolverWrapper.train_step_alter)
                    solver._apply(solver.optimizer, count_step=solver.opt == 'sgd')
                    sup = [losses[k] for k in SUP_TERMS]
                if ws_start <= it <= ws_end and (it + 1) % cfg.TRAIN.WS_TRAIN_INTERVAL == 0:     # :368
                    cur_lr = solver.current_lr()
                    mil = solver.weak_backward(layers['train_ws'].forward())
                    if solver.optimizer_ws is None:
                        solver.optimizer_ws = solver._make_optimizer()
                    solver._apply(solver.optimizer_ws, count_step=True)
                running.add(sup, mil, standins)
            else:
                cur_lr = solver.current_lr()
                losses = solver.train_step_joint(layers['train'].forward())         # :737-764; the windows are ignored
                running.add([losses[k] for k in SUP_TERMS], losses['mil_cross_entropy'], standins)
            elapsed, timed = elapsed + (time.time() - t0), timed + 1

            if (it + 1) % cfg.TRAIN.DISPLAY == 0:                                    # :414-421
                v = running.last_values()
                print('iter: %d / %d' % (it + 1, max_iters))
                print('total_loss: %.4f' % v[0])
                print('rpn_loss_cls: %.4f, rpn_loss_box: %.4f, loss_cls: %.4f, loss_box: %.4f, mil_loss_cls: %.4f' % tuple(v[1:6]))
                print('speed: {:.3f}s / iter'.format(elapsed / max(timed, 1)))

            validating = (it + 1) % cfg.TRAIN.TEST_ITERS == 0
            if (it + 1) % cfg.TRAIN.SNAPSHOT_ITERS == 0:                             # :423
                last_snapshot_iter = it
                take_snapshot(it, validating)
            if validating:
                validate_at(it)
        if last_snapshot_iter != it and it >= start_iter:                            # :589
            take_snapshot(it, False)
        solver.check_flags()
        history['final_losses'] = [float(v) for v in running.sums()]
    finally:
        if writer:
            f_log.close()
            f_sum.close()
    return history


def train_model(solver, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test, output_dir, max_iters,
                s_start_iter=0, s_end_iter=80000, ws_start_iter=0, ws_end_iter=80000, vis=False, resume=None, val_ims_per_batch=1,
                max_per_image=300, thresh=0.05, data_layers=None, test_pass=None):
    """The joint loop (train_bus.py:595-958): one RoIDataLayerJoint.forward() and one train_step_joint per iteration.
    The four window arguments are accepted and ignored, as in the reference.  Returns the history dict:
    'validations' (per validation: iter, training_loss, validate's whole result, lr), 'snapshots' (paths),
    'final_losses'.  data_layers / test_pass: replacements for the layers built here and for the validation pass
    (tests)."""
    from .train_bus import get_data_layer
    net_name = type(solver.net).__name__
    layers = data_layers or dict(train=get_data_layer((roidb_train_s, roidb_train_ws), net_name, imdb_train_s.num_classes, True,
                                                      is_ws=True, is_joint=True))
    return _run(solver, False, layers, imdb_train_ws, imdb_test, roidb_test, output_dir, net_name, max_iters,
                (s_start_iter, s_end_iter, ws_start_iter, ws_end_iter), vis, resume, val_ims_per_batch, max_per_image, thresh, test_pass)


def train_model_alter(solver, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test, output_dir,
                      max_iters, s_start_iter=0, s_end_iter=80000, ws_start_iter=0, ws_end_iter=80000, vis=False, resume=None,
                      val_ims_per_batch=1, max_per_image=300, thresh=0.05, data_layers=None, test_pass=None):
    """The alternating loop (train_bus.py:175-593).  The supervised half runs only when s_start_iter <= iter <=
    s_end_iter, the weak half only when ws_start_iter <= iter <= ws_end_iter and (iter+1) %
    cfg.TRAIN.WS_TRAIN_INTERVAL == 0; a skipped half takes no batch and no optimiser step.  The halves are
    SolverWrapper.supervised_backward / weak_backward / _apply with train_step_alter's step-counting rule (the 'sgd'
    exception included); optimizer_ws is created as there.  Returns the history dict of train_model."""
    from .train_bus import get_data_layer
    net_name = type(solver.net).__name__
    layers = data_layers or dict(
        train_s=get_data_layer(roidb_train_s, net_name, imdb_train_s.num_classes, True),
        train_ws=get_data_layer(roidb_train_ws, net_name, imdb_train_ws.num_classes, True, is_ws=True))
    return _run(solver, True, layers, imdb_train_ws, imdb_test, roidb_test, output_dir, net_name, max_iters,
                (s_start_iter, s_end_iter, ws_start_iter, ws_end_iter), vis, resume, val_ims_per_batch, max_per_image, thresh, test_pass)


def _train(alter, network, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test, output_dir,
           pretrained_model, max_iters, windows, opt, lr, lr_scheduling, vis, resume, dist_ctx, val_ims_per_batch, max_per_image, thresh,
           mil_funcs=None):
    from .train_bus import SolverWrapper
    solver = SolverWrapper(network, lr, dist_ctx, opt, lr_scheduling, max_iters, mil_funcs=mil_funcs)
    if pretrained_model is not None:
        snap.load_pretrained(network, pretrained_model)                              # before the first step (:308-311)
    print('Solving...')
    run = train_model_alter if alter else train_model
    history = run(solver, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test, output_dir, max_iters,
                  windows[0], windows[1], windows[2], windows[3], vis=vis, resume=resume, val_ims_per_batch=val_ims_per_batch,
                  max_per_image=max_per_image, thresh=thresh)
    print('done solving')
    return history
