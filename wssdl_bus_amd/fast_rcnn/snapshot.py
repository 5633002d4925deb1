"""Snapshots of a training run and their restoration (reference: SolverWrapper.snapshot, fast_rcnn/train_bus.py:133-173).

File name: <output_dir>/<net_name[:6]>_fast_rcnn[_<cfg.TRAIN.SNAPSHOT_INFIX>]_iter_<iter+1>.pt -- the reference's name
(:158-164) with '.pt' for '.ckpt'; net_name is the network's class name.  The bbox-regression un-normalisation the
reference once did here is commented out there (:148-153), so it is not reproduced.

One file (torch.save) holds everything the next iteration reads:
  model                         the network's state_dict
  optimizer, optimizer_ws       both optimisers' state_dict() (optimizer_ws: None until the first alternating iteration)
  global_step                   the solver's step count (MIL scale factor, 'pc' schedule)
  opt, lr, lr_scheduling, max_iters    the solver's settings; a mismatch at restore raises ValueError
  roi_pool                      cfg.ROI_POOL_MODE, ROI_ALIGN_SAMPLING, ROI_ALIGN_ALIGNED as dict(mode, sampling, aligned): the
                                head was trained on that pooling, so a mismatch at restore raises ValueError; a file without
                                the key was written under 'max'
  rop                           the plateau handler's state (cur_lr, best, wait, cooldown_counter) or None
  loop                          the training loop's own state: iteration, running loss sums, the previous interval's
                                means (the alternating loop's stand-ins), ...
  data_layers                   name -> state_dict() of every data layer (permutations and cursors)
  rng                           np.random's state, torch's CPU generator state, the device generator's state (VGG-16's
                                dropout), cfg.DEVICE_RNG_SEED and the call counters the two device samplers fold into
                                their seeds

restore() puts all of it into freshly built objects.  Multi-rank runs: the file is written by rank 0; every rank
restores the shared state (model, optimisers, step, schedule, loop), while rank-local state -- the data cursors and
generators of ranks > 0 -- restarts from seed + rank: `rank_local=False` skips those entries.
"""
import os

import numpy as np
import torch

from ..roi_pooling_layer import roi_align_op
from ..rpn_msr import anchor_target_layer_tf_bus, proposal_target_layer_tf_bus
from .config import cfg

FORMAT = 1
SETTINGS = ('opt', 'lr', 'lr_scheduling', 'max_iters')
ROP_STATE = ('cur_lr', 'best', 'wait', 'cooldown_counter')


def snapshot_path(output_dir, net_name, iteration):
    infix = ('_' + cfg.TRAIN.SNAPSHOT_INFIX if cfg.TRAIN.SNAPSHOT_INFIX != '' else '')
    return os.path.join(output_dir, net_name[:6] + '_fast_rcnn' + infix + '_iter_{:d}'.format(iteration + 1) + '.pt')


def rng_state():
    state = dict(numpy=np.random.get_state(), torch_cpu=torch.get_rng_state(), torch_device=None,
                 device_rng_seed=int(cfg.DEVICE_RNG_SEED),
                 anchor_calls=anchor_target_layer_tf_bus.get_device_calls(),
                 roi_calls=proposal_target_layer_tf_bus.get_device_calls())
    if torch.cuda.is_available():
        state['torch_device'] = torch.cuda.get_rng_state()
    return state


def set_rng_state(state):
    np.random.set_state(state['numpy'])
    torch.set_rng_state(state['torch_cpu'])
    if state.get('torch_device') is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(state['torch_device'])
    cfg.DEVICE_RNG_SEED = int(state['device_rng_seed'])
    anchor_target_layer_tf_bus.set_device_calls(state['anchor_calls'])
    proposal_target_layer_tf_bus.set_device_calls(state['roi_calls'])


def solver_state(solver):
    rop = getattr(solver, 'rop', None)
    return dict(model=solver.net.state_dict(), optimizer=solver.optimizer.state_dict(),
                optimizer_ws=None if solver.optimizer_ws is None else solver.optimizer_ws.state_dict(),
                global_step=int(solver.global_step), opt=solver.opt, lr=float(solver.lr), lr_scheduling=solver.lr_scheduling,
                max_iters=solver.max_iters, rop=None if rop is None else {k: getattr(rop, k) for k in ROP_STATE})


def save_snapshot(solver, output_dir, net_name, iteration, loop_state=None, data_layers=None):
    """Writes the snapshot of `iteration` (0-based, as the reference counts) and returns its path.
    solver.check_flags() comes first: a raised device flag means the parameters are tainted, so no file is written
    and the error propagates.  The file appears under its name only whole (temporary name, then os.replace)."""
    solver.check_flags()
    path = snapshot_path(output_dir, net_name, iteration)
    state = solver_state(solver)
    state.update(format=FORMAT, iteration=int(iteration), net_name=net_name, loop=dict(loop_state or {}),
                 data_layers={k: v.state_dict() for k, v in (data_layers or {}).items()}, rng=rng_state(),
                 roi_pool=roi_align_op.settings())
    os.makedirs(output_dir, exist_ok=True)
    tmp = "%s.%d.tmp" % (path, os.getpid())
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    print('Wrote snapshot to: {:s}'.format(path))
    return path


def load_file(path):
    return torch.load(path, map_location='cpu', weights_only=False)


def load_pretrained(network, path):
    """pretrained_model: a snapshot written by this package, or a torch state_dict file, loaded NON-strictly (the
    reference's net.load(..., ignore_missing=True), :308-311).  Prints and returns the names that were missing.  The
    reference's .npy layout of TensorFlow variables is out of scope."""
    print('Loading pretrained model weights from {:s}'.format(path))
    state = load_file(path)
    if isinstance(state, dict) and 'model' in state and 'format' in state:
        state = state['model']
    result = network.load_state_dict(state, strict=False)
    missing = list(result.missing_keys)
    for name in missing:
        print('ignore missing: ' + name)
    return missing


def restore(path, solver, data_layers=None, rank_local=True):
    """Restores a snapshot into a freshly built solver (and data layers) and returns (iteration to continue at,
    the loop's state dict).  The solver's opt / lr / lr_scheduling / max_iters must be the saved ones: ValueError."""
    state = load_file(path)
    for key in SETTINGS:
        if state[key] != getattr(solver, key):
            raise ValueError("resume: the snapshot was written with %s=%r, this run has %s=%r"
                             % (key, state[key], key, getattr(solver, key)))
    saved, now = state.get('roi_pool') or dict(mode='max'), roi_align_op.settings()
    # (the two RoIAlign values only matter to a head that was trained on RoIAlign)
    keys = ('mode', 'sampling', 'aligned') if saved['mode'] == 'align' else ('mode',)
    for key in keys:
        if saved[key] != now[key]:
            raise ValueError("resume: the snapshot was written with RoI pooling %s=%r, this run has %s=%r"
                             % (key, saved[key], key, now[key]))
    solver.net.load_state_dict(state['model'])
    solver.optimizer.load_state_dict(state['optimizer'])
    if state['optimizer_ws'] is not None:
        if solver.optimizer_ws is None:
            solver.optimizer_ws = solver._make_optimizer()
        solver.optimizer_ws.load_state_dict(state['optimizer_ws'])
    solver.global_step = int(state['global_step'])
    if state['rop'] is not None:
        for k in ROP_STATE:
            setattr(solver.rop, k, state['rop'][k])
    if rank_local:
        for name, layer in (data_layers or {}).items():
            if name not in state['data_layers']:
                raise ValueError("resume: the snapshot holds no state of the data layer %r" % name)
            layer.load_state_dict(state['data_layers'][name])
        set_rng_state(state['rng'])
    return int(state['iteration']) + 1, state['loop']
