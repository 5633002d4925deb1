"""ctypes binding of ``libwssdl_plumbing_hip.so``: the fused row batch-norm (+ReLU) and residual-join kernels
(``csrc/plumbing/rowbn.hip``), the group-norm kernels (``groupnorm.hip``), the 3x3 patch kernels (``im2col.hip``) and the class-packed 3x3 convolutions
(``taps.hip``) of the two networks, the one-launch L2 weight decay of the training step (``l2decay.hip``) and the one-launch reference optimisers (``optim.hip``, bound by fast_rcnn/optim.py).  Plumbing around the hot path, not the drop-in C ABI; when the library has not
been built the networks fall back to stock PyTorch ops (slower, same maths) and say so once.  Imports no sibling
module: networks/rownorm.py, backbones.py and roi_head.py build on it, in that order.  Every export goes through
`_call`; the `*_usable` predicates, `fused_running_stats`, `running_of`, TAPS_MIN_ROIS and TAP_GEMM_GROUPED are
looked up as attributes of this module at call time (tests patch them)."""
import ctypes
import os
import warnings

import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_HERE, "libwssdl_plumbing_hip.so")
_lib = None
_warned = [False]

_vp, _i, _ll, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t
_RUN = [_vp, _vp, _f, _vp]          # running_mean, running_var, momentum, num_batches_tracked (struct Running)
_REN = [_vp, _vp, _vp, ctypes.c_double, _vp, _vp]   # renorm_mean, renorm_stddev, renorm_weight, renorm_momentum, r, d (struct Renorm)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            if not _warned[0]:
                _warned[0] = True
                warnings.warn("%s not built: the per-RoI head uses stock PyTorch batch-norm ops "
                              "(python -m wssdl_bus_amd.build builds it)" % LIB_PATH)
            return None
        L = ctypes.CDLL(LIB_PATH)
        L.wsplumb_rowbn_workspace_bytes.restype = _sz
        L.wsplumb_rowbn_workspace_bytes.argtypes = [_ll, _i]
        L.wsplumb_rowbn_supported.restype = _i
        L.wsplumb_rowbn_supported.argtypes = [_ll, _i]
        L.wsplumb_rowbn_forward.restype = _i
        L.wsplumb_rowbn_forward.argtypes = ([_vp, _ll, _i, _vp, _vp, _f, _i, _vp, _i, _i, _i] + [_vp] * 8 + [_sz, _vp]
                                            + _RUN)
        L.wsplumb_rowbn_stats.restype = _i
        L.wsplumb_rowbn_stats.argtypes = [_vp, _ll, _i, _vp, _vp, _f, _vp, _i, _i, _i] + [_vp] * 7 + [_sz, _vp] + _RUN
        L.wsplumb_rowbn_apply.restype = _i
        L.wsplumb_rowbn_apply.argtypes = [_vp, _ll, _i, _vp, _vp, _i, _vp, _vp]
        L.wsplumb_rowbn_backward.restype = _i
        L.wsplumb_rowbn_backward.argtypes = ([_vp, _vp, _ll, _i] + [_vp] * 5 + [_i, _vp, _i, _i, _i] + [_vp] * 5
                                             + [_sz, _vp])
        L.wsplumb_rowbn_backward_entry.restype = _i
        L.wsplumb_rowbn_backward_entry.argtypes = [_vp] * 4 + [_i, _ll, _i] + [_vp] * 6 + [_i, _i] + [_vp] * 5 + [_sz, _vp]
        L.wsplumb_rowbn_forward_entry.restype = _i
        L.wsplumb_rowbn_forward_entry.argtypes = ([_vp, _ll, _i, _vp, _vp, _f, _vp, _i, _i, _vp, _i] + [_vp] * 9
                                                  + [_sz, _vp] + _RUN)
        L.wsplumb_slot_mean.restype = _i
        L.wsplumb_slot_mean.argtypes = [_vp, _i, _i, _i, _vp, _vp]
        L.wsplumb_rowbn_join_workspace_bytes.restype = _sz
        L.wsplumb_rowbn_join_workspace_bytes.argtypes = [_ll, _i]
        L.wsplumb_rowbn_join_forward.restype = _i
        L.wsplumb_rowbn_join_forward.argtypes = [_vp, _vp, _ll, _i, _vp, _vp, _f, _vp, _vp, _f, _vp, _vp, _f, _vp, _i, _i,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]
        L.wsplumb_rowbn_join_forward_exit.restype = _i
        L.wsplumb_rowbn_join_forward_exit.argtypes = L.wsplumb_rowbn_join_forward.argtypes + [_i]
        L.wsplumb_rowbn_join_backward.restype = _i
        L.wsplumb_rowbn_join_backward.argtypes = [_vp] * 5 + [_ll, _i] + [_vp] * 7 + [_i, _i] + [_vp] * 8 + [_sz, _vp]
        L.wsplumb_rowbn_join_backward_exit.restype = _i
        L.wsplumb_rowbn_join_backward_exit.argtypes = ([_vp, _vp, _i, _vp, _vp, _ll, _i] + [_vp] * 7 + [_i, _i] + [_vp] * 8
                                                       + [_sz, _vp])
        # the batch-renormalisation twins: the plain export's arguments, then the renorm state / factors
        for name, extra in (("forward", _REN), ("stats", _REN), ("forward_entry", _REN), ("backward", [_vp, _vp]),
                            ("backward_entry", [_vp, _vp])):
            f = getattr(L, "wsplumb_rowbn_%s_renorm" % name)
            f.restype = _i
            f.argtypes = getattr(L, "wsplumb_rowbn_" + name).argtypes + extra
        L.wsplumb_rowbn_join_forward_renorm.restype = _i
        L.wsplumb_rowbn_join_forward_renorm.argtypes = L.wsplumb_rowbn_join_forward.argtypes + [_i, _vp, _vp]
        L.wsplumb_rowbn_join_backward_renorm.restype = _i
        L.wsplumb_rowbn_join_backward_renorm.argtypes = ([_vp] * 3 + [_i, _vp, _vp, _ll, _i] + [_vp] * 7 + [_i, _i]
                                                         + [_vp] * 8 + [_sz, _vp, _i])
        L.wsplumb_tap_table_ints.restype = _i
        L.wsplumb_tap_table_ints.argtypes = []
        for name in ("wsplumb_tap_gather", "wsplumb_tap_col2im"):
            f = getattr(L, name)
            f.restype = _i
            f.argtypes = [_vp, _ll, _i, _vp, _vp, _i, _vp, _vp]
        L.wsplumb_tap_gather_norm.restype = _i
        L.wsplumb_tap_gather_norm.argtypes = [_vp, _ll, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]
        for name in ("wsplumb_tap_weight_gather", "wsplumb_tap_weight_scatter"):
            f = getattr(L, name)
            f.restype = _i
            f.argtypes = [_vp, _i, _i, _vp, _vp, _vp, _vp]
        for name in ("wsplumb_im2col3x3", "wsplumb_col2im3x3"):
            f = getattr(L, name)
            f.restype = _i
            f.argtypes = [_vp, _ll, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]
        L.wsplumb_groupnorm_supported.restype = _i
        L.wsplumb_groupnorm_supported.argtypes = [_ll, _ll, _i, _i]
        L.wsplumb_groupnorm_workspace_bytes.restype = _sz
        L.wsplumb_groupnorm_workspace_bytes.argtypes = [_ll, _ll, _i]
        L.wsplumb_groupnorm_plan.restype = _i
        L.wsplumb_groupnorm_plan.argtypes = [_ll, _ll, _i, _vp]
        L.wsplumb_groupnorm_forward.restype = _i
        L.wsplumb_groupnorm_forward.argtypes = [_vp, _ll, _ll, _i, _i, _ll, _ll, _vp, _vp, _f, _i] + [_vp] * 5 + [_sz, _vp]
        L.wsplumb_groupnorm_backward.restype = _i
        L.wsplumb_groupnorm_backward.argtypes = ([_vp, _vp, _ll, _ll, _i, _i, _ll, _ll] + [_vp] * 4 + [_i] + [_vp] * 5
                                                 + [_sz, _vp])
        L.wsplumb_l2decay_chunk.restype = _i
        L.wsplumb_l2decay_chunk.argtypes = []
        L.wsplumb_l2decay_forward.restype = _i
        L.wsplumb_l2decay_forward.argtypes = [_vp, _i, _vp, _f, _vp, _vp]
        L.wsplumb_l2decay_backward.restype = _i
        L.wsplumb_l2decay_backward.argtypes = [_vp, _i, _vp, _f, _vp, _vp]
        L.wsplumb_optim_chunk.restype = _i
        L.wsplumb_optim_chunk.argtypes = []
        L.wsplumb_optim_step.restype = _i
        L.wsplumb_optim_step.argtypes = [_i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp] + [_f] * 6 + [_vp]
        _lib = L
    return _lib


# The A/B switches of the two networks: environment variables, set to anything non-empty, that take one fused route
# out for a measurement or a test.  Read at call time (switch), never cached: tests set them mid-process.
SWITCHES = {
    "WSSDL_DISABLE_FUSED_BN": "no row batch-norm kernel at all: stock PyTorch ops (usable)",
    "WSSDL_BN_TORCH_RUNNING_STATS": "running statistics by torch's lerp_, not the finish kernels (fused_running_stats); "
                                    "plain batch norms only: a renorm layer's state and running statistics are always "
                                    "the finish kernel's",
    "WSSDL_HEAD_UNFUSED_ENTRY": "block 1's entry: torch's index_select forward, scatter and add, then the plain "
                                "backward (entry_usable)",
    "WSSDL_HEAD_UNFUSED_EXIT": "the head's exit: the last join writes y, the slot-mean kernel reads it back, the mean's "
                               "gradient is expanded in memory (exit_usable)",
    "WSSDL_HEAD_UNFUSED_JOIN": "the head's residual joins: separate norms and a torch add (join_usable)",
    "WSSDL_TRUNK_UNFUSED_JOIN": "the trunk's residual joins: separate layers (backbones._join)",
    "WSSDL_DISABLE_FUSED_IM2COL": "3x3 patches by pad / unfold, not the patch kernels (im2col_usable)",
    "WSSDL_HEAD_UNFUSED_TAPNORM": "a bottleneck's conv1 norm as its own layer in front of the 3x3 patch gather "
                                  "(tapnorm_usable)",
    "WSSDL_HEAD_DENSE_3X3": "the head's 3x3 convolutions on the dense patch route (taps_usable)",
    "WSSDL_DISABLE_FUSED_GN": "no group-norm kernel: stock PyTorch ops (groupnorm_usable)",
    "WSSDL_TORCH_L2_DECAY": "the L2 weight decay by torch's per-parameter multiply / sum chain (l2decay_usable)",
    "WSSDL_TORCH_OPTIM": "the reference optimisers (fast_rcnn/optim.py) as a per-parameter chain of torch ops, not the "
                         "one-launch kernel (optim.hip_usable)",
}


def switch(name):
    assert name in SWITCHES, name
    return bool(os.environ.get(name))


def _same_pad(size, k, s):
    """TF 'SAME' padding along one axis: (before, after)."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _pn(t):
    return _p(t) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, dev, *args, tail=()):
    """One export on `dev` and its current stream (the argument after `args`; `tail` follows it); raises on rc != 0."""
    with torch.cuda.device(dev):
        rc = getattr(lib(), name)(*args, _stream(), *tail)
    if rc:
        raise RuntimeError("%s failed (%d)" % (name, rc))


def _mask_args(mask, M):
    """(mask, n_rois, rows per RoI) as the exports take them, (None, 0, 1) without a mask."""
    if mask is None:
        return None, 0, 1
    n_rois = mask.shape[0]
    assert M % n_rois == 0 and mask.dtype == torch.float32 and mask.is_contiguous()
    return _p(mask), n_rois, M // n_rois


def _workspace(x, join=False):
    """The scratch bytes a forward or backward over the [M, C] tensor x needs (`join`: of the join kernels)."""
    sizer = lib().wsplumb_rowbn_join_workspace_bytes if join else lib().wsplumb_rowbn_workspace_bytes
    return torch.empty((sizer(x.shape[0], x.shape[1]),), dtype=torch.uint8, device=x.device)


def usable(x):
    """True when the fused kernels can take this [M, C] tensor."""
    if switch("WSSDL_DISABLE_FUSED_BN"):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()):
        return False
    L = lib()
    return L is not None and bool(L.wsplumb_rowbn_supported(x.shape[0], x.shape[1]))


def fused_running_stats():
    """True when the forward finish kernel updates the layers' running statistics (rowbn.hip, struct Running);
    else torch's lerp_ does (rownorm.track)."""
    return not switch("WSSDL_BN_TORCH_RUNNING_STATS")


def running_of(bn):
    """The `running` argument of rowbn_forward / rowbn_join_forward for a norm module: (running_mean, running_var,
    momentum, num_batches_tracked or None), or None when torch updates the buffers (fused_running_stats)."""
    if not fused_running_stats() and renorm_of(bn) is None:     # (a renorm layer's buffers are always the kernel's)
        return None
    mom = bn.momentum if bn.momentum is not None else 0.1
    return bn.running_mean, bn.running_var, mom, getattr(bn, "num_batches_tracked", None)


def renorm_of(bn):
    """The `renorm` argument of the fused forwards for a norm module: (renorm_mean, renorm_stddev, renorm_weight,
    renorm_momentum) of a batch renormalisation layer (rownorm.RowBatchNorm / backbones.BatchNormAct2d built with
    renorm=True), None for a plain batch norm."""
    if not getattr(bn, "renorm", False):
        return None
    return bn.renorm_mean, bn.renorm_stddev, bn.renorm_weight, bn.renorm_momentum


def _run_args(running):
    if running is None:
        return None, None, 0.0, None
    rm, rv, mom, nbt = running
    assert rm.dtype == torch.float32 and rv.dtype == torch.float32 and rm.is_contiguous() and rv.is_contiguous()
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.numel() == 1)
    return _p(rm), _p(rv), float(mom), _pn(nbt)


def _state_ok(t, C):
    return t.dtype == torch.float32 and t.shape == (C,) and t.is_contiguous()


def _stats_block(x, renorm, n=None):
    """The statistic block(s) of a fused forward over x [M, C]: [5, C] = mean, var, rstd, scale, shift, or for a batch
    renormalisation layer [7, C], the step's r and d after them ([n, 5 or 7, C] for n norms)."""
    rows = 7 if renorm is not None else 5
    shape = (rows, x.shape[1]) if n is None else (n, rows, x.shape[1])
    return torch.empty(shape, dtype=torch.float32, device=x.device)


def _renorm_tail(renorm, stats):
    """(export suffix, the arguments after the running statistics) of a single-norm forward: the layer's renorm state
    (renorm_of) and rows 5 / 6 of its statistic block for r / d."""
    if renorm is None:
        return "", ()
    rm, rs, rw, rho = renorm
    assert all(_state_ok(t, stats.shape[1]) for t in (rm, rs, rw))
    return "_renorm", (_p(rm), _p(rs), _p(rw), float(rho), _p(stats[5]), _p(stats[6]))


def _rd(stats):
    """(export suffix, the r / d arguments) of a single-norm backward from the forward's statistic block"""
    return ("_renorm", (_p(stats[5]), _p(stats[6]))) if stats.shape[0] == 7 else ("", ())


def rowbn_forward(x, weight, bias, eps, relu, mask=None, pos_major=False, *, running=None, renorm=None):
    """mask: [n_rois] f32 on x's device (0 = dead RoI), x = [n_rois * per, C] with row r belonging to RoI
    r // per, or r % n_rois when pos_major; returns (y, stats, count) where count is None without a mask,
    else a [1] tensor holding the number of live rows.  running: the layer's buffers to update in the same
    kernels (running_of), or None.  renorm: the state of a batch renormalisation layer (renorm_of), updated in the
    same kernels; stats is then [7, C] (_stats_block) and scale / shift are the renorm layer's."""
    M, C = x.shape
    y = torch.empty_like(x)
    stats = _stats_block(x, renorm)
    count = torch.empty((1,), dtype=torch.float32, device=x.device) if mask is not None else None
    ws = _workspace(x)
    suffix, ren = _renorm_tail(renorm, stats)
    _call("wsplumb_rowbn_forward" + suffix, x.device, _p(x), M, C, _p(weight), _p(bias), float(eps), int(relu),
          *_mask_args(mask, M), int(bool(pos_major) and mask is not None), _p(y), *[_p(stats[i]) for i in range(5)],
          _pn(count), _p(ws), ws.numel(), tail=_run_args(running) + ren)
    return y, stats, count


def rowbn_stats(x, weight, bias, eps, mask=None, pos_major=False, *, running=None, renorm=None):
    """rowbn_forward without its apply pass: (stats, count), the layer's output left to a consumer that applies
    stats[3] / stats[4] (scale / shift) while it reads x (tap_gather_norm)."""
    M, C = x.shape
    stats = _stats_block(x, renorm)
    count = torch.empty((1,), dtype=torch.float32, device=x.device) if mask is not None else None
    ws = _workspace(x)
    suffix, ren = _renorm_tail(renorm, stats)
    _call("wsplumb_rowbn_stats" + suffix, x.device, _p(x), M, C, _p(weight), _p(bias), float(eps), *_mask_args(mask, M),
          int(bool(pos_major) and mask is not None), *[_p(stats[i]) for i in range(5)], _pn(count), _p(ws), ws.numel(),
          tail=_run_args(running) + ren)
    return stats, count


def rowbn_apply(x, scale, shift, relu):
    M, C = x.shape
    y = torch.empty_like(x)
    _call("wsplumb_rowbn_apply", x.device, _p(x), M, C, _p(scale), _p(shift), int(relu), _p(y))
    return y


def _backward_outputs(x):
    """dx, dwb [2, C] = (dweight, dbias) and the coefficient scratch of a backward call"""
    dwb = torch.empty((2, x.shape[1]), dtype=torch.float32, device=x.device)
    coef = torch.empty((3, x.shape[1]), dtype=torch.float32, device=x.device)
    return torch.empty_like(x), dwb, coef


def rowbn_backward(x, dy, weight, stats, relu, mask=None, pos_major=False):
    M, C = x.shape
    dx, dwb, coef = _backward_outputs(x)
    ws = _workspace(x)
    suffix, rd = _rd(stats)                        # a [7, C] block: the backward of a renorm layer
    _call("wsplumb_rowbn_backward" + suffix, x.device, _p(x), _p(dy), M, C, _p(weight), _p(stats[0]), _p(stats[2]),
          _p(stats[3]), _p(stats[4]), int(relu), *_mask_args(mask, M), int(bool(pos_major) and mask is not None),
          _p(dx), _p(dwb[0]), _p(dwb[1]), _p(coef), _p(ws), ws.numel(), tail=rd)
    return dx, dwb[0], dwb[1]


def entry_usable(x):
    """True when block 1's pre-activation norm may take its output's gradient in two parts (rowbn_backward_entry)
    for this roi-major [M, C] tensor."""
    return not switch("WSSDL_HEAD_UNFUSED_ENTRY") and usable(x) and x.shape[0] < 2 ** 31


def rowbn_forward_entry(x, weight, bias, eps, possel, n_slots, mask=None, *, running=None, renorm=None):
    """rowbn_forward(relu=True) of roi-major rows x [R * per, C] that also hands out, position-major, the rows of the
    positions possel names (int32 [per] on the device: the slot of each position or -1; every slot 0 .. n_slots - 1
    exactly once): returns (y, ys [n_slots * R, C], stats, count) with ys[possel[p] * R + roi] = y[roi * per + p],
    written by the apply pass itself."""
    M, C = x.shape
    per = possel.shape[0]
    n_rois = M // per
    assert M == n_rois * per and possel.dtype == torch.int32 and possel.is_contiguous() and 1 <= n_slots <= per
    assert mask is None or mask.shape[0] == n_rois
    y = torch.empty_like(x)
    ys = torch.empty((n_slots * n_rois, C), dtype=torch.float32, device=x.device)
    stats = _stats_block(x, renorm)
    count = torch.empty((1,), dtype=torch.float32, device=x.device) if mask is not None else None
    ws = _workspace(x)
    suffix, ren = _renorm_tail(renorm, stats)
    _call("wsplumb_rowbn_forward_entry" + suffix, x.device, _p(x), M, C, _p(weight), _p(bias), float(eps),
          _mask_args(mask, M)[0], n_rois, per, _p(possel), n_slots, _p(y), _p(ys), *[_p(stats[i]) for i in range(5)],
          _pn(count), _p(ws), ws.numel(), tail=_run_args(running) + ren)
    return y, ys, stats, count


def rowbn_backward_entry(x, dy, dys, possel, n_slots, weight, stats, mask=None):
    """rowbn_backward(relu=True) of roi-major rows x [R * per, C] whose output gradient is dy [R * per, C] plus, at the
    positions p with possel[p] = slot >= 0 (int32 [per] on the device), the position-major dys [n_slots * R, C]:
    bit-identical to the plain backward on dy + scatter(dys), without forming that sum in memory."""
    M, C = x.shape
    per = possel.shape[0]
    n_rois = M // per
    assert M == n_rois * per and dy.shape == x.shape and dys.shape == (n_slots * n_rois, C)
    assert dy.is_contiguous() and dys.is_contiguous() and possel.dtype == torch.int32 and possel.is_contiguous()
    assert mask is None or mask.shape[0] == n_rois
    dx, dwb, coef = _backward_outputs(x)
    ws = _workspace(x)
    suffix, rd = _rd(stats)
    _call("wsplumb_rowbn_backward_entry" + suffix, x.device, _p(x), _p(dy), _p(dys), _p(possel), n_slots, M, C, _p(weight),
          _p(stats[0]), _p(stats[2]), _p(stats[3]), _p(stats[4]), _mask_args(mask, M)[0], n_rois, per, _p(dx),
          _p(dwb[0]), _p(dwb[1]), _p(coef), _p(ws), ws.numel(), tail=rd)
    return dx, dwb[0], dwb[1]


def join_usable(x):
    """True when the residual-join kernels may take this position-major [M, C] tensor."""
    return not switch("WSSDL_HEAD_UNFUSED_JOIN") and usable(x)


def exit_usable(x):
    """True when the last join of the head may take its exit form for this position-major [M, C] tensor."""
    return not switch("WSSDL_HEAD_UNFUSED_EXIT") and join_usable(x) and x.shape[0] < 2 ** 31


def slot_mean(x, n_slots):
    """[n_slots * R, C] position-major rows -> [R, C]: the mean over the slots in the one order of the exit kernels
    (csrc/plumbing/bn_math.hip.h), not torch's."""
    M, C = x.shape
    R = M // n_slots
    assert M == R * n_slots and x.is_contiguous() and x.dtype == torch.float32
    feat = torch.empty((R, C), dtype=torch.float32, device=x.device)
    _call("wsplumb_slot_mean", x.device, _p(x), n_slots, R, C, _p(feat))
    return feat


def rowbn_join_forward(x3, bn3, other, bns, bnn, mask=None, *, running=None, exit_slots=None, renorm=None):
    """out = bn3(x3) + (bns(other) if bns else other); y = relu(bnn(out)): training-mode row batch norms over
    position-major rows, each bn a (weight, bias, eps) triple, mask as in rowbn_forward(pos_major=True).
    Returns (out, y, stats3, stats_s, stats_n, count or None), stats_s unwritten without bns; bit-identical to the
    separate calls.  running: None, or the running_of() of bn3, bns (None without it) and bnn.
    exit_slots = n_slots (the head's exit): y is never written; in its place comes feat [M / n_slots, C] =
    slot_mean(y, n_slots), bit for bit.
    renorm: None, or the renorm_of() of bn3, bns and bnn (None for a plain norm among them): the three statistic
    blocks are then [7, C] (_stats_block; rows 5 / 6 of a plain norm's are not written) and rowbn_join_backward needs
    renorm_bits(renorm)."""
    M, C = x3.shape
    dev = x3.device
    assert other.shape == x3.shape and other.is_contiguous() and other.dtype == torch.float32
    out = torch.empty_like(x3)
    if exit_slots:
        assert M % exit_slots == 0 and (mask is None or mask.shape[0] * exit_slots == M)
        y = torch.empty((M // exit_slots, C), dtype=torch.float32, device=dev)
    else:
        y = torch.empty_like(x3)
    if renorm is not None and all(r is None for r in renorm):
        renorm = None
    stats = _stats_block(x3, renorm, 3)
    count = torch.empty((1,), dtype=torch.float32, device=dev) if mask is not None else None
    ws_, bs_, es_ = bns if bns is not None else (None, None, 0.0)
    run = (None, None, None)
    if running is not None:
        a = [_run_args(r) for r in running]
        val = lambda q: q.value if q is not None else None
        run = ((_vp * 6)(*[val(q) for r in a for q in r[:2]]), (_f * 3)(*[r[2] for r in a]),
               (_vp * 3)(*[val(r[3]) for r in a]))
    ws = _workspace(x3, join=True)
    if renorm is not None:
        assert bns is not None or renorm[1] is None
        assert all(_state_ok(t, C) for r in renorm if r is not None for t in r[:3])
        name = "wsplumb_rowbn_join_forward_renorm"
        tail = run + (int(exit_slots or 0),
                      (_vp * 9)(*[t.data_ptr() if r is not None else None for r in renorm for t in (r or (0, 0, 0))[:3]]),
                      (ctypes.c_double * 3)(*[float(r[3]) if r is not None else 0.0 for r in renorm]))
    else:
        name = "wsplumb_rowbn_join_forward_exit" if exit_slots else "wsplumb_rowbn_join_forward"
        tail = run + ((int(exit_slots),) if exit_slots else ())
    _call(name, dev, _p(x3), _p(other), M, C,
          _p(bn3[0]), _p(bn3[1]), float(bn3[2]), _pn(ws_), _pn(bs_), float(es_), _p(bnn[0]), _p(bnn[1]), float(bnn[2]),
          *_mask_args(mask, M), _p(out), _p(y), _p(stats[0]), _p(stats[1]) if bns is not None else None, _p(stats[2]),
          _pn(count), _p(ws), ws.numel(), tail=tail)
    return out, y, stats[0], stats[1], stats[2], count


def renorm_bits(renorm):
    """rowbn_join_backward's `renorm` from rowbn_join_forward's: bit 0 / 1 / 2 for a renorm bn3 / bns / bnn."""
    return sum(1 << k for k, r in enumerate(renorm or ()) if r is not None)


def rowbn_join_backward(out, dy, dres, x3, xs, wn, stats_n, w3, stats3, ws_, stats_s, mask=None, exit_slots=None,
                        renorm=0):
    """Gradients of rowbn_join_forward: dy for y, dres (or None) for out; xs / ws_ / stats_s None in the identity
    form.  Returns (g, dx3, dxs or None, dwb_n, dwb3, dwb_s or None), the dwb [2, C] = (dweight, dbias); g is the
    gradient of `other` in the identity form.  exit_slots = n_slots: dy is the gradient of feat [M / n_slots, C] and
    dres must be None; bit-identical to the plain form on (dy * (1 / n_slots)) repeated over the slots.
    renorm: renorm_bits() of the forward's renorm argument (the [7, C] blocks of those norms carry their r and d)."""
    M, C = x3.shape
    if exit_slots:
        assert dres is None and dy.shape == (M // exit_slots, C) and dy.is_contiguous()
    dual = xs is not None
    g, dx3 = torch.empty_like(x3), torch.empty_like(x3)
    dxs = torch.empty_like(x3) if dual else None
    dwb = torch.empty((3, 2, C), dtype=torch.float32, device=x3.device)
    coef = torch.empty((9, C), dtype=torch.float32, device=x3.device)
    ws = _workspace(x3, join=True)
    tail = ()
    if renorm:
        assert all(st is None or st.shape[0] == 7 for st in (stats_n, stats3, stats_s))
        name, third, tail = "wsplumb_rowbn_join_backward_renorm", (_pn(dres), int(exit_slots or 0)), (int(renorm),)
    elif exit_slots:
        name, third = "wsplumb_rowbn_join_backward_exit", (int(exit_slots),)
    else:
        name, third = "wsplumb_rowbn_join_backward", (_pn(dres),)
    _call(name, x3.device, _p(out), _p(dy), *third, _p(x3), _pn(xs), M, C, _p(wn),
          _p(stats_n), _p(w3), _p(stats3), _pn(ws_), _pn(stats_s), *_mask_args(mask, M), _p(g), _p(dx3), _pn(dxs),
          _p(dwb[0]), _p(dwb[1]), _p(dwb[2]) if dual else None, _p(coef), _p(ws), ws.numel(), tail=tail)
    return g, dx3, dxs, dwb[0], dwb[1], dwb[2] if dual else None


# ---- group normalisation over [S * P, C] rows (csrc/plumbing/groupnorm.hip) ----
def groupnorm_usable(x, P, G):
    """True when the fused group-norm kernels take this [M, C] tensor as M / P samples of P rows in G groups."""
    if switch("WSSDL_DISABLE_FUSED_GN"):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and x.data_ptr() % 16 == 0):
        return False
    if P < 1 or x.shape[0] == 0 or x.shape[0] % P:
        return False
    L = lib()
    return L is not None and bool(L.wsplumb_groupnorm_supported(x.shape[0] // P, P, x.shape[1], G))


def groupnorm_plan(S, P, C):
    """(small regime?, workgroups or chunks per sample, rows per chunk) of a fused call: what the tests annotate."""
    what = (_ll * 3)()
    if lib().wsplumb_groupnorm_plan(S, P, C, what):
        raise ValueError("group norm: unsupported shape")
    return bool(what[0]), int(what[1]), int(what[2])


def _gn_args(x, P, mask, pos_major):
    """(S, P, C, the two row strides, the mask pointer) of a group-norm call over x [S * P, C]: row (s, p) is
    s * P + p, or p * S + s when position-major."""
    M, C = x.shape
    S = M // P
    assert M == S * P and x.is_contiguous() and x.dtype == torch.float32
    assert mask is None or (mask.shape == (S,) and mask.dtype == torch.float32 and mask.is_contiguous())
    ss, ps = (1, S) if pos_major else (P, 1)
    return S, P, C, ss, ps, _pn(mask)


def _gn_workspace(x, S, P):
    n = lib().wsplumb_groupnorm_workspace_bytes(S, P, x.shape[1])
    return torch.empty((max(n, 16),), dtype=torch.uint8, device=x.device)


def groupnorm_forward(x, P, gamma, beta, eps, G, relu, mask=None, pos_major=False):
    """y = act(group_norm(x)) over the S = M / P samples of x [M, C] (interleaved groups: channel c in group c % G);
    mask [S] f32 (0 = dead sample: zeros out, rows not read).  Returns (y, mean [S, G], rstd [S, G])."""
    S, P, C, ss, ps, pm = _gn_args(x, P, mask, pos_major)
    y = torch.empty_like(x)
    mean = torch.empty((S, G), dtype=torch.float32, device=x.device)
    rstd = torch.empty((S, G), dtype=torch.float32, device=x.device)
    ws = _gn_workspace(x, S, P)
    _call("wsplumb_groupnorm_forward", x.device, _p(x), S, P, C, G, ss, ps, _p(gamma), _p(beta), float(eps), int(relu), pm,
          _p(y), _p(mean), _p(rstd), _p(ws), ws.numel())
    return y, mean, rstd


def groupnorm_backward(x, dy, P, gamma, beta, mean, rstd, relu, mask=None, pos_major=False):
    """(dx, dgamma, dbeta) of groupnorm_forward from its input, the output's gradient and its mean / rstd; the ReLU gate
    is recomputed from x (which is what beta is for)."""
    S, P, C, ss, ps, pm = _gn_args(x, P, mask, pos_major)
    G = mean.shape[1]
    assert dy.shape == x.shape and dy.is_contiguous() and dy.dtype == torch.float32
    assert mean.shape == (S, G) and rstd.shape == (S, G) and mean.is_contiguous() and rstd.is_contiguous()
    dx = torch.empty_like(x)
    dgb = torch.empty((2, C), dtype=torch.float32, device=x.device)
    ws = _gn_workspace(x, S, P)
    _call("wsplumb_groupnorm_backward", x.device, _p(x), _p(dy), S, P, C, G, ss, ps, _p(gamma), _p(beta), _p(mean),
          _p(rstd), int(relu), pm, _p(dx), _p(dgb[0]), _p(dgb[1]), _p(ws), ws.numel())
    return dx, dgb[0], dgb[1]


def im2col_usable(x):
    """True when the 3x3 patch kernels can take this [R, h, w, C] tensor."""
    return (not switch("WSSDL_DISABLE_FUSED_IM2COL") and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous() and x.shape[3] % 4 == 0 and x.shape[0] > 0 and lib() is not None)


class Im2Col3x3Fn(torch.autograd.Function):
    """[R, h, w, C] -> [R*oh*ow, 9*C] patches (kh, kw, c), TF 'SAME' padding given by (pt, pl)."""

    @staticmethod
    def forward(ctx, x, stride, oh, ow, pt, pl):
        r, h, w, c = x.shape
        cols = torch.empty((r * oh * ow, 9 * c), dtype=torch.float32, device=x.device)
        _call("wsplumb_im2col3x3", x.device, _p(x), r, h, w, c, oh, ow, stride, pt, pl, _p(cols))
        ctx.geom = (r, h, w, c, oh, ow, stride, pt, pl)
        return cols

    @staticmethod
    def backward(ctx, dcols):
        r, h, w, c = ctx.geom[:4]
        dcols = dcols.contiguous()
        dx = torch.empty((r, h, w, c), dtype=torch.float32, device=dcols.device)
        _call("wsplumb_col2im3x3", dcols.device, _p(dcols), *ctx.geom, _p(dx))
        return dx, None, None, None, None, None


# ---- 3x3 convolutions without their padding taps (csrc/plumbing/taps.hip) ----
# Class table layout: keep in sync with the TAB_* / C_* constants of taps.hip.
_TAB_CLS, _CLS_STRIDE, _MAX_CLS, _MAX_POS = 16, 24, 9, 64
_TAB_SLOTPOS = _TAB_CLS + _CLS_STRIDE * _MAX_CLS
_TAB_POSSLOT, _TAB_SLOTCLS = _TAB_SLOTPOS + _MAX_POS, _TAB_SLOTPOS + 2 * _MAX_POS
_TAB_INTS = _TAB_SLOTCLS + _MAX_POS

# one GEMM call per group of equal-shape classes (batched) or one per class (measurement switch)
TAP_GEMM_GROUPED = True
# Fewer RoIs than this keep the dense route: the class-packed route issues ~3x the launches of the dense one
# (gather, weight gather, 3 GEMMs per pass instead of 1), which at a few hundred RoIs cost more than the skipped
# FLOPs save (resnet18_sup_b2, R = 256: 15-25 % slower per step; profiles/README.md).
TAPS_MIN_ROIS = 2048


class TapPlan:
    """Position classes of a 3x3 TF-'SAME' convolution of an h x w map at stride s.

    Along each axis an output position's valid taps are those whose input lies inside the map; positions
    with the same valid taps form an axis class, and a 2-D class is a (row class, column class) pair.  A
    class is one GEMM with K = (its taps) * C.  Classes are ordered by (taps, positions) descending
    (centre | edges | corners for a 4x4 output), and the output positions get SLOTS in that order:
    position-major rows are slot * R + roi.  Classes of equal shape are adjacent and form one `group`.
    """

    def __init__(self, h, w, s):
        self.h, self.w, self.s = h, w, s
        self.pt, self.pl = _same_pad(h, 3, s)[0], _same_pad(w, 3, s)[0]
        self.oh, self.ow = -(-h // s), -(-w // s)

        def axis(n_in, n_out, pad):
            cls = {}
            for o in range(n_out):
                taps = tuple(k for k in range(3) if 0 <= o * s + k - pad < n_in)
                cls.setdefault(taps, []).append(o)
            return list(cls.items())

        classes = []
        for ty, ys in axis(h, self.oh, self.pt):
            for tx, xs in axis(w, self.ow, self.pl):
                classes.append(([ky * 3 + kx for ky in ty for kx in tx], [(y, x) for y in ys for x in xs]))
        classes.sort(key=lambda c: (-len(c[0]), -len(c[1])))        # stable: raster order within a shape
        self.classes = classes
        self.slots = [p for _, pos in classes for p in pos]
        self.groups, k = [], 0                      # (first class, n classes, npos, ntaps)
        while k < len(classes):
            j = k
            while j < len(classes) and (len(classes[j][0]), len(classes[j][1])) == \
                    (len(classes[k][0]), len(classes[k][1])):
                j += 1
            self.groups.append((k, j - k, len(classes[k][1]), len(classes[k][0])))
            k = j
        self.cum, self.wcum, self.slot_base = [], [], []
        u = wu = sb = 0
        for taps, pos in classes:
            self.cum.append(u)
            self.wcum.append(wu)
            self.slot_base.append(sb)
            u, wu, sb = u + len(taps) * len(pos), wu + len(taps), sb + len(pos)
        self.units, self.wunits = u, wu
        self.ok = (len(classes) <= _MAX_CLS and self.oh * self.ow <= _MAX_POS and h * w <= _MAX_POS
                   and self.units < 9 * self.oh * self.ow)          # nothing to skip: the dense route
        self.table = self._table()
        self.hnum = self.table.ctypes.data_as(ctypes.c_void_p)     # host copy: the entry points' shape checks
        self._dev = {}

    def _table(self):
        import numpy as np
        T = np.full(_TAB_INTS, -1, np.int32)
        T[:10] = [len(self.classes), self.h, self.w, self.oh, self.ow, self.s, self.pt, self.pl, self.units,
                  self.wunits]
        for k, (taps, pos) in enumerate(self.classes[:_MAX_CLS]):
            b = _TAB_CLS + _CLS_STRIDE * k
            T[b:b + 5] = [len(pos), len(taps), self.slot_base[k], self.cum[k], self.wcum[k]]
            T[b + 6:b + 6 + len(taps)] = taps
            for i, t in enumerate(taps):
                T[b + 15 + t] = i
        for sl, (y, x) in enumerate(self.slots[:_MAX_POS]):
            T[_TAB_SLOTPOS + sl] = y * self.ow + x
            T[_TAB_POSSLOT + y * self.ow + x] = sl
            T[_TAB_SLOTCLS + sl] = next(k for k in range(len(self.classes))
                                        if self.slot_base[k] <= sl < self.slot_base[k] + len(self.classes[k][1]))
        return T

    def device_table(self, dev):
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = torch.from_numpy(self.table).to(dev)
        return t

    def subsample_index(self, w_in, s, dev):
        """Flat input positions (y*s)*w_in + x*s of the slots: a 1x1 stride-s convolution in slot order."""
        key = ("sub", w_in, s, dev)
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.tensor([y * s * w_in + x * s for y, x in self.slots],
                                              dtype=torch.long, device=dev)
        return t


    def subsample_slots(self, h_in, w_in, s, dev):
        """Inverse of subsample_index as an int32 [h_in * w_in] tensor: the slot that reads each input position,
        -1 for the positions no slot reads."""
        key = ("subinv", h_in, w_in, s, dev)
        t = self._dev.get(key)
        if t is None:
            inv = [-1] * (h_in * w_in)
            for sl, (y, x) in enumerate(self.slots):
                inv[y * s * w_in + x * s] = sl
            t = self._dev[key] = torch.tensor(inv, dtype=torch.int32, device=dev)
        return t


_PLANS = {}


def tap_plan(h, w, s):
    p = _PLANS.get((h, w, s))
    if p is None:
        p = _PLANS[(h, w, s)] = TapPlan(h, w, s)
    return p


def taps_usable(x):
    """True when the head may run its 3x3 convolutions on the class-packed route (x: [R, h, w, C])."""
    return not switch("WSSDL_HEAD_DENSE_3X3") and im2col_usable(x) and x.shape[0] >= TAPS_MIN_ROIS


def tap_gather(x, plan, in_pm, R):
    """class-packed patches (plan.units * R * C floats) of x: roi-major [R, h, w, C] or position-major."""
    C = x.shape[-1]
    cols = torch.empty((plan.units * R * C,), dtype=torch.float32, device=x.device)
    _call("wsplumb_tap_gather", x.device, _p(x), R, C, _p(plan.device_table(x.device)), plan.hnum, int(in_pm), _p(cols))
    return cols


def tapnorm_usable(x):
    """True when the patch gather may apply the norm + ReLU of the [M, C] rows x it reads (tap_gather_norm)."""
    return not switch("WSSDL_HEAD_UNFUSED_TAPNORM") and usable(x)


def tap_gather_norm(x, plan, in_pm, R, scale, shift, mask=None):
    """tap_gather(relu(x * scale + shift) with the rows of the RoIs mask marks dead zeroed) without that tensor:
    x the rows [h*w*R, C] of a row batch norm's input (roi-major or position-major), scale / shift its stats[3] /
    stats[4], mask [R] f32 or None."""
    C = x.shape[-1]
    assert x.numel() == plan.h * plan.w * R * C and x.is_contiguous() and (not in_pm or plan.h == plan.oh)
    assert scale.shape == (C,) and shift.shape == (C,) and scale.is_contiguous() and shift.is_contiguous()
    assert mask is None or (mask.shape == (R,) and mask.dtype == torch.float32 and mask.is_contiguous())
    cols = torch.empty((plan.units * R * C,), dtype=torch.float32, device=x.device)
    _call("wsplumb_tap_gather_norm", x.device, _p(x), R, C, _p(plan.device_table(x.device)), plan.hnum, int(in_pm),
          _p(scale), _p(shift), _pn(mask), _p(cols))
    return cols


def tap_col2im(dcols, plan, in_pm, R, C):
    """adjoint of tap_gather: dx roi-major [R, h, w, C], or position-major [h*w*R, C] with in_pm."""
    shape = (plan.h * plan.w * R, C) if in_pm else (R, plan.h, plan.w, C)
    dx = torch.empty(shape, dtype=torch.float32, device=dcols.device)
    _call("wsplumb_tap_col2im", dcols.device, _p(dcols), R, C, _p(plan.device_table(dcols.device)), plan.hnum,
          int(in_pm), _p(dx))
    return dx


def tap_weight_gather(weight, plan):
    """[c_o, 9*C] -> class-packed (plan.wunits * c_o * C floats): class k is [c_o, ntaps_k * C]."""
    CO, C = weight.shape[0], weight.shape[1] // 9
    wp = torch.empty((plan.wunits * CO * C,), dtype=torch.float32, device=weight.device)
    _call("wsplumb_tap_weight_gather", weight.device, _p(weight), CO, C, _p(plan.device_table(weight.device)),
          plan.hnum, _p(wp))
    return wp


def tap_weight_scatter(dwp, plan, CO, C):
    """adjoint of tap_weight_gather: [c_o, 9*C], each column the class contributions summed in class order."""
    dw = torch.empty((CO, 9 * C), dtype=torch.float32, device=dwp.device)
    _call("wsplumb_tap_weight_scatter", dwp.device, _p(dwp), CO, C, _p(plan.device_table(dwp.device)), plan.hnum,
          _p(dw))
    return dw


def _gemm_groups(plan, fn):
    for k0, n, npos, ntaps in plan.groups:
        if TAP_GEMM_GROUPED or n == 1:
            fn(k0, n, npos, ntaps, slice(0, n))
        else:
            for j in range(n):
                fn(k0, n, npos, ntaps, slice(j, j + 1))


def tap_gemms_forward(cols, weight, bias, plan, R):
    """The class GEMMs of a 3x3 convolution over the class-packed patches `cols`: (position-major output
    [oh*ow*R, c_o], the class-packed weight)."""
    C, CO = weight.shape[1] // 9, weight.shape[0]
    wp = tap_weight_gather(weight.contiguous(), plan)
    out = torch.empty((plan.oh * plan.ow * R, CO), dtype=torch.float32, device=cols.device)

    def gemm(k0, n, npos, ntaps, j):
        a = cols[plan.cum[k0] * R * C:(plan.cum[k0] + n * npos * ntaps) * R * C].view(n, npos * R, ntaps * C)
        b = wp[plan.wcum[k0] * CO * C:(plan.wcum[k0] + n * ntaps) * CO * C].view(n, CO, ntaps * C)
        o = out[plan.slot_base[k0] * R:(plan.slot_base[k0] + n * npos) * R].view(n, npos * R, CO)
        if j.stop - j.start == 1:
            torch.mm(a[j.start], b[j.start].t(), out=o[j.start])
        else:
            torch.bmm(a, b.transpose(1, 2), out=o)

    _gemm_groups(plan, gemm)
    if bias is not None:
        out.add_(bias)
    return out, wp


def tap_gemms_backward(dy, cols, wp, plan, R, C, CO, need_x, need_w):
    """Gradients of tap_gemms_forward: (the input's in the layout of tap_col2im's result or None, the weight's
    [c_o, 9*C] or None)."""
    dcols = torch.empty_like(cols) if need_x else None
    dwp = torch.empty_like(wp) if need_w else None

    def gemm(k0, n, npos, ntaps, j):
        g = dy[plan.slot_base[k0] * R:(plan.slot_base[k0] + n * npos) * R].view(n, npos * R, CO)
        cs = slice(plan.cum[k0] * R * C, (plan.cum[k0] + n * npos * ntaps) * R * C)
        ws = slice(plan.wcum[k0] * CO * C, (plan.wcum[k0] + n * ntaps) * CO * C)
        one = j.stop - j.start == 1
        if need_x:
            b = wp[ws].view(n, CO, ntaps * C)
            o = dcols[cs].view(n, npos * R, ntaps * C)
            if one:
                torch.mm(g[j.start], b[j.start], out=o[j.start])
            else:
                torch.bmm(g, b, out=o)
        if need_w:
            a = cols[cs].view(n, npos * R, ntaps * C)
            o = dwp[ws].view(n, CO, ntaps * C)
            if one:
                torch.mm(g[j.start].t(), a[j.start], out=o[j.start])
            else:
                torch.bmm(g.transpose(1, 2), a, out=o)

    _gemm_groups(plan, gemm)
    return dcols, tap_weight_scatter(dwp, plan, CO, C) if need_w else None


class TapConv3x3Fn(torch.autograd.Function):
    """3x3 TF-'SAME' convolution over the valid taps only (TapPlan): x is roi-major [R, h, w, C] or, with
    in_pm, position-major [h*w*R, C] in the plan's slot order; weight [c_o, 9*C] (kh, kw, c); returns the
    position-major [oh*ow*R, c_o] output.  One GEMM per class group (torch's hipBLASLt); patches, weights
    and their gradients move between the dense and the class-packed layouts in taps.hip.

    With norm_w / norm_b (a row batch norm's weight and bias; eps, roi_mask, running and renorm as rowbn_forward takes them)
    x is instead the RAW rows [h*w*R, C] in front of that norm + ReLU -- a bottleneck's conv1 output -- and the
    convolution runs over relu(bn(x)): the forward takes the norm's statistics (two of the layer's three kernels,
    running statistics included) and the patch gather applies scale, shift and ReLU while it copies
    (tap_gather_norm), so the layer's output is never written, read back or kept for the backward.  The backward is
    the two layers': the class GEMMs, the patches' adjoint, then rowbn_backward on (x, that gradient).  Returns
    (out, mean, var, live-row count) then; bit-identical to the separate layers."""

    @staticmethod
    def forward(ctx, x, weight, bias, plan, in_pm, R, norm_w=None, norm_b=None, eps=0.0, roi_mask=None, running=None,
                renorm=None):
        C, CO = weight.shape[1] // 9, weight.shape[0]
        x = x.contiguous()
        assert x.shape[-1] == C and x.numel() == plan.h * plan.w * R * C and (not in_pm or plan.h == plan.oh)
        normed = norm_w is not None
        if normed:
            x = x.view(-1, C)
            stats, count = rowbn_stats(x, norm_w, norm_b, eps, roi_mask, in_pm, running=running, renorm=renorm)
            cols = tap_gather_norm(x, plan, in_pm, R, stats[3], stats[4], roi_mask)
        else:
            cols = tap_gather(x, plan, in_pm, R)
        out, wp = tap_gemms_forward(cols, weight, bias, plan, R)
        ctx.geom = (plan, bool(in_pm), R, C, CO, bias is not None, normed)
        if not normed:
            ctx.save_for_backward(cols, wp)
            return out
        ctx.save_for_backward(cols, wp, x, norm_w, stats, roi_mask)
        mean, var = stats[0], stats[1]
        if count is None:
            count = stats[0, :1]                           # placeholder without a mask (unused: no extra launch)
        ctx.mark_non_differentiable(mean, var, count)
        ctx.set_materialize_grads(False)                   # no zero-filled gradients for the side outputs
        return out, mean, var, count

    @staticmethod
    def backward(ctx, dy, *_):
        cols, wp = ctx.saved_tensors[:2]
        plan, in_pm, R, C, CO, has_bias, normed = ctx.geom
        dy = dy.contiguous() if dy is not None else cols.new_zeros((plan.oh * plan.ow * R, CO))
        need_x = ctx.needs_input_grad[0] or (normed and (ctx.needs_input_grad[6] or ctx.needs_input_grad[7]))
        dcols, dw = tap_gemms_backward(dy, cols, wp, plan, R, C, CO, need_x, ctx.needs_input_grad[1])
        dx = tap_col2im(dcols, plan, in_pm, R, C) if need_x else None
        db = dwn = dbn = None
        if has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        if normed and need_x:
            x, norm_w, stats, roi_mask = ctx.saved_tensors[2:]
            dx, dwn, dbn = rowbn_backward(x, dx.view(x.shape), norm_w, stats, True, roi_mask, in_pm)
        return dx, dw, db, None, None, None, dwn, dbn, None, None, None, None

# ---- L2 weight decay over all the decayed parameters as one device op (csrc/plumbing/l2decay.hip) ----
_L2_CHUNK = 4096                    # floats per chunk: keep in sync with CHUNK of l2decay.hip
_L2_ALIGN = 4                       # every parameter starts on a float4 of the flat gradient buffer


def _storage_dense(p):
    """True when p's elements fill numel() consecutive floats of its storage in some order of its dimensions
    (contiguous, channels_last, any permutation of a contiguous tensor)."""
    expect = 1
    for stride, size in sorted((st, sz) for sz, st in zip(p.shape, p.stride()) if sz != 1):
        if stride != expect:
            return False
        expect *= size
    return p.numel() > 0


def l2decay_usable(params):
    """True when l2_decay takes this parameter list: every one a dense f32 tensor on the same GPU."""
    if switch("WSSDL_TORCH_L2_DECAY") or not params:
        return False
    dev = params[0].device
    if not all(p.is_cuda and p.device == dev and p.dtype == torch.float32 and _storage_dense(p) for p in params):
        return False
    return lib() is not None


class _L2Table:
    """Device table of l2decay.hip for one parameter list: row i = (address of chunk i's first float, its element
    offset in the flat gradient buffer, its length), the parameters walked in storage order; `offsets` are the
    parameters' own offsets in the flat buffer, `total` its length."""

    def __init__(self, params):
        rows, self.offsets, off = [], [], 0
        for p in params:
            self.offsets.append(off)
            n, base = p.numel(), p.data_ptr()
            for first in range(0, n, _L2_CHUNK):
                rows.append((base + 4 * first, off + first, min(_L2_CHUNK, n - first)))
            off += -(-n // _L2_ALIGN) * _L2_ALIGN
        self.total, self.n_chunks = off, len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(params[0].device)


_L2_TABLES = {}                     # device -> (key, _L2Table): the last parameter list seen on it
L2_TABLE_BUILDS = [0]               # tables built so far (tests read it)


def _l2_table(params):
    """The table of `params`, cached while they stay where they are (the optimiser updates them in place, so a
    training run builds it once); anything else -- another list, a re-allocated parameter -- rebuilds it."""
    key = tuple((p.data_ptr(), tuple(p.shape), p.stride()) for p in params)
    dev = params[0].device
    hit = _L2_TABLES.get(dev)
    if hit is None or hit[0] != key:
        assert lib().wsplumb_l2decay_chunk() == _L2_CHUNK
        hit = _L2_TABLES[dev] = (key, _L2Table(params))
        L2_TABLE_BUILDS[0] += 1
    return hit[1]


class _L2DecayFn(torch.autograd.Function):
    """f32(sum over every parameter of sum(p * p)) * k as two launches; the backward writes every parameter's
    gradient 2 * p * (gout * k) into one flat buffer with one launch and returns views of it that have the
    parameters' own strides.  The gradients are bit-identical to those of torch's chain
    stack([(p * p).sum() ...]).sum() * k; the value is the f64 sum rounded once (torch sums in f32)."""

    @staticmethod
    def forward(ctx, k, *params):
        tab = _l2_table(params)
        dev = params[0].device
        partial = torch.empty((tab.n_chunks,), dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        _call("wsplumb_l2decay_forward", dev, _p(tab.table), tab.n_chunks, _p(partial), float(k), _p(out))
        ctx.save_for_backward(*params)
        ctx.k = float(k)
        return out

    @staticmethod
    def backward(ctx, gout):
        params = ctx.saved_tensors
        tab = _l2_table(params)
        dev = params[0].device
        gout = gout.to(torch.float32).contiguous()
        flat = torch.empty((tab.total,), dtype=torch.float32, device=dev)
        _call("wsplumb_l2decay_backward", dev, _p(tab.table), tab.n_chunks, _p(gout), ctx.k, _p(flat))
        # (as_strided's offset counts from the storage's start, not from flat's own first element)
        return (None,) + tuple(flat.as_strided(p.shape, p.stride(), flat.storage_offset() + off) if need else None
                               for p, off, need in zip(params, tab.offsets, ctx.needs_input_grad[1:]))


def l2_decay(params, k):
    """sum(sum(p * p) for p in params) * k as a 0-dim f32 tensor on the parameters' device (l2decay_usable)."""
    return _L2DecayFn.apply(float(k), *params)
