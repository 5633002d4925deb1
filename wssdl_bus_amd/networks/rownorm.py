"""Batch norm and group norm over the rows of an [M, C] matrix, the one form both networks normalise in: the trunk's [N, H, W, C]
maps are [N*H*W, C] row views (backbones.BatchNormAct2d), the per-RoI head's activations are rows already
(RowBatchNorm, roi-major or position-major).  Here live the autograd Functions over the kernels of
csrc/plumbing/rowbn.hip (single norm, block-1 entry norm, residual join) with their stock-PyTorch stand-ins, the
live-row mask of the head, the one running-statistics update (`track`, `running`) and the one residual join over row
matrices (`join_norms`, `join_rows`).  Group norm (norm_type 'GN': RowGroupNorm over csrc/plumbing/groupnorm.hip)
has no batch statistics and takes none of the batch-norm fusions (`is_bn`); `make_norm` is the one place that turns a
norm_type into a module.  Batch renormalisation (cfg.TRAIN.USE_BRN: a batch-norm module built with renorm=True) is
the batch norm it is to every fusion: the kernels take its state (`renorm`) and own its update; `stock_rows` / `renorm_step`
are the same algorithm with torch ops.  Imports only _plumbing and the config; backbones.py and roi_head.py import from here.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _plumbing
from ..fast_rcnn.config import cfg


class _RowBatchNormFn(torch.autograd.Function):
    """Training-mode batch norm over the rows of [M, C] built from column reductions
    (`var_mean`, `sum`) and fused elementwise ops (stock PyTorch; used on the CPU and when the
    plumbing library is not built).  PyTorch's native channels-last batch-norm kernels take
    12 ms forward+backward on a [136k, 2048] f32 tensor on MI355X; this form about 2.5 ms.
    r, d ([C] each, or None): the factors of a batch renormalisation step (renorm_step), constants of the backward:
    y = w * (xhat * r + d) + b."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, r=None, d=None):
        var, mean = torch.var_mean(x, dim=0, unbiased=False)
        rstd = torch.rsqrt(var + eps)
        scale = rstd * weight
        shift = bias - mean * scale
        if r is not None:
            scale = scale * r
            shift = bias + weight * d - mean * scale
        y = torch.addcmul(shift, x, scale)
        ctx.save_for_backward(x, mean, rstd, weight, r, d)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        x, mean, rstd, weight, r, d = ctx.saved_tensors
        m = x.shape[0]
        sum_dy = dy.sum(0)
        sum_dy_x = (dy * x).sum(0)
        sum_dy_xhat = (sum_dy_x - mean * sum_dy) * rstd
        # dx = w*rstd * (dy - mean(dy) - xhat * mean(dy*xhat)),  xhat = (x - mean) * rstd
        a = weight * rstd
        dw = sum_dy_xhat
        if r is not None:                                # renorm: a = w*r*rstd, dweight = r*sum(g*xhat) + d*sum(g)
            a = a * r
            dw = r * sum_dy_xhat + d * sum_dy
        k1 = a * rstd * sum_dy_xhat / m                  # multiplies (x - mean)
        k0 = a * sum_dy / m - k1 * mean                  # constant per column: a*mean(dy) - k1*mean
        dx = torch.addcmul(-k0, dy, a)
        dx.addcmul_(x, -k1)
        return dx, dw, sum_dy, None, None, None


def _side_outputs(ctx, count, placeholder, *side):
    """Shared end of the fused Functions' forwards: the statistics and the live-row count they return next to the
    activations carry no gradient.  Without a mask the count is a placeholder view of `placeholder` (unused: no extra
    launch).  Returns the count to hand out."""
    if count is None:
        count = placeholder[0, :1]
    ctx.mark_non_differentiable(*side, count)
    ctx.set_materialize_grads(False)                   # no zero-filled gradients for the side outputs
    return count


def _grad(dy, like):
    """An output's gradient as the kernels take it: contiguous, zeros when autograd has none for it."""
    return dy.contiguous() if dy is not None else torch.zeros_like(like)


class _FusedRowBatchNormFn(torch.autograd.Function):
    """The same layer (optionally with its ReLU) on the fused HIP kernels of
    csrc/plumbing/rowbn.hip: 3 passes over the tensor forward, 5 backward, instead of 5 + 14
    with separate elementwise ops; the ReLU mask is recomputed from x in the backward.  `running`
    (_plumbing.running_of: the layer's buffers, not autograd inputs) are updated by the forward kernels, and so is
    `renorm`, the state of a batch renormalisation layer (_plumbing.renorm_of): the statistic block then carries the
    step's r and d, which is all the backward needs to know."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu, roi_mask=None, pos_major=False, running=None, renorm=None):
        y, stats, count = _plumbing.rowbn_forward(x, weight, bias, eps, relu, roi_mask, pos_major, running=running,
                                                  renorm=renorm)
        ctx.save_for_backward(x, weight, stats, roi_mask)
        ctx.relu, ctx.pos_major = relu, pos_major
        mean, var = stats[0], stats[1]
        return y, mean, var, _side_outputs(ctx, count, stats, mean, var)

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar, _dcount):
        x, weight, stats, roi_mask = ctx.saved_tensors
        dx, dw, db = _plumbing.rowbn_backward(x, _grad(dy, x), weight, stats, ctx.relu, roi_mask, ctx.pos_major)
        return dx, dw, db, None, None, None, None, None, None


class _JoinFn(torch.autograd.Function):
    """The end of a residual block in one Function: out = bn3(x3) + other, where other is the
    identity shortcut or (with the shortcut norm's weight / bias) bn_s(xs), then y = relu(bn_n(out)) with the next
    block's pre-activation norm or the network's final norm.  The join kernels of csrc/plumbing/rowbn.hip apply
    bn3 (and bn_s), add and take bn_n's statistics in one pass over the tensors, and in the backward form
    g = bn_n's dx + the residual gradient together with the sums bn3's (bn_s's) backward takes over it; results
    are bit-identical to the separate layers and torch's adds.  Returns out, y, the three [5, C] statistic
    blocks (stats_s is not written in the identity form) and the live-row count.  `renorm` (the norms'
    _plumbing.renorm_of, None for a plain one among them): batch renormalisation layers, [7, C] blocks.

    With exit_slots = n_slots -- the last join of the head, whose y is only ever averaged over the n_slots positions
    of each RoI -- the second output is instead feat [M / n_slots, C] = slot_mean(y): one kernel reads out once and
    y is never written; the backward takes feat's gradient and the kernels form y's, dfeat[r % R] * (1 / n_slots), in
    registers.  Bit-identical to the plain form followed by _SlotMeanFn."""

    @staticmethod
    def forward(ctx, x3, other, w3, b3, ws, bs, wn, bn, eps3, eps_s, eps_n, roi_mask, running=None, exit_slots=None,
                renorm=None):
        dual = ws is not None
        out, y, st3, sts, stn, count = _plumbing.rowbn_join_forward(
            x3, (w3, b3, eps3), other, (ws, bs, eps_s) if dual else None, (wn, bn, eps_n), roi_mask, running=running,
            exit_slots=exit_slots, renorm=renorm)
        ctx.dual, ctx.exit_slots, ctx.renorm = dual, exit_slots, _plumbing.renorm_bits(renorm)
        ctx.save_for_backward(x3, other if dual else None, out, w3, ws, wn, st3, sts, stn, roi_mask)
        return out, y, st3, sts, stn, _side_outputs(ctx, count, stn, st3, sts, stn)

    @staticmethod
    def backward(ctx, dres, dy, *_):
        x3, xs, out, w3, ws, wn, st3, sts, stn, roi_mask = ctx.saved_tensors
        n = ctx.exit_slots
        if n and dy is None:
            dy = out.new_zeros((out.shape[0] // n, out.shape[1]))
        if n and dres is not None:               # a gradient for `out` as well: y's gradient in memory, the plain form
            dy, n = _slot_mean_grad(dy, n), None
        g, dx3, dxs, dwbn, dwb3, dwbs = _plumbing.rowbn_join_backward(
            out, dy.contiguous() if n else _grad(dy, out), dres.contiguous() if dres is not None else None, x3, xs, wn,
            stn, w3, st3, ws, sts, roi_mask, exit_slots=n, renorm=ctx.renorm)
        if ctx.dual:
            return (dx3, dxs, dwb3[0], dwb3[1], dwbs[0], dwbs[1], dwbn[0], dwbn[1]) + (None,) * 7
        return (dx3, g, dwb3[0], dwb3[1], None, None, dwbn[0], dwbn[1]) + (None,) * 7


def _slot_mean_grad(dfeat, n_slots):
    """The gradient of the rows a slot mean was taken over: dfeat * (1 / n_slots) for every slot, [n_slots * R, C]."""
    return (dfeat * (1.0 / n_slots)).unsqueeze(0).expand(n_slots, *dfeat.shape).reshape(-1, dfeat.shape[1])


class _SlotMeanFn(torch.autograd.Function):
    """[n_slots * R, C] position-major rows -> [R, C], the mean over the slots in the order of the exit kernels
    (_plumbing.slot_mean; csrc/plumbing/bn_math.hip.h): what every position-major route of the head that does not take
    the last join's exit form ends in, so that all of them produce the same bits."""

    @staticmethod
    def forward(ctx, y, n_slots):
        ctx.n_slots = n_slots
        return _plumbing.slot_mean(y.contiguous(), n_slots)

    @staticmethod
    def backward(ctx, dfeat):
        return _slot_mean_grad(dfeat, ctx.n_slots), None


def _pm_rows(x, plan, s):
    """roi-major [R, h, w, C] -> position-major [slots * R, C]: the inputs x[:, y*s, x*s] of the slots."""
    r, h, w, c = x.shape
    idx = plan.subsample_index(w, s, x.device)
    return x.view(r, h * w, c).transpose(0, 1).index_select(0, idx).reshape(-1, c)


class _EntryNormFn(torch.autograd.Function):
    """Block 1's pre-activation norm + ReLU on the position-major route, with both consumers of its output y in
    one Function: returns y (roi-major rows, for conv1) and the position-major rows of the positions the
    projection shortcut samples (what _pm_rows(y) selects, written by the norm's apply pass while it holds them:
    rowbn.hip, EntryRows).  The backward takes the two gradients as they arrive and forms
    their sum inside the norm's two backward passes (rowbn.hip, EntryGrad): no zero-fill, index_add, strided
    add or contiguous copy of a [R, 49, C] tensor.  Bit-identical to the separate layers."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, roi_mask, plan, s, hw, running=None, renorm=None):
        h, w = hw
        y, ys, stats, count = _plumbing.rowbn_forward_entry(x, weight, bias, eps, plan.subsample_slots(h, w, s, x.device),
                                                            len(plan.slots), roi_mask, running=running, renorm=renorm)
        ctx.save_for_backward(x, weight, stats, roi_mask)
        ctx.geom = (plan, s, h, w)
        mean, var = stats[0], stats[1]
        return y, ys, mean, var, _side_outputs(ctx, count, stats, mean, var)

    @staticmethod
    def backward(ctx, dy, dys, *_):
        x, weight, stats, roi_mask = ctx.saved_tensors
        plan, s, h, w = ctx.geom
        if dys is None:
            dys = x.new_zeros((len(plan.slots) * (x.shape[0] // (h * w)), x.shape[1]))
        dx, dw, db = _plumbing.rowbn_backward_entry(x, _grad(dy, x), dys.contiguous(),
                                                    plan.subsample_slots(h, w, s, x.device), len(plan.slots), weight,
                                                    stats, roi_mask)
        return dx, dw, db, None, None, None, None, None, None, None


# The head can see RoI rows that are not live: the padding rows of the fixed-shape blob
# (cfg.PADDED_ROIS) and those of a supervised image that ran short of candidates under the device
# sampler (cfg.SAMPLING_RNG = 'device': the layer keeps its fixed S*128 rows, batch index -1).
# The networks set this mask ([R] f32, 1 = live) around the head call; batch statistics are
# taken over the live rows only and dead rows are zeroed after every normalisation, so that the
# live rows come out as if the blob had been compacted.  On the GPU this is the masked form of the
# fused kernels (csrc/plumbing/rowbn.hip: dead rows are not even read); elsewhere plain PyTorch ops.
# No host sync either way.
_ROI_MASK = None


def set_roi_mask(mask):
    global _ROI_MASK
    _ROI_MASK = mask


def live_mask(rows):
    """(the live-row mask or None, whether a matrix of `rows` rows can take it: none set, or its RoI count divides
    them)."""
    return _ROI_MASK, _ROI_MASK is None or rows % _ROI_MASK.shape[0] == 0


def _masked_row_batch_norm(x, weight, bias, eps, relu, roi_mask, pos_major=False, renorm=None):
    """renorm: a callable (mean, var) -> (r, d), the constants of a batch renormalisation step (renorm_step)."""
    M = x.shape[0]
    per = M // roi_mask.shape[0]
    m = (roi_mask.repeat(per) if pos_major else roi_mask.repeat_interleave(per)).unsqueeze(1)
    n = (roi_mask.sum() * per).clamp_min(1.0)
    mean = (x * m).sum(0) / n
    d = (x - mean) * m
    var = (d * d).sum(0) / n
    if renorm is not None:
        r, dd = renorm(mean.detach(), var.detach())
        y = (d * (torch.rsqrt(var + eps) * r) + dd) * weight + bias
    else:
        y = d * (torch.rsqrt(var + eps) * weight) + bias
    if relu:
        y = F.relu(y)
    return y * m, mean.detach(), var.detach(), n


def renorm_step(bn, mean, var):
    """One batch renormalisation step of the norm module `bn` with torch ops (the CPU and WSSDL_DISABLE_FUSED_BN=1; on
    the fused route the forward finish kernel does all of this, csrc/plumbing/rowbn.hip: struct Renorm): from the
    batch mean / biased variance it returns the step's constants (r, d), formed from the state BEFORE the update,
    then updates renorm_mean / renorm_stddev / renorm_weight and, from the new state, the running statistics (no
    n / (n - 1) factor on this path)."""
    with torch.no_grad():
        sigma = torch.sqrt(var + bn.eps)
        keep = 1.0 - bn.renorm_weight
        mixed_mean = bn.renorm_mean + keep * mean
        mixed_std = bn.renorm_stddev + keep * sigma
        r, d = sigma / mixed_std, (mean - mixed_mean) / mixed_std
        k = 1.0 - bn.renorm_momentum
        bn.renorm_mean.add_((mean - bn.renorm_mean) * k)
        bn.renorm_stddev.add_((sigma - bn.renorm_stddev) * k)
        bn.renorm_weight.add_((1.0 - bn.renorm_weight) * k)
        mom = bn.momentum if bn.momentum is not None else 0.1
        bn.running_mean.lerp_(bn.renorm_mean / bn.renorm_weight, mom)
        bn.running_var.lerp_((bn.renorm_stddev / bn.renorm_weight) ** 2 - bn.eps, mom)
        if getattr(bn, "num_batches_tracked", None) is not None:
            bn.num_batches_tracked += 1
    return r, d


def init_renorm(bn, num_features):
    """Turns the batch-norm module `bn` into a batch renormalisation layer (tf.layers.batch_normalization(renorm=True),
    renorm_clipping=None, renorm_momentum=0.99): three more buffers, all zero -- biased moving averages of the batch
    mean, of the batch stddev and of the constant 1, the last one per channel (all entries equal) so that a column's
    thread of the finish kernel owns its entry."""
    bn.renorm = True
    bn.renorm_momentum = 0.99
    for name in ("renorm_mean", "renorm_stddev", "renorm_weight"):
        bn.register_buffer(name, torch.zeros(num_features))


def track(bn, mean, var, n):
    """The running statistics of a norm module (RowBatchNorm or an nn.BatchNorm2d) from one batch's mean / biased
    variance over n rows, with torch ops; n: an int, or the live-row count as a 0-d / 1-element tensor."""
    with torch.no_grad():
        mom = bn.momentum if bn.momentum is not None else 0.1
        unbias = n / (n - 1).clamp_min(1.0) if torch.is_tensor(n) else n / max(n - 1, 1)
        bn.running_mean.lerp_(mean, mom)
        bn.running_var.lerp_(var * unbias, mom)
        if getattr(bn, "num_batches_tracked", None) is not None:
            bn.num_batches_tracked += 1


def running(bns, mask, rows):
    """Who updates the running statistics of the norms `bns` (None entries: norms the call does not have) around one
    fused forward over `rows` rows: returns (run, done).  `run` is the Function's `running` argument -- the norms'
    _plumbing.running_of(), bare for a single norm -- when the finish kernels update the buffers, else None; then
    done(stats, count), called after the Function with one (mean, var, ...) per norm and the live-row count it
    returned, does it with torch ops (track).  A batch renormalisation layer's buffers are always the kernels'
    (_plumbing.running_of)."""
    each = tuple(_plumbing.running_of(b) if b is not None else None for b in bns)    # None: torch tracks that norm
    run = None
    if any(r is not None for r in each):
        run = each[0] if len(bns) == 1 else each

    def done(stats, count):
        n = count[0] if mask is not None else rows
        for b, r, st in zip(bns, each, stats):
            if b is not None and r is None:
                track(b, st[0], st[1], n)
    return run, done


def renorm(bns):
    """The fused Functions' `renorm` argument for the norms `bns`: their _plumbing.renorm_of(), bare for a single norm,
    None when none of them is a batch renormalisation layer."""
    each = tuple(_plumbing.renorm_of(b) if b is not None else None for b in bns)
    if all(r is None for r in each):
        return None
    return each[0] if len(bns) == 1 else each


def join_norms(last, short, nxt):
    """The norms (bn3, bn_s or None, bn_n) of a residual block's end when the join kernels can stand for them: `nxt`
    (the norm that follows the block) is given, `last` (the block's final convolution) applies no ReLU, and every
    norm exists, is a batch norm (is_bn) and is in training mode.  Else None.  These conditions both networks share; each adds its own."""
    bns = (last.bn, nxt) + ((short.bn,) if short is not None else ())
    if nxt is None or last.relu or any(not is_bn(b) or not b.training for b in bns):
        return None
    return last.bn, short.bn if short is not None else None, nxt


def join_rows(b3, bs, nxt, r3, rs, mask, exit_slots=None):
    """out = b3(r3) + (bs(rs) if bs is not None else rs), y = relu(nxt(out)) over [M, C] row matrices through _JoinFn,
    running statistics included; returns (out, y) -- with exit_slots (_JoinFn's exit form) (out, the mean of y over
    the slots)."""
    ws, bias_s, eps_s = (bs.weight, bs.bias, bs.eps) if bs is not None else (None, None, 0.0)
    run, done = running((b3, bs, nxt), mask, r3.shape[0])
    ren = renorm((b3, bs, nxt))
    tail = (exit_slots or None, ren) if ren is not None else ((exit_slots,) if exit_slots else ())
    out, y, st3, sts, stn, n = _JoinFn.apply(r3, rs, b3.weight, b3.bias, ws, bias_s, nxt.weight, nxt.bias, b3.eps,
                                             eps_s, nxt.eps, mask, run, *tail)
    done((st3, sts, stn), n)
    return out, y


class RowBatchNorm(nn.Module):
    """BatchNorm over rows ([M, C] input) with the usual running statistics; `relu=True`
    applies the ReLU that follows it in the network inside the same kernels.  Rows are roi-major
    (row r belongs to RoI r // (M / R)) or, with `pos_major=True`, position-major (RoI r % R): only
    the live-row mask cares.  `renorm=True`: batch renormalisation (init_renorm) -- the same kernels fed other
    per-channel scalars in training mode, the same layer in evaluation mode."""
    renorm = False

    def __init__(self, num_features, eps=1e-3, momentum=0.01, renorm=False):
        super().__init__()
        self.eps, self.momentum = eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        if renorm:
            init_renorm(self, num_features)

    def forward(self, x, relu=False, pos_major=False):
        fused = _plumbing.usable(x)
        if not self.training:
            scale = self.weight * torch.rsqrt(self.running_var + self.eps)
            shift = self.bias - self.running_mean * scale
            if fused and not torch.is_grad_enabled():
                return _plumbing.rowbn_apply(x, scale.contiguous(), shift.contiguous(), relu)
            y = torch.addcmul(shift, x, scale)
            return F.relu(y) if relu else y
        mask, fits = live_mask(x.shape[0])
        if fused and fits:
            run, done = running((self,), mask, x.shape[0])
            y, mean, var, n = _FusedRowBatchNormFn.apply(x, self.weight, self.bias, self.eps, bool(relu), mask,
                                                         bool(pos_major) and mask is not None, run,
                                                         *((renorm((self,)),) if self.renorm else ()))
            done(((mean, var),), n)
            return y
        return stock_rows(self, x, relu, mask, pos_major)


def stock_rows(bn, x, relu, mask=None, pos_major=False):
    """Training-mode batch norm (or, for a renorm module, batch renormalisation) of the rows x [M, C] with stock
    PyTorch ops, the module's buffers updated: what RowBatchNorm and BatchNormAct2d run where the fused kernels do not
    take the tensor."""
    if bn.renorm:
        if mask is not None:
            return _masked_row_batch_norm(x, bn.weight, bn.bias, bn.eps, relu, mask, pos_major,
                                          lambda mean, var: renorm_step(bn, mean, var))[0]
        with torch.no_grad():
            var, mean = torch.var_mean(x, dim=0, unbiased=False)
        r, d = renorm_step(bn, mean, var)
        y = _RowBatchNormFn.apply(x, bn.weight, bn.bias, bn.eps, r, d)[0]
        return F.relu(y) if relu else y
    if mask is not None:
        y, mean, var, n = _masked_row_batch_norm(x, bn.weight, bn.bias, bn.eps, relu, mask, pos_major)
    else:
        y, mean, var = _RowBatchNormFn.apply(x, bn.weight, bn.bias, bn.eps)
        if relu:
            y = F.relu(y)
        n = x.shape[0]
    track(bn, mean, var, n)
    return y


# ---- group normalisation (norm_type 'GN') ----
def _group_norm_rows(x, samples, weight, bias, eps, groups, relu, mask, pos_major):
    """The reference's group_norm on rows with stock PyTorch ops (any G, any dtype, any device): x [M, C] is `samples`
    samples of M / samples rows -- row s * P + p, or p * S + s when position-major -- reshaped to [S, P, C/G, G]
    (channel c in group c % G), one mean and one biased variance per (sample, group).  mask [S]: zeros for its dead
    samples, whatever their rows hold."""
    M, C = x.shape
    S, P = samples, M // samples
    v = x.view(P, S, C).transpose(0, 1) if pos_major else x.view(S, P, C)
    g = v.reshape(S, P, C // groups, groups)
    var, mean = torch.var_mean(g, dim=(1, 2), unbiased=False, keepdim=True)
    y = ((g - mean) * torch.rsqrt(var + eps)).reshape(S, P, C) * weight + bias
    if relu:
        y = F.relu(y)
    if mask is not None:
        y = torch.where(mask.view(S, 1, 1) != 0, y, torch.zeros_like(y))
    return (y.transpose(0, 1) if pos_major else y).reshape(M, C)


class _FusedRowGroupNormFn(torch.autograd.Function):
    """Group norm (optionally with its ReLU) on the kernels of csrc/plumbing/groupnorm.hip: the forward keeps the
    per-(sample, group) mean / rstd, the backward recomputes the ReLU gate from x, so y is not saved."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, groups, rows_per_sample, relu, roi_mask, pos_major):
        y, mean, rstd = _plumbing.groupnorm_forward(x, rows_per_sample, weight, bias, eps, groups, relu, roi_mask,
                                                    pos_major)
        ctx.save_for_backward(x, weight, bias, mean, rstd, roi_mask)
        ctx.args = (rows_per_sample, relu, pos_major)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, rstd, roi_mask = ctx.saved_tensors
        P, relu, pos_major = ctx.args
        dx, dw, db = _plumbing.groupnorm_backward(x, dy.contiguous(), P, weight, bias, mean, rstd, relu, roi_mask,
                                                  pos_major)
        return dx, dw, db, None, None, None, None, None, None


class RowGroupNorm(nn.Module):
    """The reference's group norm over rows ([M, C] input, `samples` samples of M / samples rows each): interleaved
    groups, eps 1e-5, gamma / beta per channel as `weight` / `bias`, no buffers and no difference between training and
    evaluation.  `relu=True` applies the ReLU that follows it inside the same kernels; rows are sample-major or, with
    `pos_major=True`, position-major.  The head's live-row mask, when set, is the live-sample mask (one entry per
    RoI).  On the fused kernels when they take the tensor (_plumbing.groupnorm_usable), else stock PyTorch ops."""

    def __init__(self, num_features, groups, eps=1e-5):
        super().__init__()
        if groups < 1 or num_features % groups:
            raise ValueError("group norm: %d channels do not split into %d groups" % (num_features, groups))
        self.groups, self.eps = groups, eps
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))

    def forward(self, x, samples, relu=False, pos_major=False):
        M = x.shape[0]
        if samples < 1 or M % samples:
            raise ValueError("group norm: %d rows are not %d samples" % (M, samples))
        mask = _ROI_MASK
        if mask is not None and mask.shape[0] != samples:
            raise ValueError("group norm: the live-row mask has %d entries for %d samples" % (mask.shape[0], samples))
        if M and _plumbing.groupnorm_usable(x, M // samples, self.groups):
            return _FusedRowGroupNormFn.apply(x, self.weight, self.bias, self.eps, self.groups, M // samples,
                                              bool(relu), mask, bool(pos_major))
        return _group_norm_rows(x, samples, self.weight, self.bias, self.eps, self.groups, relu, mask, pos_major)


def is_bn(norm):
    """True for a batch-norm module: what the batch-norm fusions (joins, entry, the norm inside the patch gather) may
    stand for.  None and group norms are not."""
    return norm is not None and not isinstance(norm, RowGroupNorm)


def apply_norm(norm, x, samples, relu, pos_major=False):
    """norm(x) over [M, C] rows for either kind of row norm; `samples` (what a group norm needs) is the RoI count."""
    if isinstance(norm, RowGroupNorm):
        return norm(x, samples, relu=relu, pos_major=pos_major)
    return norm(x, relu=relu, pos_major=pos_major)


def gn_groups(c):
    """The reference's group count for c channels (network.py:126): min(GN_MIN_NUM_G, c // GN_MIN_CHS_PER_G), at most c."""
    return max(min(cfg.TRAIN.GN_MIN_NUM_G, c // cfg.TRAIN.GN_MIN_CHS_PER_G, c), 1)


# (kind, rows) -> factory(c).  rows=True: modules over [M, C] rows (the head); rows=False: over NCHW-shaped tensors
# (the trunk, the NCHW head), registered by backbones.py.
# A 'BN' factory reads cfg.TRAIN.USE_BRN when it is called (the reference's renorm=cfg.TRAIN.USE_BRN): batch
# renormalisation then.
NORM_MAKERS = {("BN", True): lambda c: RowBatchNorm(c, renorm=bool(cfg.TRAIN.USE_BRN)),
               ("GN", True): lambda c: RowGroupNorm(c, gn_groups(c))}


def make_norm(kind, c, rows):
    """The norm module of a site with c channels: None for kind None, batch norm for 'BN' (batch renormalisation with
    cfg.TRAIN.USE_BRN, read here, at construction), group norm for 'GN' (group count from cfg); anything else is an
    error."""
    if kind is None:
        return None
    if kind not in ("BN", "GN"):
        raise ValueError("norm_type must be None, 'BN' or 'GN', not %r" % (kind,))
    return NORM_MAKERS[(kind, bool(rows))](c)
