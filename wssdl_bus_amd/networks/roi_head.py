"""Per-RoI ResNet head (group3 ... gap) as NHWC GEMMs.

Reference wiring: code/lib/networks/Resnet_train_bus.py:91-97 (group3 -> norm -> relu -> gap),
blocks network.py:457-491.  The number of RoIs changes from step to step (NMS keeps a
data-dependent count), and MIOpen re-tunes / re-compiles convolution kernels for every new
batch dimension (tens of seconds per new R on this stack), so the head does not use
convolution kernels at all: RoI-pool output is already [R,7,7,C] NHWC, 1x1 convs are
F.linear on [R*h*w, C] rows, 3x3 convs gather their TF-'SAME' patches and run one GEMM, and
normalisation is batch-norm over rows.  GEMMs (rocBLAS/hipBLASLt) are shape-agnostic.
Plumbing, not the product: stock PyTorch ops, except that batch-norm (+ReLU) runs on the
fused kernels of csrc/plumbing/rowbn.hip when that library is built (the activations are
[R*h*w, C] with up to ~4e5 rows: separate elementwise passes over them were a third of the
step).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _plumbing
from .backbones import RESNET_DEFS, _same_pad


class _RowBatchNormFn(torch.autograd.Function):
    """Training-mode batch norm over the rows of [M, C] built from column reductions
    (`var_mean`, `sum`) and fused elementwise ops (stock PyTorch; used on the CPU and when the
    plumbing library is not built).  PyTorch's native channels-last batch-norm kernels take
    12 ms forward+backward on a [136k, 2048] f32 tensor on MI355X; this form about 2.5 ms."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        var, mean = torch.var_mean(x, dim=0, unbiased=False)
        rstd = torch.rsqrt(var + eps)
        scale = rstd * weight
        y = torch.addcmul(bias - mean * scale, x, scale)
        ctx.save_for_backward(x, mean, rstd, weight)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        x, mean, rstd, weight = ctx.saved_tensors
        m = x.shape[0]
        sum_dy = dy.sum(0)
        sum_dy_x = (dy * x).sum(0)
        sum_dy_xhat = (sum_dy_x - mean * sum_dy) * rstd
        # dx = w*rstd * (dy - mean(dy) - xhat * mean(dy*xhat)),  xhat = (x - mean) * rstd
        a = weight * rstd
        k1 = a * rstd * sum_dy_xhat / m                  # multiplies (x - mean)
        k0 = a * sum_dy / m - k1 * mean                  # constant per column: a*mean(dy) - k1*mean
        dx = torch.addcmul(-k0, dy, a)
        dx.addcmul_(x, -k1)
        return dx, sum_dy_xhat, sum_dy, None


def _side_outputs(ctx, count, placeholder, *side):
    """Shared end of the fused Functions' forwards: the statistics and the live-row count they return next to the
    activations carry no gradient.  Without a mask the count is a placeholder view of `placeholder` (unused: no extra
    launch).  Returns the count to hand out."""
    if count is None:
        count = placeholder[0, :1]
    ctx.mark_non_differentiable(*side, count)
    ctx.set_materialize_grads(False)                   # no zero-filled gradients for the side outputs
    return count


class _FusedRowBatchNormFn(torch.autograd.Function):
    """The same layer (optionally with its ReLU) on the fused HIP kernels of
    csrc/plumbing/rowbn.hip: 3 passes over the tensor forward, 5 backward, instead of 5 + 14
    with separate elementwise ops; the ReLU mask is recomputed from x in the backward.  `running`
    (_plumbing.running_of: the layer's buffers, not autograd inputs) are updated by the forward kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu, roi_mask=None, pos_major=False, running=None):
        y, stats, count = _plumbing.rowbn_forward(x, weight, bias, eps, relu, roi_mask, pos_major, running=running)
        ctx.save_for_backward(x, weight, stats, roi_mask)
        ctx.relu, ctx.pos_major = relu, pos_major
        mean, var = stats[0], stats[1]
        return y, mean, var, _side_outputs(ctx, count, stats, mean, var)

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar, _dcount):
        x, weight, stats, roi_mask = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(x)
        dx, dw, db = _plumbing.rowbn_backward(x, dy.contiguous(), weight, stats, ctx.relu, roi_mask, ctx.pos_major)
        return dx, dw, db, None, None, None, None, None


class _JoinFn(torch.autograd.Function):
    """The end of a block on the position-major route in one Function: out = bn3(x3) + other, where other is the
    identity shortcut or (with the shortcut norm's weight / bias) bn_s(xs), then y = relu(bn_n(out)) with the next
    block's pre-activation norm or the head's final norm.  The join kernels of csrc/plumbing/rowbn.hip apply
    bn3 (and bn_s), add and take bn_n's statistics in one pass over the tensors, and in the backward form
    g = bn_n's dx + the residual gradient together with the sums bn3's (bn_s's) backward takes over it; results
    are bit-identical to the separate layers and torch's adds.  Returns out, y, the three [5, C] statistic
    blocks (stats_s is not written in the identity form) and the live-row count."""

    @staticmethod
    def forward(ctx, x3, other, w3, b3, ws, bs, wn, bn, eps3, eps_s, eps_n, roi_mask, running=None):
        dual = ws is not None
        out, y, st3, sts, stn, count = _plumbing.rowbn_join_forward(
            x3, (w3, b3, eps3), other, (ws, bs, eps_s) if dual else None, (wn, bn, eps_n), roi_mask, running=running)
        ctx.dual = dual
        ctx.save_for_backward(x3, other if dual else None, out, w3, ws, wn, st3, sts, stn, roi_mask)
        return out, y, st3, sts, stn, _side_outputs(ctx, count, stn, st3, sts, stn)

    @staticmethod
    def backward(ctx, dres, dy, *_):
        x3, xs, out, w3, ws, wn, st3, sts, stn, roi_mask = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(out)
        g, dx3, dxs, dwbn, dwb3, dwbs = _plumbing.rowbn_join_backward(
            out, dy.contiguous(), dres.contiguous() if dres is not None else None, x3, xs, wn, stn, w3, st3, ws, sts,
            roi_mask)
        if ctx.dual:
            return dx3, dxs, dwb3[0], dwb3[1], dwbs[0], dwbs[1], dwbn[0], dwbn[1], None, None, None, None, None
        return dx3, g, dwb3[0], dwb3[1], None, None, dwbn[0], dwbn[1], None, None, None, None, None


class _EntryNormFn(torch.autograd.Function):
    """Block 1's pre-activation norm + ReLU on the position-major route, with both consumers of its output y in
    one Function: returns y (roi-major rows, for conv1) and the position-major rows of the positions the
    projection shortcut samples (_pm_rows).  The backward takes the two gradients as they arrive and forms
    their sum inside the norm's two backward passes (rowbn.hip, EntryGrad): no zero-fill, index_add, strided
    add or contiguous copy of a [R, 49, C] tensor.  Bit-identical to the separate layers."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, roi_mask, plan, s, hw, running=None):
        y, stats, count = _plumbing.rowbn_forward(x, weight, bias, eps, True, roi_mask, False, running=running)
        h, w = hw
        r = x.shape[0] // (h * w)
        ys = _pm_rows(y.view(r, h, w, -1), plan, s)
        ctx.save_for_backward(x, weight, stats, roi_mask)
        ctx.geom = (plan, s, h, w)
        mean, var = stats[0], stats[1]
        return y, ys, mean, var, _side_outputs(ctx, count, stats, mean, var)

    @staticmethod
    def backward(ctx, dy, dys, *_):
        x, weight, stats, roi_mask = ctx.saved_tensors
        plan, s, h, w = ctx.geom
        if dy is None:
            dy = torch.zeros_like(x)
        if dys is None:
            dys = x.new_zeros((len(plan.slots) * (x.shape[0] // (h * w)), x.shape[1]))
        dx, dw, db = _plumbing.rowbn_backward_entry(x, dy.contiguous(), dys.contiguous(),
                                                    plan.subsample_slots(h, w, s, x.device), len(plan.slots), weight,
                                                    stats, roi_mask)
        return dx, dw, db, None, None, None, None, None, None


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


def _masked_row_batch_norm(x, weight, bias, eps, relu, roi_mask, pos_major=False):
    M = x.shape[0]
    per = M // roi_mask.shape[0]
    m = (roi_mask.repeat(per) if pos_major else roi_mask.repeat_interleave(per)).unsqueeze(1)
    n = (roi_mask.sum() * per).clamp_min(1.0)
    mean = (x * m).sum(0) / n
    d = (x - mean) * m
    var = (d * d).sum(0) / n
    y = d * (torch.rsqrt(var + eps) * weight) + bias
    if relu:
        y = F.relu(y)
    return y * m, mean.detach(), var.detach(), n


class RowBatchNorm(nn.Module):
    """BatchNorm over rows ([M, C] input) with the usual running statistics; `relu=True`
    applies the ReLU that follows it in the network inside the same kernels.  Rows are roi-major
    (row r belongs to RoI r // (M / R)) or, with `pos_major=True`, position-major (RoI r % R): only
    the live-row mask cares."""

    def __init__(self, num_features, eps=1e-3, momentum=0.01):
        super().__init__()
        self.eps, self.momentum = eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def forward(self, x, relu=False, pos_major=False):
        fused = _plumbing.usable(x)
        if not self.training:
            scale = self.weight * torch.rsqrt(self.running_var + self.eps)
            shift = self.bias - self.running_mean * scale
            if fused and not torch.is_grad_enabled():
                return _plumbing.rowbn_apply(x, scale.contiguous(), shift.contiguous(), relu)
            y = torch.addcmul(shift, x, scale)
            return F.relu(y) if relu else y
        # on the fused route the forward kernels update the running statistics themselves (run is not None)
        run = _plumbing.running_of(self) if fused else None
        mask = _ROI_MASK
        if fused and (mask is None or x.shape[0] % mask.shape[0] == 0):
            y, mean, var, n = _FusedRowBatchNormFn.apply(x, self.weight, self.bias, self.eps, bool(relu), mask,
                                                         bool(pos_major) and mask is not None, run)
            if run is not None:
                return y
            n = n[0] if mask is not None else x.shape[0]
        elif mask is not None:
            y, mean, var, n = _masked_row_batch_norm(x, self.weight, self.bias, self.eps, relu, mask, pos_major)
        else:
            y, mean, var = _RowBatchNormFn.apply(x, self.weight, self.bias, self.eps)
            if relu:
                y = F.relu(y)
            n = x.shape[0]
        self._track(mean, var, n)
        return y

    def _track(self, mean, var, n):
        """running statistics from one batch's mean / biased variance over n rows (n: an int, or the live-row
        count as a 0-d tensor)."""
        with torch.no_grad():
            unbias = n / (n - 1).clamp_min(1.0) if torch.is_tensor(n) else n / max(n - 1, 1)
            self.running_mean.lerp_(mean, self.momentum)
            self.running_var.lerp_(var * unbias, self.momentum)


class ConvNHWC(nn.Module):
    """conv (TF 'SAME') + optional BN + optional ReLU on NHWC tensors via one GEMM.
    weight [c_o, k*k*c_i] with the patch laid out (kh, kw, c_i)."""

    def __init__(self, c_i, c_o, k, s, norm=None, relu=True):
        super().__init__()
        self.c_i, self.c_o, self.k, self.s, self.relu = c_i, c_o, k, s, relu
        self.weight = nn.Parameter(torch.empty(c_o, k * k * c_i))
        nn.init.trunc_normal_(self.weight, std=0.01, a=-0.02, b=0.02)
        self.bias = nn.Parameter(torch.zeros(c_o)) if norm is None else None
        self.bn = RowBatchNorm(c_o) if norm == "BN" else None

    def forward(self, x):
        r, h, w, c = x.shape
        k, s = self.k, self.s
        if k == 1:
            if s > 1:
                x = x[:, ::s, ::s, :]
            oh, ow = x.shape[1], x.shape[2]
            rows = x.reshape(-1, c)
        elif k == 3 and _plumbing.im2col_usable(x):
            pt, pb = _same_pad(h, k, s)
            pl, pr = _same_pad(w, k, s)
            oh, ow = -(-h // s), -(-w // s)
            rows = _plumbing.Im2Col3x3Fn.apply(x, s, oh, ow, pt, pl)
        else:
            pt, pb = _same_pad(h, k, s)
            pl, pr = _same_pad(w, k, s)
            xp = F.pad(x, (0, 0, pl, pr, pt, pb))
            p = xp.unfold(1, k, s).unfold(2, k, s)            # [R, oh, ow, C, kh, kw]
            oh, ow = p.shape[1], p.shape[2]
            rows = p.permute(0, 1, 2, 4, 5, 3).reshape(-1, k * k * c)
        return self._act(F.linear(rows, self.weight, self.bias)).view(r, oh, ow, self.c_o)

    def _act(self, y, pos_major=False):
        if self.bn is not None:
            return self.bn(y, relu=self.relu, pos_major=pos_major)
        return F.relu(y) if self.relu else y

    # ---- position-major route of the head's 4x4 section (ResNetHeadNHWC.forward) ----
    def forward_pm(self, x, plan, R, act=True):
        """x: roi-major [R, h, w, C] or position-major [rows, C] rows in `plan`'s slot order; returns
        position-major rows.  3x3: the class-packed GEMMs of `plan` (TapConv3x3Fn); 1x1 at stride s on a
        roi-major input: the input positions of the slots, then a row GEMM; 1x1 on rows: a row GEMM.
        act=False: the convolution's raw output (its norm is applied by the block's join, _join_pm)."""
        if self.k == 3:
            y = _plumbing.TapConv3x3Fn.apply(x, self.weight, self.bias, plan, x.dim() == 2, R)
        else:
            if x.dim() == 4:
                x = _pm_rows(x, plan, self.s)
            y = F.linear(x, self.weight, self.bias)
        return self._act(y, pos_major=True) if act else y


def _pm_rows(x, plan, s):
    """roi-major [R, h, w, C] -> position-major [slots * R, C]: the inputs x[:, y*s, x*s] of the slots."""
    r, h, w, c = x.shape
    idx = plan.subsample_index(w, s, x.device)
    return x.view(r, h * w, c).transpose(0, 1).index_select(0, idx).reshape(-1, c)


def _bn_rows(bn, x, relu=False):
    r, h, w, c = x.shape
    return bn(x.reshape(-1, c), relu=relu).view(r, h, w, c)


class BottleneckNHWC(nn.Module):
    expansion = 4

    def __init__(self, c_i, c_o, s, preact, norm):
        super().__init__()
        self.preact = preact
        self.pre_bn = RowBatchNorm(c_i) if (preact != "no_preact" and norm == "BN") else None
        self.conv1 = ConvNHWC(c_i, c_o, 1, 1, norm)
        self.conv2 = ConvNHWC(c_o, c_o, 3, s, norm)
        self.conv3 = ConvNHWC(c_o, c_o * 4, 1, 1, norm, relu=False)
        self.short = ConvNHWC(c_i, c_o * 4, 1, s, norm, relu=False) if c_i != c_o * 4 else None

    def forward(self, x):
        ori = x
        if self.preact != "no_preact":
            y = _bn_rows(self.pre_bn, x, relu=True) if self.pre_bn is not None else F.relu(x)
            if self.preact == "both_preact":
                ori = y
            x = y
        x = self.conv3(self.conv2(self.conv1(x)))
        return x + (self.short(ori) if self.short is not None else ori)

    def forward_pm(self, x, plans, R, pre=None, nxt=None):
        """forward on the position-major route: x roi-major [R, 7, 7, C] (first block) or position-major rows;
        plans: {stride: TapPlan}; pre: this block's pre-activation when the previous block's join computed it;
        nxt: the norm (+ReLU) that follows this block.  Returns (position-major rows, nxt's output or None)."""
        pm = x.dim() == 2
        ori = x
        s = self.conv2.s
        plan = plans[s]
        if self._entry_fused(x, pre):
            x, ori = _entry_pre_act(self.pre_bn, x, plan, s)   # ori: the shortcut's rows, already position-major
        elif self.preact != "no_preact":
            y = pre if pre is not None else _pre_act(self.pre_bn, x, pm)
            if self.preact == "both_preact":
                ori = y
            x = y
        if not pm:
            x = self.conv1(x)                                   # 1x1 on the roi-major 7x7 map
        else:
            x = self.conv1.forward_pm(x, plan, R)
        x = self.conv3.forward_pm(self.conv2.forward_pm(x, plan, R), plan, R, act=False)
        return _join_pm(self.conv3, x, self.short, ori, plan, s, R, nxt)


    def _entry_fused(self, x, pre):
        """True when this is block 1 of the position-major route in the form _EntryNormFn covers: a roi-major
        input, a training-mode pre-activation norm whose output feeds both conv1 and a projection shortcut."""
        bn, mask = self.pre_bn, _ROI_MASK
        if x.dim() != 4 or pre is not None or self.preact != "both_preact" or self.short is None or bn is None:
            return False
        rows = x.reshape(-1, x.shape[3])
        return (bn.training and torch.is_grad_enabled() and _plumbing.entry_usable(rows)
                and (mask is None or rows.shape[0] % mask.shape[0] == 0))


class BasicBlockNHWC(nn.Module):
    expansion = 1

    def __init__(self, c_i, c_o, s, preact, norm):
        super().__init__()
        self.preact = preact
        self.pre_bn = RowBatchNorm(c_i) if (preact != "no_preact" and norm == "BN") else None
        self.conv1 = ConvNHWC(c_i, c_o, 3, s, norm)
        self.conv2 = ConvNHWC(c_o, c_o, 3, 1, norm, relu=False)
        self.short = ConvNHWC(c_i, c_o, 1, s, norm, relu=False) if c_i != c_o else None

    def forward(self, x):
        ori = x
        if self.preact != "no_preact":
            y = _bn_rows(self.pre_bn, x, relu=True) if self.pre_bn is not None else F.relu(x)
            if self.preact == "both_preact":
                ori = y
            x = y
        x = self.conv2(self.conv1(x))
        return x + (self.short(ori) if self.short is not None else ori)

    def forward_pm(self, x, plans, R, pre=None, nxt=None):
        """BottleneckNHWC.forward_pm for the basic block."""
        pm = x.dim() == 2
        ori = x
        if self.preact != "no_preact":
            y = pre if pre is not None else _pre_act(self.pre_bn, x, pm)
            if self.preact == "both_preact":
                ori = y
            x = y
        s = self.conv1.s
        plan = plans[s]
        x = self.conv2.forward_pm(self.conv1.forward_pm(x, plan, R), plans[1], R, act=False)
        return _join_pm(self.conv2, x, self.short, ori, plan, s, R, nxt)


def _join_pm(last, x3, short, ori, plan, s, R, nxt):
    """The end of a block (stride s) on the position-major route: act(x3) + shortcut, x3 the raw output of the
    block's last convolution `last`.  Returns (out, relu(nxt(out))) from the join kernels (_JoinFn) when `nxt` is given and
    every norm involved is a training-mode RowBatchNorm on a tensor the kernels take; else (out, None) from the
    separate layers (also with WSSDL_HEAD_UNFUSED_JOIN=1)."""
    if short is not None:
        xs = short.forward_pm(ori, plan, R, act=False)
    else:
        xs = ori if ori.dim() == 2 else _pm_rows(ori, plan, s)
    bns = [last.bn, nxt] + ([short.bn] if short is not None else [])
    mask = _ROI_MASK
    if (nxt is None or any(b is None or not b.training for b in bns) or last.relu or not _plumbing.join_usable(x3)
            or (mask is not None and x3.shape[0] % mask.shape[0] != 0)):
        return last._act(x3, pos_major=True) + (short._act(xs, pos_major=True) if short is not None else xs), None
    b3, bs = last.bn, short.bn if short is not None else None
    run = None
    if _plumbing.fused_running_stats():
        run = (_plumbing.running_of(b3), _plumbing.running_of(bs) if bs is not None else None, _plumbing.running_of(nxt))
    out, y, st3, sts, stn, n = _JoinFn.apply(
        x3, xs.contiguous(), b3.weight, b3.bias, bs.weight if bs is not None else None,
        bs.bias if bs is not None else None, nxt.weight, nxt.bias, b3.eps, bs.eps if bs is not None else 0.0, nxt.eps,
        mask, run)
    if run is not None:                                 # the join's finish kernels updated the running statistics
        return out, y
    n = n[0] if mask is not None else x3.shape[0]
    b3._track(st3[0], st3[1], n)
    if bs is not None:
        bs._track(sts[0], sts[1], n)
    nxt._track(stn[0], stn[1], n)
    return out, y


def _entry_pre_act(bn, x, plan, s):
    """Block 1's pre-activation through _EntryNormFn: (y roi-major [R, h, w, C], the shortcut's position-major rows)."""
    r, h, w, c = x.shape
    run = _plumbing.running_of(bn)
    y, ys, mean, var, n = _EntryNormFn.apply(x.reshape(-1, c), bn.weight, bn.bias, bn.eps, _ROI_MASK, plan, s, (h, w),
                                             run)
    if run is None:
        bn._track(mean, var, n[0] if _ROI_MASK is not None else r * h * w)
    return y.view(r, h, w, c), ys


def _pre_act(bn, x, pm):
    if not pm:
        return _bn_rows(bn, x, relu=True) if bn is not None else F.relu(x)
    return bn(x, relu=True, pos_major=True) if bn is not None else F.relu(x)


class ResNetHeadNHWC(nn.Module):
    """[R,7,7,C] NHWC -> [R, 512*expansion]."""

    def __init__(self, depth, norm="BN"):
        super().__init__()
        defs, block = RESNET_DEFS[depth]
        blk = BottleneckNHWC if block.expansion == 4 else BasicBlockNHWC
        e = blk.expansion
        blocks = [blk(256 * e, 512, 2, "both_preact", norm)]
        for _ in range(1, defs[3]):
            blocks.append(blk(512 * e, 512, 1, "default", norm))
        self.group3 = nn.Sequential(*blocks)
        self.norm = RowBatchNorm(512 * e) if norm == "BN" else None
        self.out_features = 512 * e

    def forward(self, x):
        plans = self._tap_plans(x)
        if plans is not None:
            return self._forward_pm(x, plans)
        x = self.group3(x)
        x = _bn_rows(self.norm, x, relu=True) if self.norm is not None else F.relu(x)
        return x.mean(dim=(1, 2))

    @staticmethod
    def _tap_plans(x):
        """The class plans of the two 3x3 shapes (h x w at stride 2, then its output at stride 1), or None
        for the dense route: CPU tensors, no plumbing library, WSSDL_HEAD_DENSE_3X3=1, fewer RoIs than
        _plumbing.TAPS_MIN_ROIS, or a geometry with no padding taps to skip or different slot orders for the
        two shapes."""
        if not _plumbing.taps_usable(x):
            return None
        p2 = _plumbing.tap_plan(x.shape[1], x.shape[2], 2)
        p1 = _plumbing.tap_plan(p2.oh, p2.ow, 1)
        if not (p2.ok and p1.ok and p1.slots == p2.slots):
            return None
        return {2: p2, 1: p1}

    def _forward_pm(self, x, plans):
        """The 4x4 section in POSITION-MAJOR rows (row = slot * R + roi, slots ordered centre | edges |
        corners by _plumbing.TapPlan): each 3x3 class GEMM writes its own contiguous slab; batch norm,
        1x1 convolutions and residual adds do not care about row order, the final mean reduces over slots."""
        R = x.shape[0]
        blocks, pre = list(self.group3), None
        for i, blk in enumerate(blocks):
            # the norm (+ReLU) after this block: the next block's pre-activation, or the final norm
            nxt = self.norm if i + 1 == len(blocks) else \
                (blocks[i + 1].pre_bn if blocks[i + 1].preact != "no_preact" else None)
            x, pre = blk.forward_pm(x, plans, R, pre, nxt)
        if pre is None:
            pre = self.norm(x, relu=True, pos_major=True) if self.norm is not None else F.relu(x)
        return pre.view(-1, R, pre.shape[1]).mean(dim=0)
