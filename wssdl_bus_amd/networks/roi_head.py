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
step).  The norm layers, their autograd Functions and the live-row mask live in rownorm.py, the
block wiring shared with the trunk in backbones.py; both are re-exported here under their names.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _plumbing, rownorm
from .backbones import RESNET_DEFS, _convs, _init_block, _preact, _same_pad, _walk, layer_group
from .rownorm import (RowBatchNorm, RowGroupNorm, _EntryNormFn, _FusedRowBatchNormFn, _JoinFn, _RowBatchNormFn,  # noqa: F401
                      _SlotMeanFn, _pm_rows, set_roi_mask)


class ConvNHWC(nn.Module):
    """conv (TF 'SAME') + optional norm (rownorm.make_norm) + optional ReLU on NHWC tensors via one GEMM.
    weight [c_o, k*k*c_i] with the patch laid out (kh, kw, c_i)."""

    def __init__(self, c_i, c_o, k, s, norm=None, relu=True):
        super().__init__()
        self.c_i, self.c_o, self.k, self.s, self.relu = c_i, c_o, k, s, relu
        self.weight = nn.Parameter(torch.empty(c_o, k * k * c_i))
        nn.init.trunc_normal_(self.weight, std=0.01, a=-0.02, b=0.02)
        self.bias = nn.Parameter(torch.zeros(c_o)) if norm is None else None
        self.bn = rownorm.make_norm(norm, c_o, rows=True)

    def forward(self, x):
        r, h, w, c = x.shape
        k, s = self.k, self.s
        (pt, pb), (pl, pr) = _same_pad(h, k, s), _same_pad(w, k, s)
        if k == 1:
            if s > 1:
                x = x[:, ::s, ::s, :]
            oh, ow = x.shape[1], x.shape[2]
            rows = x.reshape(-1, c)
        elif k == 3 and _plumbing.im2col_usable(x):
            oh, ow = -(-h // s), -(-w // s)
            rows = _plumbing.Im2Col3x3Fn.apply(x, s, oh, ow, pt, pl)
        else:
            xp = F.pad(x, (0, 0, pl, pr, pt, pb))
            p = xp.unfold(1, k, s).unfold(2, k, s)            # [R, oh, ow, C, kh, kw]
            oh, ow = p.shape[1], p.shape[2]
            rows = p.permute(0, 1, 2, 4, 5, 3).reshape(-1, k * k * c)
        return self._act(F.linear(rows, self.weight, self.bias), r).view(r, oh, ow, self.c_o)

    def _act(self, y, R, pos_major=False):
        """norm and ReLU over the rows y of R RoIs (a group norm's samples)."""
        if self.bn is not None:
            return rownorm.apply_norm(self.bn, y, R, self.relu, pos_major)
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
        return self._act(y, R, pos_major=True) if act else y


def _norm_tap_conv(c1, c2, rows, plan, in_pm, R, mask):
    """c2 (3x3, raw output) over relu(c1.bn(rows)) with the norm inside the patch gather (TapConv3x3Fn's norm form),
    c1.bn's running statistics included."""
    bn = c1.bn
    run, done = rownorm.running((bn,), mask, rows.shape[0])
    y, mean, var, n = _plumbing.TapConv3x3Fn.apply(rows, c2.weight, None, plan, in_pm, R, bn.weight, bn.bias, bn.eps,
                                                   mask, run, *((rownorm.renorm((bn,)),) if bn.renorm else ()))
    done(((mean, var),), n)
    return y


def _norm_relu(bn, x, R=None):
    """relu(bn(x)), bn a row norm or None, x a roi-major [R, h, w, C] map or the position-major rows of R RoIs."""
    if bn is None:
        return F.relu(x)
    if x.dim() == 2:
        return rownorm.apply_norm(bn, x, R, True, pos_major=True)
    r, h, w, c = x.shape
    return rownorm.apply_norm(bn, x.reshape(-1, c), r, True).view(r, h, w, c)


class _BlockNHWC(nn.Module):
    """A residual block of the head on NHWC tensors; the subclasses name their chain."""

    def __init__(self, c_i, c_o, s, preact, norm):
        super().__init__()
        _init_block(self, ConvNHWC, True, c_i, c_o, s, preact, norm)

    def forward(self, x):
        x, ori = _preact(self, x, None, _norm_relu)
        for conv in _convs(self):
            x = conv(x)
        return x + (self.short(ori) if self.short is not None else ori)

    def forward_pm(self, x, plans, R, pre=None, nxt=None, exit=None):
        """forward on the position-major route: x roi-major [R, 7, 7, C] (first block) or position-major rows;
        plans: {stride: TapPlan}; pre: this block's pre-activation when the previous block's join computed it;
        nxt: the norm (+ReLU) that follows this block; exit: the head's _Exit when this is its last block and nxt its
        final norm.  Returns (position-major rows, nxt's output or None) -- _join_pm."""
        s = self.stride
        if self._entry_fused(x, pre):
            x, ori = _entry_pre_act(self.pre_bn, x, plans[s], s)   # ori: the shortcut's rows, already position-major
        else:
            x, ori = _preact(self, x, pre, lambda bn, t: _norm_relu(bn, t, R))
        *body, last = _convs(self)
        if self._tapnorm_fused(body, x):
            x, body = self._conv12_pm(body[0], body[1], x, plans[body[1].s], R), ()
        for conv in body:
            # a 1x1 ahead of the strided convolution keeps a roi-major map roi-major (the bottleneck's conv1 on 7x7)
            x = conv(x) if (conv.k == 1 and x.dim() == 4) else conv.forward_pm(x, plans[conv.s], R)
        x = last.forward_pm(x, plans[last.s], R, act=False)
        return _join_pm(last, x, self.short, ori, plans[s], s, R, nxt, exit)

    @staticmethod
    def _tapnorm_fused(body, x):
        """True when the body is a bottleneck's conv1 -> conv2 pair in the form TapConv3x3Fn's norm form covers: a 1x1 at
        stride 1 with a training-mode batch norm and a ReLU, then a 3x3 without a bias, on the GPU, and the switch
        WSSDL_HEAD_UNFUSED_TAPNORM not set."""
        if len(body) != 2 or _plumbing.switch("WSSDL_HEAD_UNFUSED_TAPNORM"):
            return False
        c1, c2 = body
        return (c1.k == 1 and c1.s == 1 and c1.relu and rownorm.is_bn(c1.bn) and c1.bn.training and c2.k == 3
                and c2.bias is None and x.is_cuda and _plumbing.lib() is not None)

    @staticmethod
    def _conv12_pm(c1, c2, x, plan, R):
        """conv1 -> conv2 with their norms: conv1's norm inside conv2's patch gather when the kernels take conv1's
        raw rows and the live-row mask is one entry per RoI, else the separate layers."""
        in_pm = x.dim() == 2
        rows = F.linear(x if in_pm else x.reshape(-1, x.shape[3]), c1.weight, c1.bias)
        mask, fits = rownorm.live_mask(rows.shape[0])
        if _plumbing.tapnorm_usable(rows) and fits and (mask is None or mask.shape[0] == R):
            y = _norm_tap_conv(c1, c2, rows, plan, in_pm, R, mask)
        else:
            y1 = c1._act(rows, R, pos_major=in_pm)
            y = _plumbing.TapConv3x3Fn.apply(y1 if in_pm else y1.view(R, plan.h, plan.w, -1), c2.weight, c2.bias, plan,
                                             in_pm, R)
        return c2._act(y, R, pos_major=True)

    def _entry_fused(self, x, pre):
        """True when this is block 1 of the position-major route in the form _EntryNormFn covers: a roi-major
        input, a training-mode pre-activation batch norm whose output feeds both a 1x1 conv1 (the bottleneck's; the basic
        block's 3x3 conv1 was never routed through it) and a projection shortcut."""
        bn = self.pre_bn
        if (x.dim() != 4 or pre is not None or self.preact != "both_preact" or self.short is None
                or not rownorm.is_bn(bn) or self.conv1.k != 1):
            return False
        rows = x.reshape(-1, x.shape[3])
        return (bn.training and torch.is_grad_enabled() and _plumbing.entry_usable(rows)
                and rownorm.live_mask(rows.shape[0])[1])


class BottleneckNHWC(_BlockNHWC):
    expansion, chain = 4, ((1, False), (3, True), (1, False))


class BasicBlockNHWC(_BlockNHWC):
    expansion, chain = 1, ((3, True), (3, False))


class _Exit:
    """The head's exit as its last block sees it: `n_slots` positions per RoI, and `taken`, set by the block's join
    when it returned the mean over the slots in place of the final norm's output (_JoinFn's exit form)."""

    def __init__(self, n_slots):
        self.n_slots, self.taken = n_slots, False


def _join_pm(last, x3, short, ori, plan, s, R, nxt, exit=None):
    """The end of a block (stride s) on the position-major route: act(x3) + shortcut, x3 the raw output of the
    block's last convolution `last`.  Returns (out, relu(nxt(out))) from the join kernels (rownorm.join_rows) under
    rownorm.join_norms' conditions when, besides, the kernels take x3 and the live-row mask fits its rows -- with or
    without autograd; else (out, None) from the separate layers (also with WSSDL_HEAD_UNFUSED_JOIN=1).
    With `exit` (the head's last block, nxt its final norm) the join takes its exit form unless
    WSSDL_HEAD_UNFUSED_EXIT=1 or the mask is not one entry per RoI: the second result is then the head's output
    [R, C], the mean of relu(nxt(out)) over the slots, and exit.taken is set."""
    if short is not None:
        xs = short.forward_pm(ori, plan, R, act=False)
    else:
        xs = ori if ori.dim() == 2 else _pm_rows(ori, plan, s)
    bns = rownorm.join_norms(last, short, nxt)
    mask, fits = rownorm.live_mask(x3.shape[0])
    if bns is None or not _plumbing.join_usable(x3) or not fits:
        return last._act(x3, R, pos_major=True) + (short._act(xs, R, pos_major=True) if short is not None else xs), None
    if exit is not None and _plumbing.exit_usable(x3) and (mask is None or mask.shape[0] == R):
        exit.taken = True
        return rownorm.join_rows(*bns, x3, xs.contiguous(), mask, exit.n_slots)
    return rownorm.join_rows(*bns, x3, xs.contiguous(), mask)


def _entry_pre_act(bn, x, plan, s):
    """Block 1's pre-activation through _EntryNormFn: (y roi-major [R, h, w, C], the shortcut's position-major rows)."""
    r, h, w, c = x.shape
    mask, _ = rownorm.live_mask(r * h * w)
    run, done = rownorm.running((bn,), mask, r * h * w)
    y, ys, mean, var, n = _EntryNormFn.apply(x.reshape(-1, c), bn.weight, bn.bias, bn.eps, mask, plan, s, (h, w), run,
                                             *((rownorm.renorm((bn,)),) if bn.renorm else ()))
    done(((mean, var),), n)
    return y.view(r, h, w, c), ys


class ResNetHeadNHWC(nn.Module):
    """[R,7,7,C] NHWC -> [R, 512*expansion]."""

    def __init__(self, depth, norm="BN"):
        super().__init__()
        defs, block = RESNET_DEFS[depth]
        blk = BottleneckNHWC if block.expansion == 4 else BasicBlockNHWC
        e = blk.expansion
        self.group3 = layer_group(blk, 256 * e, 512, defs[3], 2, norm)
        self.norm = rownorm.make_norm(norm, 512 * e, rows=True)
        self.out_features = 512 * e

    def forward(self, x):
        plans = self._tap_plans(x)
        if plans is not None:
            return self._forward_pm(x, plans)
        return _norm_relu(self.norm, self.group3(x)).mean(dim=(1, 2))

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
        1x1 convolutions and residual adds do not care about row order, the final mean reduces over slots -- inside
        the last block's join (its exit form), else by the slot-mean kernel over the final norm's output: one order
        of additions (csrc/plumbing/bn_math.hip.h) on every position-major route, so that they agree bit for bit."""
        R = x.shape[0]
        blocks = list(self.group3)
        exit = _Exit(len(plans[1].slots))

        def step(blk, x, pre, nxt):
            last = self.norm is not None and nxt is self.norm and blk is blocks[-1]
            return blk.forward_pm(x, plans, R, pre, nxt, exit if last else None)

        y = _walk(blocks, x, self.norm, lambda bn, t: _norm_relu(bn, t, R), step)
        return y if exit.taken else _SlotMeanFn.apply(y, exit.n_slots)
