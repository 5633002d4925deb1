"""PyTorch-ROCm backbones with the reference's wiring (plumbing: stock conv / BN / pool;
the detection hot path lives in the HIP library).

Reference: code/lib/networks/network.py:100-172 (conv / conv_int), :417-545 (ResNet blocks,
layer_group, normalization), Resnet_train_bus.py:55-63,91-101, VGGnet_train_bus.py:43-101.
Tensors are NCHW-shaped in channels_last memory format, so ``x.permute(0, 2, 3, 1)`` is the
contiguous NHWC view the hot-path ops take, with no copy.  The block wiring (_preact, _init_block,
_walk) also serves the per-RoI head's NHWC blocks (roi_head.py); the norms run on rownorm.py.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _plumbing, rownorm
from ._plumbing import _same_pad


class BatchNormAct2d(nn.BatchNorm2d):
    """nn.BatchNorm2d (same parameters and buffers) whose forward can also apply the ReLU that
    follows it.  On channels_last GPU tensors in training mode the layer runs on the fused row
    batch-norm kernels of the plumbing library ([N,H,W,C] is an [N*H*W, C] row matrix there);
    anywhere else it is the stock module followed by F.relu.  `renorm=True`: batch renormalisation
    (rownorm.init_renorm) on the same kernels; where they do not take the tensor, rownorm.stock_rows over the rows."""
    renorm = False

    def __init__(self, *args, renorm=False, **kwargs):
        super().__init__(*args, **kwargs)
        if renorm:
            rownorm.init_renorm(self, self.num_features)

    def forward(self, x, relu=False):
        if self.training and x.is_cuda and self.track_running_stats:
            r2 = _rows(x)
            if r2 is not None and _plumbing.usable(r2):
                run, done = rownorm.running((self,), None, r2.shape[0])
                y, mean, var, n = rownorm._FusedRowBatchNormFn.apply(r2, self.weight, self.bias, self.eps, bool(relu),
                                                                     None, False, run,
                                                                     *((rownorm.renorm((self,)),) if self.renorm else ()))
                done(((mean, var),), n)
                return _nchw(y, x)
        if self.renorm and self.training:
            n, c, h, w = x.shape
            y = rownorm.stock_rows(self, x.permute(0, 2, 3, 1).reshape(-1, c), relu)
            return y.view(n, h, w, c).permute(0, 3, 1, 2)
        y = super().forward(x)
        return F.relu(y) if relu else y


def _bn(c):
    return BatchNormAct2d(c, eps=1e-3, momentum=0.01, renorm=bool(rownorm.cfg.TRAIN.USE_BRN))


class GroupNormAct2d(rownorm.RowGroupNorm):
    """BatchNormAct2d's counterpart for norm_type 'GN': the reference's group norm (rownorm.RowGroupNorm) of an
    [N, C, H, W] tensor, a sample being an image.  A channels_last tensor is normalised through its [N*H*W, C] row
    view with no copy; any other layout through a copy of it."""

    def forward(self, x, relu=False):
        n, c, h, w = x.shape
        r2 = _rows(x)
        if r2 is not None:
            return _nchw(super().forward(r2, n, relu=relu), x)
        y = super().forward(x.permute(0, 2, 3, 1).reshape(-1, c), n, relu=relu)
        return y.view(n, h, w, c).permute(0, 3, 1, 2)


rownorm.NORM_MAKERS[("BN", False)] = _bn
rownorm.NORM_MAKERS[("GN", False)] = lambda c: GroupNormAct2d(c, rownorm.gn_groups(c))


class Conv(nn.Module):
    """conv + optional norm (rownorm.make_norm) + optional ReLU (network.py:100-135).  TF 'SAME' padding
    is reproduced exactly (asymmetric when needed); bias only without normalisation."""

    def __init__(self, c_i, c_o, k, s, norm=None, relu=True, padding="SAME"):
        super().__init__()
        self.k, self.s, self.padding, self.relu = k, s, padding, relu
        self.conv = nn.Conv2d(c_i, c_o, k, s, 0, bias=(norm is None))
        nn.init.trunc_normal_(self.conv.weight, std=0.01, a=-0.02, b=0.02)     # :110
        if self.conv.bias is not None:
            nn.init.zeros_(self.conv.bias)
        self.bn = rownorm.make_norm(norm, c_o, rows=False)

    def forward(self, x, act=True):
        """act=False: the convolution's raw output (its norm is applied by the block's join, _join)."""
        if self.padding == "SAME" and self.k > 1:
            pt, pb = _same_pad(x.shape[2], self.k, self.s)
            pl, pr = _same_pad(x.shape[3], self.k, self.s)
            x = F.pad(x, (pl, pr, pt, pb))
        x = self.conv(x)
        return self._act(x) if act else x

    def _act(self, x):
        if self.bn is not None:
            return self.bn(x, relu=self.relu)
        return F.relu(x) if self.relu else x


def _rows(x):
    """The [N*H*W, C] row matrix of an NCHW-shaped channels_last tensor (a view), or None."""
    if x.dim() != 4:
        return None
    r = x.permute(0, 2, 3, 1)
    return r.reshape(-1, r.shape[3]) if r.is_contiguous() else None


def _nchw(rows, like):
    """_rows back: the NCHW-shaped channels_last view of the row matrix of a tensor shaped like `like`."""
    n, c, h, w = like.shape
    return rows.view(n, h, w, c).permute(0, 3, 1, 2)


def _join(last, x, short, ori, nxt):
    """The end of a trunk block: last(x) + shortcut, `last` the block's final Conv (norm, no ReLU), the shortcut
    `ori` itself or short(ori); then, when `nxt` is given, relu(nxt(out)) with the norm that follows the block.
    Returns (out, relu(nxt(out))) from the residual-join kernels (rownorm.join_rows on the [N*H*W, C] row views, no
    mask) under rownorm.join_norms' conditions when, besides, every norm is a BatchNormAct2d with running statistics,
    both sides are CUDA f32 channels_last tensors of one shape that the kernels take, and autograd is recording; else
    (out, None) from the separate layers (also with WSSDL_TRUNK_UNFUSED_JOIN=1)."""
    x3 = last(x, act=False)
    xs = short(ori, act=False) if short is not None else ori
    bns = rownorm.join_norms(last, short, nxt)
    if (bns is not None and torch.is_grad_enabled() and not _plumbing.switch("WSSDL_TRUNK_UNFUSED_JOIN")
            and all(isinstance(b, BatchNormAct2d) and b.track_running_stats for b in bns if b is not None)
            and xs.shape == x3.shape):
        r3, rs = _rows(x3), _rows(xs)
        if r3 is not None and rs is not None and _plumbing.usable(r3) and _plumbing.usable(rs):
            out, y = rownorm.join_rows(*bns, r3, rs, None)
            return _nchw(out, x3), _nchw(y, x3)
    return last._act(x3) + (short._act(xs) if short is not None else xs), None


def _norm_relu(bn, x):
    """relu(bn(x)), bn a BatchNormAct2d, a GroupNormAct2d or None."""
    return bn(x, relu=True) if bn is not None else F.relu(x)


def _preact(blk, x, pre, norm_relu):
    """What a block's residual branch and its shortcut take (network.py:424-457), as (branch input, shortcut input).
    'no_preact': both the block's input x.  Otherwise the branch takes y = relu(pre_bn(x)) -- `pre` when the previous
    block's join computed it, else norm_relu(blk.pre_bn, x) -- and the shortcut y too ('both_preact') or the raw x
    ('default')."""
    if blk.preact == "no_preact":
        return x, x
    y = pre if pre is not None else norm_relu(blk.pre_bn, x)
    return y, (y if blk.preact == "both_preact" else x)


def _init_block(blk, conv, rows, c_i, c_o, s, preact, norm):
    """The layers of a residual block of either layout (`conv`: its convolution class; `rows`: norms over row matrices,
    rownorm.make_norm) from
    blk.chain, the (kernel, carries the stride) pairs of conv1, conv2, ...: pre_bn (None without pre-activation norm),
    the chain c_i -> c_o -> ... -> c_o * expansion with no ReLU on its last member, and the projection shortcut
    `short` (None when the channel counts agree)."""
    blk.preact, blk.stride = preact, s
    blk.pre_bn = rownorm.make_norm(norm, c_i, rows) if preact != "no_preact" else None
    c_out, c = c_o * blk.expansion, c_i
    for i, (k, strided) in enumerate(blk.chain, 1):
        last = i == len(blk.chain)
        setattr(blk, "conv%d" % i, conv(c, c_out if last else c_o, k, s if strided else 1, norm, relu=not last))
        c = c_o
    blk.short = conv(c_i, c_out, 1, s, norm, relu=False) if c_i != c_out else None


def _convs(blk):
    return [getattr(blk, "conv%d" % i) for i in range(1, len(blk.chain) + 1)]


class _Block(nn.Module):
    """A trunk-layout residual block (NCHW-shaped channels_last tensors); the subclasses name their chain."""

    def __init__(self, c_i, c_o, s, preact, norm):
        super().__init__()
        _init_block(self, Conv, False, c_i, c_o, s, preact, norm)

    def forward(self, x, pre=None, nxt=None):
        """pre: this block's pre-activation when the previous block's join computed it; nxt: the norm (+ReLU)
        that follows this block.  Returns (the block's output, nxt's output or None): _join."""
        x, ori = _preact(self, x, pre, _norm_relu)
        *body, last = _convs(self)
        for conv in body:
            x = conv(x)
        return _join(last, x, self.short, ori, nxt)


class Bottleneck(_Block):
    """network.py:475-491: 1x1 -> 3x3 (stride here) -> 1x1(x4), pre-activation variants."""
    expansion, chain = 4, ((1, False), (3, True), (1, False))


class BasicBlock(_Block):
    """network.py:457-473: 3x3 (stride here) -> 3x3."""
    expansion, chain = 1, ((3, True), (3, False))


def layer_group(block, c_i, c_o, count, s, norm, first=False):
    """network.py:493-502."""
    blocks = [block(c_i, c_o, s, "no_preact" if first else "both_preact", norm)]
    for _ in range(1, count):
        blocks.append(block(c_o * block.expansion, c_o, 1, "default", norm))
    return nn.Sequential(*blocks)


def _walk(blocks, x, final, norm_relu, step=nn.Module.__call__, join=True):
    """The blocks in order through step(blk, x, pre, nxt) -> (x, pre), by default the block's forward, each told (with `join`) the norm that follows it
    -- the next block's pre-activation norm, or `final` after the last -- so that its join can apply it, and handed
    the pre-activation the previous join computed; returns relu(final(x)), from the last join or norm_relu."""
    pre = None
    for i, blk in enumerate(blocks):
        nxt = None
        if join:
            nxt = final if i + 1 == len(blocks) else blocks[i + 1].pre_bn
        x, pre = step(blk, x, pre, nxt)
    return pre if pre is not None else norm_relu(final, x)


RESNET_DEFS = {18: ([2, 2, 2, 2], BasicBlock), 34: ([3, 4, 6, 3], BasicBlock),
               50: ([3, 4, 6, 3], Bottleneck), 101: ([3, 4, 23, 3], Bottleneck)}   # Resnet_train_bus.py:32-37


class ResNetTrunk(nn.Module):
    """conv0 ... group2/relu (Resnet_train_bus.py:55-63): stride-16 feature map."""

    def __init__(self, depth, norm="BN"):
        super().__init__()
        defs, block = RESNET_DEFS[depth]
        e = block.expansion
        self.conv0 = Conv(3, 64, 7, 2, norm)
        self.group0 = layer_group(block, 64, 64, defs[0], 1, norm, first=True)
        self.group1 = layer_group(block, 64 * e, 128, defs[1], 2, norm)
        self.group2 = layer_group(block, 128 * e, 256, defs[2], 2, norm)
        self.norm = rownorm.make_norm(norm, 256 * e, rows=False)
        self.out_channels = 256 * e

    def forward(self, x):
        x = self.conv0(x)
        x = F.max_pool2d(x, 3, 2)                         # 'VALID'
        return _walk(list(self.group0) + list(self.group1) + list(self.group2), x, self.norm, _norm_relu)


class ResNetHead(nn.Module):
    """group3 -> norm -> relu -> global average pool (Resnet_train_bus.py:91-97)."""

    def __init__(self, depth, norm="BN"):
        super().__init__()
        defs, block = RESNET_DEFS[depth]
        e = block.expansion
        self.group3 = layer_group(block, 256 * e, 512, defs[3], 2, norm)
        self.norm = rownorm.make_norm(norm, 512 * e, rows=False)
        self.out_features = 512 * e

    def forward(self, x):
        return _walk(list(self.group3), x, self.norm, _norm_relu, join=False).mean(dim=(2, 3))


class VGGTrunk(nn.Module):
    """conv1_1 ... conv5_3 (VGGnet_train_bus.py:44-61); conv1_x / conv2_x are frozen there."""

    def __init__(self):
        super().__init__()
        cfgs = [(3, 64), (64, 64), "P", (64, 128), (128, 128), "P", (128, 256), (256, 256), (256, 256),
                "P", (256, 512), (512, 512), (512, 512), "P", (512, 512), (512, 512), (512, 512)]
        layers = []
        n_conv = 0
        for c in cfgs:
            if c == "P":
                layers.append(nn.MaxPool2d(2, 2))         # 'VALID'
            else:
                conv = Conv(c[0], c[1], 3, 1, None)
                n_conv += 1
                if n_conv <= 4:                           # trainable=False for conv1_1..conv2_2
                    for p in conv.parameters():
                        p.requires_grad_(False)
                layers.append(conv)
        self.features = nn.Sequential(*layers)
        self.out_channels = 512

    def forward(self, x):
        return self.features(x)


class VGGHead(nn.Module):
    """fc6 -> drop6 -> fc7 -> drop7 (VGGnet_train_bus.py:91-96); fc flattens in (C,H,W)
    order (network.py:336)."""

    def __init__(self, keep_prob=0.5):
        super().__init__()
        self.fc6 = nn.Linear(512 * 7 * 7, 512)
        self.fc7 = nn.Linear(512, 512)
        for fc in (self.fc6, self.fc7):
            nn.init.trunc_normal_(fc.weight, std=0.01, a=-0.02, b=0.02)
            nn.init.zeros_(fc.bias)
        self.drop = nn.Dropout(1.0 - keep_prob)
        self.out_features = 512

    def forward(self, x):
        x = x.reshape(x.shape[0], -1)                     # NCHW-shaped input: (C,H,W) order
        x = self.drop(F.relu(self.fc6(x)))
        return self.drop(F.relu(self.fc7(x)))
