"""RoIAlign / its gradient on the GPU (cfg.ROI_POOL_MODE = 'align'; csrc/roi_align.hip).

Not in the reference, whose head only has RoI max pooling: bilinear sampling of every bin at S x S points, no rounding
of the RoI or of the bin edges.  include/wssdl_bus_hip.h pins the semantics (per-axis f32 arithmetic, void samples,
dead rows); parity with torchvision's or Detectron's binaries is UNPINNED.

Layouts are the RoI-pool op's: bottom_data [N,H,W,C] f32 (NHWC), bottom_rois [R,5] f32 (batch index, x1, y1, x2, y2),
top_data [R,PH,PW,C] f32.  The gradient goes to the feature map only.
"""
import numpy as np
import torch

from .. import _lib
from ..fast_rcnn.config import cfg

MODES = ('max', 'align')
TABLE_NAMES = ('ylo', 'yhi', 'yh', 'yl', 'xlo', 'xhi', 'xh', 'xl', 'win')


def pool_mode():
    """cfg.ROI_POOL_MODE, checked where it is read."""
    mode = cfg.ROI_POOL_MODE
    if mode not in MODES:
        raise ValueError("cfg.ROI_POOL_MODE must be one of %r, got %r" % (MODES, mode))
    return mode


def settings():
    """The three cfg values a snapshot records (fast_rcnn/snapshot.py)."""
    return dict(mode=pool_mode(), sampling=int(cfg.ROI_ALIGN_SAMPLING), aligned=bool(cfg.ROI_ALIGN_ALIGNED))


class _Geom(object):
    def __init__(self, shape, rois, pooled_height, pooled_width, spatial_scale, sampling_ratio, aligned):
        if len(shape) != 4:
            raise ValueError("data must be 4-dimensional")
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError("rois must be [R, 5]")
        self.nhwc = self.N, self.H, self.W, self.C = tuple(int(v) for v in shape)
        self.R = int(rois.shape[0])
        self.ph, self.pw = int(pooled_height), int(pooled_width)
        self.scale = float(spatial_scale)
        self.S = int(cfg.ROI_ALIGN_SAMPLING if sampling_ratio is None else sampling_ratio)
        if self.S == 0:
            raise ValueError("sampling_ratio 0 (adaptive sampling) is not supported: use 1, 2, 3 or 4")
        if not 1 <= self.S <= 4:
            raise ValueError("sampling_ratio must be 1, 2, 3 or 4, got %r" % (sampling_ratio,))
        self.aligned = int(bool(cfg.ROI_ALIGN_ALIGNED if aligned is None else aligned))

    def meta(self, **extra):
        return dict(N=self.N, H=self.H, W=self.W, C=self.C, R=self.R, S=self.S, aligned=self.aligned, **extra)

    def top_shape(self):
        return (self.R, self.ph, self.pw, self.C)


def _run(name, meta, export, *args):
    with _lib.timed(name, meta):
        _lib.check(getattr(_lib.lib(), export)(*(args + (_lib.stream(),))), export)


def _tables(g, rois):
    """The device buffer of the axis tables of these RoIs (header: layout) and its size."""
    nb = int(_lib.lib().wssdl_roi_align_tables_bytes(g.R, g.ph, g.pw, g.S))
    if g.R and not nb:
        raise ValueError("pooled sizes must be in 1..16, got %d x %d" % (g.ph, g.pw))
    buf = torch.empty((max(nb, 4),), dtype=torch.uint8, device=rois.device)
    _run("roi_align_tables", dict(R=g.R), "wssdl_roi_align_tables", _lib.ptr(rois), g.R, g.N, g.H, g.W, g.ph, g.pw, g.scale,
         g.S, g.aligned, _lib.ptr(buf), nb)
    return buf, nb


def _forward(g, data, tables, nb):
    top = torch.empty(g.top_shape(), dtype=torch.float32, device=data.device)
    _run("roi_align_forward", g.meta(), "wssdl_roi_align_forward", _lib.ptr(data), g.N, g.H, g.W, g.C, g.R, g.ph, g.pw, g.S,
         _lib.ptr(tables), nb, _lib.ptr(top))
    return top


def _prepare(g, tables, nb):
    """The per-(image, tile) RoI lists of the backward: they depend on the RoIs only."""
    nws = int(_lib.lib().wssdl_roi_align_backward_workspace_bytes(g.R, g.N, g.H, g.W))
    ws = torch.empty((max(nws, 4),), dtype=torch.uint8, device=tables.device)
    _run("roi_align_backward_prepare", g.meta(), "wssdl_roi_align_backward_prepare", g.R, g.N, g.H, g.W, g.ph, g.pw, g.S,
         _lib.ptr(tables), nb, _lib.ptr(ws), nws)
    return ws, nws


def _backward(g, grad, tables, nb, ws, nws):
    out = torch.empty(g.nhwc, dtype=torch.float32, device=grad.device)
    _run("roi_align_backward", g.meta(), "wssdl_roi_align_backward", _lib.ptr(grad), g.R, g.N, g.H, g.W, g.C, g.ph, g.pw, g.S,
         _lib.ptr(tables), nb, _lib.ptr(ws), nws, _lib.ptr(out))
    return out


def roi_align_tables(bottom_rois, shape, pooled_height, pooled_width, spatial_scale, sampling_ratio=None, aligned=None):
    """The axis tables of the RoIs on a map of `shape` = (N, H, W, C): a dict of NumPy arrays, ylo / yhi i32 and
    yh / yl f32 [R,PH,S], the same four for x [R,PW,S], and win i32 [R,5]."""
    rois = _lib.to_device(bottom_rois, torch.float32)
    g = _Geom(shape, rois, pooled_height, pooled_width, spatial_scale, sampling_ratio, aligned)
    with torch.cuda.device(rois.device):
        buf, nb = _tables(g, rois)
    words = buf[:nb].cpu().numpy().view(np.int32)
    out, at = {}, 0
    for name in TABLE_NAMES:
        shp = (g.R, 5) if name == 'win' else (g.R, g.ph if name[0] == 'y' else g.pw, g.S)
        n = int(np.prod(shp))
        a = words[at:at + n].reshape(shp)
        out[name] = a.view(np.float32).copy() if name[1:] in ('h', 'l') else a.copy()
        at += n
    return out


def roi_align(bottom_data, bottom_rois, pooled_height, pooled_width, spatial_scale, sampling_ratio=None, aligned=None,
              name=None):
    """Forward op: top_data."""
    as_np = _lib.wants_numpy(bottom_data, bottom_rois)
    data = _lib.to_device(bottom_data, torch.float32)
    rois = _lib.to_device(bottom_rois, torch.float32, data.device)
    g = _Geom(data.shape, rois, pooled_height, pooled_width, spatial_scale, sampling_ratio, aligned)
    with torch.cuda.device(data.device):
        tables, nb = _tables(g, rois)
        top = _forward(g, data, tables, nb)
    return top.cpu().numpy() if as_np else top


def roi_align_grad(bottom_data, bottom_rois, grad, pooled_height, pooled_width, spatial_scale, sampling_ratio=None,
                   aligned=None, name=None):
    """Backward op: gradient w.r.t. bottom_data, written in full.  Only the SHAPE of `bottom_data` is used: the array
    itself, a meta tensor or the tuple (N, H, W, C)."""
    as_np = _lib.wants_numpy(bottom_rois, grad)
    gr = _lib.to_device(grad, torch.float32)
    rois = _lib.to_device(bottom_rois, torch.float32, gr.device)
    shape = tuple(getattr(bottom_data, 'shape', bottom_data))
    g = _Geom(shape, rois, pooled_height, pooled_width, spatial_scale, sampling_ratio, aligned)
    if tuple(gr.shape) != g.top_shape():
        raise ValueError("grad must be [R, PH, PW, C] = %r, got %r" % (g.top_shape(), tuple(gr.shape)))
    with torch.cuda.device(gr.device):
        tables, nb = _tables(g, rois)
        ws, nws = _prepare(g, tables, nb)
        out = _backward(g, gr, tables, nb, ws, nws)
    return out.cpu().numpy() if as_np else out


class RoiAlignFunction(torch.autograd.Function):
    """autograd wiring of the pair: the gradient flows to the feature map only; the RoIs get None.  The tables, and the
    backward's lists when a gradient is wanted, are built right behind the forward."""

    @staticmethod
    def forward(ctx, bottom_data, bottom_rois, pooled_height, pooled_width, spatial_scale, sampling_ratio, aligned):
        data = bottom_data.contiguous()
        rois = bottom_rois.contiguous()
        if not data.is_cuda or data.dtype != torch.float32 or rois.dtype != torch.float32:
            raise _lib.HipCallError("roi_align_autograd expects float32 tensors on the GPU")
        g = _Geom(data.shape, rois, pooled_height, pooled_width, spatial_scale, sampling_ratio, aligned)
        with torch.cuda.device(data.device):
            tables, nb = _tables(g, rois)
            top = _forward(g, data, tables, nb)
            ctx.lists = _prepare(g, tables, nb) if ctx.needs_input_grad[0] else None
        ctx.geom, ctx.tables = g, (tables, nb)
        return top

    @staticmethod
    def backward(ctx, grad_top):
        g, (tables, nb) = ctx.geom, ctx.tables
        grad = grad_top.contiguous()
        with torch.cuda.device(grad.device):
            ws, nws = ctx.lists if ctx.lists is not None else _prepare(g, tables, nb)
            out = _backward(g, grad, tables, nb, ws, nws)
        return out, None, None, None, None, None, None


def roi_align_autograd(bottom_data, bottom_rois, pooled_height, pooled_width, spatial_scale, sampling_ratio=None,
                       aligned=None):
    """Differentiable roi_align: top_data."""
    return RoiAlignFunction.apply(bottom_data, bottom_rois, pooled_height, pooled_width, spatial_scale, sampling_ratio,
                                  aligned)
