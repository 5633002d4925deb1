"""Reference of RoIAlign for the tests, written from the definition in include/wssdl_bus_hip.h ("RoIAlign"), not from any
other code base.  Two parts:

(a) `tables`: a NumPy f32 restatement of the per-axis tables -- the same operations in the same order, every operand
    f32 -- which the device tables must equal BIT FOR BIT.

(b) `forward` / `adjoint`: f64 evaluations of top and of the gradient in the DIRECT four-corner form (a sum over the
    S x S samples and their four cells; not the separable form the kernels' structure follows), taking the f32 tables as
    given.  Because the geometry is held exactly, the discontinuities at y = -1 and y = L need no excluded cases: every
    element is compared.  With each value comes an elementwise bound

        bound = count * u * sum |wy * wx * v| / S^2,        u = 2^-24 (one f32 rounding)

    where `count` is the number of f32 roundings the kernel spends on the element (below) plus one for the second-order
    terms of (1 + u)^count.  The f64 evaluation's own error (2^-53 per operation) is far below one count.

    forward (csrc/roi_align.hip, roi_align_forward_kernel): acc += (wy * wx) * v over 4 S^2 terms, then acc / (S * S):
        1 product wy * wx + 1 product with v per term      -> 2 (each relative to its own term)
        4 S^2 - 1 additions (the first, to 0, is exact)    -> 4 S^2 - 1 (each relative to a partial sum <= sum |terms|)
        1 division                                         -> 1
        FWD_COUNT(S) = 4 S^2 + 2, + 1 = 4 S^2 + 3.

    backward (roi_align_backward_kernel): per cell, acc += g * (WY * WX) over the T (roi, bin) pairs with non-zero
    weights, then acc / (S * S).  WY = the S entries of a bin summed in order; an entry's own weight
    (lo == c ? h : 0) + (hi == c ? l : 0) is exact (lo == hi only with h = 1, l = 0):
        S - 1 additions for WY, S - 1 for WX               -> 2 S - 2 (weights are >= 0: relative to the weight itself)
        1 product WY * WX, 1 product with g                -> 2
        T - 1 additions (the first is exact)               -> T - 1
        1 division                                         -> 1
        BWD_COUNT(S, T) = T + 2 S, + 1 = T + 2 S + 1.      T is counted per cell by `adjoint`.
"""
import os

import numpy as np

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def fwd_count(S):
    return 4 * S * S + 3


def bwd_count(S, T):
    return T + 2 * S + 1


# ----------------------------------------------------------------------------------------------- (a) the tables ---
def live_rows(rois, N):
    rois = np.asarray(rois, f32)
    with np.errstate(invalid='ignore'):
        return np.isfinite(rois).all(axis=1) & (rois[:, 0] >= f32(0)) & (rois[:, 0] < f32(N))


def axis_table(a1, a2, live, L, P, S, scale, aligned):
    """(lo, hi, h, l), each [R,P,S]; all arithmetic f32 in the header's order."""
    a1, a2, scale = np.asarray(a1, f32), np.asarray(a2, f32), f32(scale)
    with np.errstate(all='ignore'):
        off = f32(0.5) if aligned else f32(0.0)
        s = a1 * scale - off
        e = a2 * scale - off
        length = e - s
        if not aligned:
            length = np.maximum(length, f32(1.0))
        binsz = length / f32(P)
        p = np.arange(P, dtype=f32)[None, :, None]
        i = np.arange(S, dtype=f32)[None, None, :]
        s, binsz = s[:, None, None], binsz[:, None, None]
        y = (s + p * binsz) + ((i + f32(0.5)) * binsz) / f32(S)
        assert y.dtype == f32
        ok = live[:, None, None] & (y >= f32(-1.0)) & (y <= f32(L))
        y = np.where(ok, y, f32(0.0))
        y = np.where(y <= f32(0.0), f32(0.0), y)
        lo = y.astype(np.int32)
        top = lo >= L - 1
        lo = np.where(top, L - 1, lo).astype(np.int32)
        hi = np.where(top, L - 1, lo + 1).astype(np.int32)
        y = np.where(top, lo.astype(f32), y)
        l = (y - lo.astype(f32)).astype(f32)
        h = (f32(1.0) - l).astype(f32)
    z = np.int32(0)
    return (np.where(ok, lo, z), np.where(ok, hi, z), np.where(ok, h, f32(0)).astype(f32), np.where(ok, l, f32(0)).astype(f32),
            ok)


def tables(rois, N, H, W, PH, PW, scale, S, aligned):
    """dict(ylo, yhi, yh, yl [R,PH,S]; xlo, xhi, xh, xl [R,PW,S]; win [R,5]) as wssdl_roi_align_tables writes them."""
    rois = np.asarray(rois, f32).reshape(-1, 5)
    live = live_rows(rois, N)
    ylo, yhi, yh, yl, yok = axis_table(rois[:, 2], rois[:, 4], live, H, PH, S, scale, aligned)
    xlo, xhi, xh, xl, xok = axis_table(rois[:, 1], rois[:, 3], live, W, PW, S, scale, aligned)
    R = len(rois)
    win = np.zeros((R, 5), np.int32)
    with np.errstate(invalid='ignore'):
        win[:, 0] = np.where(live, np.where(live, rois[:, 0], 0).astype(np.int32), -1)
    for col, (lo, hi, ok, L) in ((1, (ylo, yhi, yok, H)), (3, (xlo, xhi, xok, W))):
        win[:, col] = np.where(ok, lo, L).reshape(R, -1).min(axis=1) if R else 0
        win[:, col + 1] = np.where(ok, hi, -1).reshape(R, -1).max(axis=1) if R else 0
    return dict(ylo=ylo, yhi=yhi, yh=yh, yl=yl, xlo=xlo, xhi=xhi, xh=xh, xl=xl, win=win)


# -------------------------------------------------------------------------------- (b) f64, direct four-corner form ---
def _corners(t, r, i, j):
    """The four (row indices [PH], column indices [PW], weights [PH,PW] f64) of sample (i, j) of RoI r."""
    ys = ((t['ylo'][r, :, i], t['yh'][r, :, i]), (t['yhi'][r, :, i], t['yl'][r, :, i]))
    xs = ((t['xlo'][r, :, j], t['xh'][r, :, j]), (t['xhi'][r, :, j], t['xl'][r, :, j]))
    for yi, wy in ys:
        for xi, wx in xs:
            yield yi, xi, wy.astype(np.float64)[:, None] * wx.astype(np.float64)[None, :]


def forward(data, t, S):
    """(top f64 [R,PH,PW,C], bound f64): bound = fwd_count(S) * U * sum |wy wx v| / S^2."""
    data = np.asarray(data, np.float64)
    R, PH, PW, C = t['ylo'].shape[0], t['ylo'].shape[1], t['xlo'].shape[1], data.shape[3]
    top = np.zeros((R, PH, PW, C))
    mag = np.zeros((R, PH, PW, C))
    for r in range(R):
        n = t['win'][r, 0]
        if n < 0:
            continue
        for i in range(S):
            for j in range(S):
                for yi, xi, w in _corners(t, r, i, j):
                    v = data[n][yi[:, None], xi[None, :]]              # [PH,PW,C]
                    top[r] += w[:, :, None] * v
                    mag[r] += w[:, :, None] * np.abs(v)
    return top / (S * S), fwd_count(S) * U * mag / (S * S)


def adjoint(grad, t, shape, S):
    """(bottom_diff f64 [N,H,W,C], bound f64, touched bool [N,H,W]): every row of `grad` counts once -- a box listed
    twice contributes twice.  bound = bwd_count(S, T) * U * sum |g wy wx| / S^2 with T counted per cell."""
    grad = np.asarray(grad, np.float64)
    N, H, W, C = shape
    R, PH, PW = t['ylo'].shape[0], t['ylo'].shape[1], t['xlo'].shape[1]
    out = np.zeros(shape)
    mag = np.zeros(shape)
    terms = np.zeros((N, H, W), np.int64)
    for r in range(R):
        n = t['win'][r, 0]
        if n < 0:
            continue
        nzy = np.zeros((PH, H), bool)
        nzx = np.zeros((PW, W), bool)
        for lo, w, nz in ((t['ylo'], t['yh'], nzy), (t['yhi'], t['yl'], nzy), (t['xlo'], t['xh'], nzx), (t['xhi'], t['xl'], nzx)):
            for i in range(S):
                p = np.nonzero(w[r, :, i] != 0)[0]
                nz[p, lo[r, p, i]] = True
        terms[n] += nzy.sum(axis=0)[:, None] * nzx.sum(axis=0)[None, :]
        for i in range(S):
            for j in range(S):
                for yi, xi, w in _corners(t, r, i, j):
                    idx = (yi[:, None].repeat(PW, 1), xi[None, :].repeat(PH, 0))
                    np.add.at(out[n], idx, w[:, :, None] * grad[r])
                    np.add.at(mag[n], idx, w[:, :, None] * np.abs(grad[r]))
    count = bwd_count(S, terms)[..., None]
    return out / (S * S), count * U * mag / (S * S), terms > 0


def dense_axes(t, r, H, W):
    """Ay [PH,H], Ax [PW,W] f64 of RoI r: the separable form top_r = Ay . F_n . Ax^T / S^2."""
    PH, S = t['ylo'].shape[1:]
    PW = t['xlo'].shape[1]
    Ay, Ax = np.zeros((PH, H)), np.zeros((PW, W))
    for A, lo, hi, h, l, P in ((Ay, t['ylo'], t['yhi'], t['yh'], t['yl'], PH), (Ax, t['xlo'], t['xhi'], t['xh'], t['xl'], PW)):
        for p in range(P):
            for i in range(S):
                A[p, lo[r, p, i]] += float(h[r, p, i])
                A[p, hi[r, p, i]] += float(l[r, p, i])
    return Ay, Ax


def forward_separable(data, t, S):
    data = np.asarray(data, np.float64)
    R, PH, PW = t['ylo'].shape[0], t['ylo'].shape[1], t['xlo'].shape[1]
    _, H, W, C = data.shape
    top = np.zeros((R, PH, PW, C))
    for r in range(R):
        n = t['win'][r, 0]
        if n >= 0:
            Ay, Ax = dense_axes(t, r, H, W)
            top[r] = np.einsum('ph,hwc,qw->pqc', Ay, data[n], Ax) / (S * S)
    return top


# ------------------------------------------------------------------------------------------------------ the cases ---
SCALE = 1.0 / 16
CASES = ('mixed', 'axes', 'wide', 'many', 'empty')
_cases = {}


def _boxes(rs, count, n_images, width, height, smallest=8.0):
    x = np.sort(rs.uniform(0, width, size=(count, 2)), axis=1)
    y = np.sort(rs.uniform(0, height, size=(count, 2)), axis=1)
    x[:, 1] += smallest
    y[:, 1] += smallest
    return np.stack([rs.randint(0, n_images, size=count).astype(np.float64), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1)


def make_case(name):
    """dict(name, data [N,H,W,C] f32, rois [R,5] f32, PH, PW, scale, S (the case's own sampling), and for 'mixed' the row
    numbers of its special boxes).  Built once per process and shared: do not modify."""
    if name in _cases:
        return _cases[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    extra = {}
    if name == 'mixed':
        N, H, W, C, PH, PW, S = 3, 13, 19, 160, 7, 7, 2             # the image is 304 x 208 pixels; image 2 has no live RoI
        nan = float('nan')
        special = [
            ('tiny', (0, 100, 60, 107, 66)),                        # smaller than one cell
            ('whole', (1, 0, 0, 303, 207)),
            ('left', (0, -40, 50, 60, 120)), ('top', (1, 100, -50, 180, 40)),
            ('right', (0, 250, 60, 340, 150)), ('bottom', (1, 90, 150, 200, 260)),
            ('void', (0, 400, 300, 460, 380)),                      # every sample beyond the map
            ('band', (1, -14, -14, -2, -2)), ('band_x', (0, -12, 40, -1, 90)),      # samples in [-1, 0]
            ('flipped', (1, 200, 50, 120, 120)),                    # x2 < x1
            ('twin_a', (0, 64, 48, 160, 128)), ('twin_b', (0, 64, 48, 160, 128)),
            ('pad', (-1, 10, 10, 90, 90)), ('beyond', (3, 10, 10, 90, 90)), ('nan', (1, 20, nan, 90, 100)),
            ('inf', (0, 20, 30, float('inf'), 100)), ('pad_on_2', (-1, 0, 0, 0, 0)),
        ]
        rows = [list(map(float, b)) for _, b in special]
        rows += _boxes(rs, 41 - len(rows), 2, 300, 200).tolist()   # interior boxes of several sizes on images 0 and 1
        order = rs.permutation(41)                                  # batch indices interleaved, not sorted
        rois = np.asarray(rows, f32)[order]
        where = {int(o): k for k, o in enumerate(order)}
        extra = dict(rows={nm: where[k] for k, (nm, _) in enumerate(special)}, empty_image=2)
    elif name == 'axes':
        N, H, W, C, PH, PW, S = 2, 5, 31, 3, 3, 5, 3                # C = 3: the plain (non-vector) path; aligned=False
        rois = _boxes(rs, 12, 2, 31 * 16, 5 * 16)
        rois[0, 1:] = (-30, -20, 200, 60)
        rois[1, 1:] = (300, 40, 31 * 16 + 25, 5 * 16 + 30)
        rois[2, 1:] = (100, 30, 103, 33)
    elif name == 'wide':
        N, H, W, C, PH, PW, S = 1, 4, 4, 1024, 7, 7, 2
        rois = _boxes(rs, 9, 1, 56, 56)
        rois[0, 1:] = (0, 0, 63, 63)
    elif name == 'many':
        N, H, W, C, PH, PW, S = 2, 38, 63, 32, 7, 7, 2              # long per-tile lists
        pool = np.load(os.path.join(ROOT, 'profiles', 'roofline_rois_r8512.npy'))
        a, b = pool[pool[:, 0] == 4][:750], pool[pool[:, 0] == 5][:750]
        rois = np.empty((1500, 5), f32)
        rois[0::2], rois[1::2] = a, b
        rois[0::2, 0], rois[1::2, 0] = 0, 1
    elif name == 'empty':
        N, H, W, C, PH, PW, S = 1, 5, 6, 8, 7, 7, 2
        rois = np.zeros((0, 5), f32)
    else:
        raise KeyError(name)
    rois = np.ascontiguousarray(rois, dtype=f32).reshape(-1, 5)
    data = rs.normal(size=(N, H, W, C)).astype(f32)
    grad = rs.normal(size=(len(rois), PH, PW, C)).astype(f32)
    for a in (rois, data, grad):
        a.setflags(write=False)
    _cases[name] = dict(name=name, data=data, rois=rois, grad=grad, PH=PH, PW=PW, scale=SCALE, S=S, shape=(N, H, W, C), **extra)
    return _cases[name]


_refs = {}


def reference(name, S, aligned):
    """dict(tables, top, top_bound, diff, diff_bound, touched) of a case: computed once, shared, read-only."""
    key = (name, S, bool(aligned))
    if key not in _refs:
        c = make_case(name)
        N, H, W, C = c['shape']
        t = tables(c['rois'], N, H, W, c['PH'], c['PW'], c['scale'], S, aligned)
        top, top_bound = forward(c['data'], t, S)
        diff, diff_bound, touched = adjoint(c['grad'], t, c['shape'], S)
        _refs[key] = dict(tables=t, top=top, top_bound=top_bound, diff=diff, diff_bound=diff_bound, touched=touched)
        for v in list(_refs[key].values()) + list(t.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _refs[key]
