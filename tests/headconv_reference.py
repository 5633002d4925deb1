"""Shared by test_headconv_reference_cpu.py and test_gpu_headconv_reference.py: a plain float64 statement of the
per-RoI head's convolutions (csrc/plumbing/taps.hip, csrc/plumbing/im2col.hip; TapConv3x3Fn, Im2Col3x3Fn,
ConvNHWC.forward and ConvNHWC.forward_pm in networks/) and of their gradients, elementwise error bounds counted from
the arithmetic, the cases, and a torch-f32 model of the class-packed algorithm with switches that seed defects.  torch
only, on the host, no import of the package: the padding rule, the weight layout and the position classes are all
restated here.

THE REFERENCE.  torch.nn.functional.conv2d in float64 on the CPU, on NCHW views of the NHWC operands, the input
padded explicitly with F.pad by TF's own rule (same_pad): out = ceil(n / s), total = max((out - 1) s + k - n, 0),
before = total // 2, after = total - before.  The weight [c_o, k k C] is read as (c_o, kh, kw, c).  dx, dW and db come
from autograd through that convolution.  test_headconv_reference_cpu.py checks it once against six explicit loops.

THE RULE FOR BOUNDS (as in rowbn_reference.py).  u = 2^-24 is the unit roundoff of f32.  Every output element is an
f32 sum of n products, possibly in several stages (a GEMM, then a scatter that adds GEMM results); in any order and
any blocking, with or without fused multiply-add, its error is at most gamma(n) sum|terms|, gamma(n) = n u / (1 - n u)
-- so the bound holds for whatever solution the BLAS library picks, provided that it accumulates in f32.  sum|terms|
comes from the same f64 convolution and autograd run on |x|, |W|, |b|, |dy| (the operation is linear in each operand);
n comes from the same operation on all-ones operands (counts()):
  y    n = ntaps(p) C (+ 1 with a bias: the bias add); the dense route multiplies the padding's zeros too: 9 C (+ 1)
  dx   n = c_o + (number of (output position, tap) pairs that read this input position)
  dW   n = (number of output positions that hold this tap) R + (number of classes that hold it); dense: oh ow R
  db   n = oh ow R
SLACK = 1 + 2^-20 multiplies every bound (products of two error terms, the rounding of the f64 reference itself) and
is fixed in advance.  Where sum|terms| is zero the bound is zero and the output must be exactly zero.  Every element
of every output is compared.  No constant was chosen by looking at what a GPU produced.
"""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20

# name: (geometries (h, w, s), R, C, c_o) -- the smallest shapes that reach each path of taps.hip
CASES = {
    "sharp": ([(7, 7, 2), (4, 4, 1), (6, 5, 2)], 37, 8, 12),   # K <= 72: tightest bounds; R a multiple of neither chunk
    "one": ([(7, 7, 2)], 1, 8, 12),                            # a single RoI
    "flight": ([(7, 7, 2), (4, 4, 1)], 70, 128, 64),           # C/4 = 32: eight rows per pass, four rows in flight
    "onerow": ([(4, 4, 1)], 5, 40, 8),                         # C/4 = 10 does not divide 256: one row per pass
    "wide": ([(4, 4, 1)], 3, 1028, 4),                         # C/4 = 257 > 256: the c4 loop runs twice
}
PAIRS = [(name, g) for name, v in CASES.items() for g in v[0]]
SYMMETRIC = [(7, 7, 2), (4, 4, 1)]      # before = after along both axes; (6, 5, 2) has pt = 0, pb = 1


def pair_id(p):
    return "%s-%dx%ds%d" % ((p[0],) + tuple(p[1]))


def gamma(n):
    """n u / (1 - n u), n a number or a tensor of counts"""
    nu = (n.double() if torch.is_tensor(n) else float(n)) * U
    return nu / (1.0 - nu)


def same_pad(n, s, k=3):
    """TF 'SAME' along one axis -> (out, before, after)"""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


# ---------------------------------------------------------------- the f64 reference

def conv64(x, W, b, dy, s, k=3):
    """x [R, h, w, C], W [c_o, k k C] (kh, kw, c), b [c_o] or None, dy [R, oh, ow, c_o]; any float dtype, taken to f64
    on the CPU.  -> (y [R, oh, ow, c_o], dx [R, h, w, C], dW [c_o, k k C], db [c_o] or None), f64."""
    _, h, w, C = x.shape
    co = W.shape[0]
    _, pt, pb = same_pad(h, s, k)
    _, pl, pr = same_pad(w, s, k)
    xl = x.detach().double().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    Wl = W.detach().double().cpu().view(co, k, k, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    bl = None if b is None else b.detach().double().cpu().clone().requires_grad_(True)
    y = F.conv2d(F.pad(xl, (pl, pr, pt, pb)), Wl, bl, stride=s)
    g = torch.autograd.grad(y, [xl, Wl] + ([] if bl is None else [bl]), dy.detach().double().cpu().permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1).contiguous(), g[0].permute(0, 2, 3, 1).contiguous(),
            g[1].permute(0, 2, 3, 1).reshape(co, k * k * C).contiguous(), None if bl is None else g[2])


@functools.lru_cache(maxsize=None)
def counts(h, w, s, k=3):
    """The term counts of one geometry, from the reference convolution itself on all-ones operands (R = C = 1):
    ntaps [oh, ow] valid taps per output position; pairs [h, w] (output position, tap) pairs that read each input
    position; npos [k k] output positions that hold each tap; ncls [k k] position classes (distinct sets of valid
    taps) that hold each tap; valid [oh ow, k k] bool."""
    oh, ow = same_pad(h, s, k)[0], same_pad(w, s, k)[0]
    one = torch.ones
    ntaps, pairs, npos, _ = conv64(one(1, h, w, 1), one(1, k * k), None, one(1, oh, ow, 1), s, k)
    sel, _, _, _ = conv64(one(1, h, w, 1), torch.eye(k * k), None, one(1, oh, ow, k * k), s, k)
    valid = sel.reshape(oh * ow, k * k) > 0.5
    kinds = {tuple(row) for row in valid.tolist()}
    ncls = torch.tensor([sum(1 for kind in kinds if kind[t]) for t in range(k * k)], dtype=torch.float64)
    return dict(oh=oh, ow=ow, ntaps=ntaps.reshape(oh, ow).round(), pairs=pairs.reshape(h, w).round(),
                npos=npos.reshape(k * k).round(), ncls=ncls, valid=valid)


def reference(x, W, b, dy, s, k=3):
    """The four outputs in f64 with sum|terms| of every element and the geometry's counts."""
    R, h, w, C = x.shape
    y, dx, dW, db = conv64(x, W, b, dy, s, k)
    my, mdx, mdW, mdb = conv64(x.abs(), W.abs(), None if b is None else b.abs(), dy.abs(), s, k)
    return dict(y=y, dx=dx, dW=dW, db=db, m_y=my, m_dx=mdx, m_dW=mdW, m_db=mdb, R=R, C=C, co=W.shape[0], k=k,
                cnt=counts(h, w, s, k))


def bounds(ref, dense=False):
    """gamma(n) sum|terms| SLACK per element of y, dx, dW (and db with a bias); the counts as in the module's
    docstring, `dense` for the route that multiplies the padding taps' zeros (Im2Col3x3Fn + F.linear)."""
    cnt, R, C, co, k = ref["cnt"], ref["R"], ref["C"], ref["co"], ref["k"]
    oh, ow = cnt["oh"], cnt["ow"]
    bias = 0 if ref["db"] is None else 1
    n_y = (torch.full((oh, ow), float(k * k * C)) if dense else cnt["ntaps"] * C) + bias
    n_dx = co + cnt["pairs"]
    n_dW = torch.full((k * k,), float(oh * ow * R)) if dense else cnt["npos"] * R + cnt["ncls"]
    out = dict(y=gamma(n_y).view(1, oh, ow, 1) * ref["m_y"] * SLACK,
               dx=gamma(n_dx).unsqueeze(0).unsqueeze(3) * ref["m_dx"] * SLACK,
               dW=(gamma(n_dW).view(1, k * k, 1) * ref["m_dW"].view(co, k * k, C)).reshape(co, k * k * C) * SLACK)
    if bias:
        out["db"] = gamma(oh * ow * R) * ref["m_db"] * SLACK
    return out


# ---------------------------------------------------------------- comparison

def ratio(got, ref, bound):
    """worst |got - ref| / bound over all elements (0 where the error is 0, inf where a bound of 0 is missed or the
    value is not finite)"""
    err = (got.detach().double().cpu() - ref.double()).abs()
    if not torch.is_tensor(bound):
        bound = torch.full_like(err, float(bound))
    assert err.shape == bound.shape, (tuple(err.shape), tuple(bound.shape))
    r = err / bound.clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where((err > 0) & (bound <= 0), torch.full_like(r, float("inf")), r)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def ratios(ref, got, dense=False, prefix=""):
    """got: dict with y, dx, dW and, with a bias, db in the reference's layouts (roi-major NHWC, [c_o, k k C]) ->
    worst |error| / bound per output"""
    bd = bounds(ref, dense)
    assert set(got) == set(bd), (sorted(got), sorted(bd))
    return {prefix + name: ratio(got[name], ref[name], bd[name]) for name in ("y", "dx", "dW", "db") if name in bd}


def check_ratios(case, ratios_, log=None):
    """prints and asserts every worst |error| / bound of one case; log keeps the worst per output"""
    for name, r in ratios_.items():
        print("headconv-ratio %s %.4g %s" % (name, r, case))
        if log is not None:
            log[name] = max(log.get(name, 0.0), r)
    for name, r in ratios_.items():
        assert r <= 1.0, "%s: %s misses its bound, worst |error| / bound = %.4g" % (case, name, r)


# ---------------------------------------------------------------- cases

@functools.lru_cache(maxsize=None)
def make_case(name, geom):
    """One case on the CPU in f32 (fixed seed by name and geometry; shared, never written to): x post-ReLU (about
    half exact zeros) with a different scale at every spatial position, so that a misplaced position changes values;
    W and dy signed, dy scaled per output position likewise; b non-zero."""
    geoms, R, C, co = CASES[name]
    h, w, s = geom
    assert geom in geoms
    g = torch.Generator().manual_seed(9000 + 16 * list(CASES).index(name) + geoms.index(geom))
    oh, ow = same_pad(h, s)[0], same_pad(w, s)[0]
    sx = 0.5 + 1.5 * torch.arange(h * w, dtype=torch.float32).view(1, h, w, 1) / (h * w - 1)
    sy = 1.5 - torch.arange(oh * ow, dtype=torch.float32).view(1, oh, ow, 1) / (oh * ow)
    x = (torch.relu(torch.randn((R, h, w, C), generator=g)) * sx).contiguous()
    W = (torch.randn((co, 9 * C), generator=g) * 0.1).contiguous()
    b = torch.randn((co,), generator=g) * 0.5
    b = torch.where(b.abs() < 0.05, torch.full_like(b, 0.25), b)
    dy = (torch.randn((R, oh, ow, co), generator=g) * sy).contiguous()
    return dict(name=name, geom=geom, h=h, w=w, s=s, oh=oh, ow=ow, R=R, C=C, co=co, x=x, W=W, b=b, dy=dy)


@functools.lru_cache(maxsize=None)
def case_reference(name, geom, bias=True):
    c = make_case(name, geom)
    return reference(c["x"], c["W"], c["b"] if bias else None, c["dy"], c["s"])


# ---------------------------------------------------------------- position classes and the class-packed model

DEFECTS = ["drop_tap", "swap_kykx", "swap_slabs", "scatter_skip", "swap_pad", "w_kwkh"]


class Classes:
    """The layout comment at the top of taps.hip restated: output positions whose valid taps are the same set form a
    class (centre, edges, corners), classes ordered by taps then positions, descending; slots number the output
    positions class by class; position-major rows are slot * R + roi."""

    def __init__(self, h, w, s, swap_pad=False):
        (self.oh, pt, pb), (self.ow, pl, pr) = same_pad(h, s), same_pad(w, s)
        self.h, self.w, self.s = h, w, s
        self.pt, self.pl = (pb, pr) if swap_pad else (pt, pl)

        def axis(n_in, n_out, pad):
            kinds = {}
            for o in range(n_out):
                kinds.setdefault(tuple(k for k in range(3) if 0 <= o * s + k - pad < n_in), []).append(o)
            return list(kinds.items())

        self.classes = sorted(((([ky * 3 + kx for ky in ty for kx in tx]), [(y, x) for y in ys for x in xs])
                               for ty, ys in axis(h, self.oh, self.pt) for tx, xs in axis(w, self.ow, self.pl)),
                              key=lambda c: (-len(c[0]), -len(c[1])))
        self.slots = [p for _, pos in self.classes for p in pos]
        self.slot_base = [sum(len(c[1]) for c in self.classes[:k]) for k in range(len(self.classes))]

    def equal_pair(self):
        """the first two adjacent classes of equal shape"""
        for k in range(len(self.classes) - 1):
            a, b = self.classes[k], self.classes[k + 1]
            if (len(a[0]), len(a[1])) == (len(b[0]), len(b[1])):
                return k, k + 1
        raise AssertionError("no two classes of equal shape")


def class_operands(c, pl=None):
    """Per class of the case, by plain indexing: (patches [npos R, ntaps C], weight [c_o, ntaps C], dy rows
    [npos R, c_o]) -- the operands of the three GEMMs of the class, in the dtype and on the device of c's tensors."""
    pl = pl or Classes(c["h"], c["w"], c["s"])
    x, W9, s = c["x"], c["W"].view(c["co"], 9, c["C"]), c["s"]
    out = []
    for taps, poss in pl.classes:
        a = torch.stack([torch.stack([x[:, oy * s + t // 3 - pl.pt, ox * s + t % 3 - pl.pl] for t in taps], 1)
                         for oy, ox in poss], 0)                                  # [npos, R, ntaps, C]
        g = torch.stack([c["dy"][:, oy, ox] for oy, ox in poss], 0)                # [npos, R, c_o]
        out.append((a.reshape(len(poss) * c["R"], -1).contiguous(), W9[:, taps].reshape(c["co"], -1).contiguous(),
                    g.reshape(len(poss) * c["R"], -1).contiguous()))
    return out


def model_conv(c, defects=(), bias=True):
    """The class-packed algorithm in f32 on the CPU: valid taps packed per class, one mm per class into the class's
    slab of the position-major output, the bias add; backwards one mm per class for the patches' and the packed
    weight's gradients, the adjoint summed per input position in (ky, kx) order from +0, the weight gradient
    scattered by summing the classes that hold a tap in class order.  -> dict(y, dx, dW[, db]) in the reference's
    layouts.  Defects:
      drop_tap      the first tap of the first position of the last (corner) class is neither gathered nor scattered
      swap_kykx     the gather of class 0 reads tap (ky, kx) at offset (kx, ky)
      swap_slabs    two equal-shape classes use each other's output slabs
      scatter_skip  the weight-gradient scatter skips the last class
      swap_pad      `before` and `after` of the padding swapped
      w_kwkh        the weight read as (kw, kh, c)"""
    assert set(defects) <= set(DEFECTS), defects
    h, w, s, R, C, co = (c[k] for k in ("h", "w", "s", "R", "C", "co"))
    pl = Classes(h, w, s, "swap_pad" in defects)
    x, dy = c["x"], c["dy"]
    W9 = c["W"].view(co, 3, 3, C)
    W9 = (W9.transpose(1, 2) if "w_kwkh" in defects else W9).reshape(co, 9, C)
    last = len(pl.classes) - 1
    base = list(pl.slot_base)
    if "swap_slabs" in defects:
        i, j = pl.equal_pair()
        base[i], base[j] = base[j], base[i]
    slot_of = {p: sl for sl, p in enumerate(pl.slots)}

    def src(k, t):
        ky, kx = divmod(t, 3)
        return (kx, ky) if ("swap_kykx" in defects and k == 0) else (ky, kx)

    cols, wp = [], []
    for k, (taps, poss) in enumerate(pl.classes):
        a = torch.zeros((len(poss), R, len(taps), C))
        for i, (oy, ox) in enumerate(poss):
            for tl, t in enumerate(taps):
                if "drop_tap" in defects and (k, i, tl) == (last, 0, 0):
                    continue
                ky, kx = src(k, t)
                a[i, :, tl] = x[:, oy * s + ky - pl.pt, ox * s + kx - pl.pl]
        cols.append(a.view(len(poss) * R, len(taps) * C))
        wp.append(W9[:, taps].reshape(co, len(taps) * C))
    out = torch.zeros((pl.oh * pl.ow, R, co))
    for k, (taps, poss) in enumerate(pl.classes):
        out[base[k]:base[k] + len(poss)] = torch.mm(cols[k], wp[k].t()).view(len(poss), R, co)
    if bias:
        out = out + c["b"]
    y = torch.stack([out[slot_of[(oy, ox)]] for oy in range(pl.oh) for ox in range(pl.ow)], 1).view(R, pl.oh, pl.ow, co)

    dy_pm = torch.stack([dy[:, oy, ox] for oy, ox in pl.slots], 0)                  # [slots, R, c_o]
    dcols, dwp = [], []
    for k, (taps, poss) in enumerate(pl.classes):
        g = dy_pm[base[k]:base[k] + len(poss)].reshape(len(poss) * R, co)
        dcols.append(torch.mm(g, wp[k]).view(len(poss), R, len(taps), C))
        dwp.append(torch.mm(g.t(), cols[k]).view(co, len(taps), C))
    cls_of = {p: (k, i) for k, (_, poss) in enumerate(pl.classes) for i, p in enumerate(poss)}
    dx = torch.zeros((R, h, w, C))
    for iy in range(h):
        for ix in range(w):
            acc = torch.zeros((R, C))
            for ky in range(3):
                for kx in range(3):
                    ny, nx = iy + pl.pt - ky, ix + pl.pl - kx
                    if ny < 0 or ny % s or nx < 0 or nx % s or ny // s >= pl.oh or nx // s >= pl.ow:
                        continue
                    k, i = cls_of[(ny // s, nx // s)]
                    tl = pl.classes[k][0].index(ky * 3 + kx)
                    if "drop_tap" in defects and (k, i, tl) == (last, 0, 0):
                        continue
                    acc = acc + dcols[k][i, :, tl]
            dx[:, iy, ix] = acc
    dW9 = torch.zeros((co, 9, C))
    for t in range(9):
        acc = torch.zeros((co, C))
        for k, (taps, _) in enumerate(pl.classes):
            if t in taps and not ("scatter_skip" in defects and k == last):
                acc = acc + dwp[k][:, taps.index(t)]
        dW9[:, t] = acc
    if "w_kwkh" in defects:
        dW9 = dW9.view(co, 3, 3, C).transpose(1, 2)
    got = dict(y=y, dx=dx, dW=dW9.reshape(co, 9 * C))
    if bias:
        got["db"] = dy_pm.reshape(-1, co).sum(0)
    return got
