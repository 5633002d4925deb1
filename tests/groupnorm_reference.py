"""Shared by test_groupnorm_cpu.py and test_gpu_groupnorm_reference.py: a plain float64 statement of the group norm
of csrc/plumbing/groupnorm.hip (reached through networks/_plumbing.py), elementwise error bounds counted from the
kernels' roundings, inputs that stress them, and a model of the kernels' arithmetic with switches that seed defects.
torch only, any device, no import of wssdl_bus_amd.

WHAT IS COMPUTED.  x is [M, C], M = S * P: S samples of P rows, row (s, p) = s * P + p (sample-major) or p * S + s
(position-major).  The rows of a sample are reshaped to [P, C/G, G] -- channel c belongs to group c % G, the reference
project's interleaved groups -- and one mean and one biased variance are taken per (sample, group) over n = P * C/G
values.  y = act((x - mean) * rstd * gamma[c] + beta[c]), rstd = (var + eps)^-1/2.  With g = dy * gate and
xhat = (x - mean) * rstd:  A = mean(g gamma), B = mean(g gamma xhat) per (sample, group),
dx = rstd (g gamma - A - xhat B), dgamma[c] = sum g xhat, dbeta[c] = sum g over all live samples.  A dead sample
(mask[s] = 0) has y = dx = 0, mean = rstd = 0 and adds nothing to dgamma / dbeta.

THE RULE FOR BOUNDS is the one at the top of rowbn_reference.py: u = 2^-24 per f32 rounding times the magnitude of
what is rounded, carried to the output by whatever multiplies it; e = 2^-53 per f64 operation of the sums; the same
fixed SLACK; the constant in front of u is the count of roundings listed in each bound's docstring; no constant was
chosen by looking at what a GPU produced.
"""
import torch

from rowbn_reference import E, SLACK, U, ratio  # noqa: F401  (ratio: re-exported for the tests)

G = 8
EPS = 1e-5

# ---- the launch geometry of groupnorm.hip (constants of its anonymous namespace; test_groupnorm_cpu.py reads the
# source and holds these to it) ----
GN_SMALL_MAX_FLOATS = 65536
GN_BLOCK_SMALL, GN_BLOCK_LARGE = 512, 256
GN_SMALL_MAX_WG = 1024
GN_CACHE, GN_CACHE_BWD = 16, 8
GN_CHUNK_STEPS, GN_MAX_CHUNKS = 8, 128
GN_MAX_C = 2048


def geometry(S, P, C):
    """What make_plan of groupnorm.hip decides: ('small', workgroups, rows a thread takes, of which in registers
    forward / backward) or ('large', chunks per sample, rows per chunk, row step RS, column passes)."""
    C4 = C // 4
    if P * C <= GN_SMALL_MAX_FLOATS:
        L = min(C4, GN_BLOCK_SMALL)
        RS = GN_BLOCK_SMALL // L
        rows = -(-P // RS)
        return ("small", min(S, GN_SMALL_MAX_WG), rows, min(rows, GN_CACHE), min(rows, GN_CACHE_BWD))
    L = min(C4, GN_BLOCK_LARGE)
    RS = GN_BLOCK_LARGE // L
    want = -(-P // (RS * GN_CHUNK_STEPS))
    nchunk = max(1, min(want, GN_MAX_CHUNKS))
    return ("large", nchunk, -(-P // nchunk), RS, -(-C4 // L))


# (S, P, C) and the path each reaches
TABLE = [
    (1, 1, 8),         # small; one value per group: var = 0 exactly, y = beta
    (3, 49, 64),       # small; L=16, RS=32: 2 rows per thread, all in registers
    (5, 16, 2048),     # small; L=512, RS=1: 16 rows per thread = the forward's register budget, 8 of 16 in the backward
    (2, 49, 1024),     # small; a 200 KB sample: 25 rows per thread, 16 (8) in registers, the rest re-read
    (3001, 16, 64),    # small; more samples than the 1024 workgroups: the sample loop, the carried dgamma partials
    (4, 7, 72),        # small; C/4 = 18 is no power of two: L=18, RS=28, 8 idle threads
    (2, 64, 1024),     # small; exactly GN_SMALL_MAX_FLOATS per sample: just below the switch
    (2, 65, 1024),     # large; just above the switch: RS=1, 9 chunks of 8 rows, the last of 1
    (2, 1031, 64),     # large; RS=16, 9 chunks of 115 rows: no multiple of the row step (one-row tails)
    (1, 16400, 64),    # large; the chunk count hits its cap: 128 chunks of 129 rows, the last of 17
    (2, 40, 2048),     # large; two column passes (C/4 = 512 > 256 threads)
    (1, 300, 264),     # large; C/4 = 66: L=66, RS=3, 58 idle threads
]
MASK_KINDS = ["random", "one_live", "all_dead", "first_last_dead"]
DEFECTS = {
    "contiguous": "contiguous instead of interleaved groups",
    "unbiased": "unbiased variance",
    "eps": "eps 1e-3",
    "layout": "position-major read as sample-major",
    "dead_dgamma": "dead samples counted in dgamma",
    "no_gate": "the ReLU gate missing from the backward",
}


def is_small(S, P, C):
    return geometry(S, P, C)[0] == "small"


def make_case(seed, S, P, C, device):
    """x with per-channel offsets and scales of different size (a group mixes C/G channels: its variance holds their
    spread), a gradient, gamma in [0.5, 1.5], beta in [-0.2, 0.2]"""
    g = torch.Generator().manual_seed(seed * 1000003 + S * 7919 + P * 104729 + C)
    M = S * P
    col_scale = torch.rand(C, generator=g) * 2.0 + 0.25
    col_off = torch.randn(C, generator=g) * 1.5
    x = torch.randn(M, C, generator=g) * col_scale + col_off
    dy = torch.randn(M, C, generator=g)
    w = torch.rand(C, generator=g) + 0.5
    b = torch.rand(C, generator=g) * 0.4 - 0.2
    return {k: v.to(device) for k, v in dict(x=x, dy=dy, w=w, b=b).items()}


def make_mask(kind, S, seed, device):
    g = torch.Generator().manual_seed(seed + 17 * S)
    if kind == "random":
        m = (torch.rand(S, generator=g) < 0.6).float()
    elif kind == "one_live":
        m = torch.zeros(S)
        m[int(torch.randint(S, (1,), generator=g))] = 1.0
    elif kind == "all_dead":
        m = torch.zeros(S)
    elif kind == "first_last_dead":
        m = torch.ones(S)
        m[0] = m[-1] = 0.0
    else:
        raise ValueError(kind)
    return m.to(device)


# ---------------------------------------------------------------- layouts
def to_groups(t, S, P, groups, pos_major=False, contiguous=False):
    """[M, C] -> [S, P, C/G, G] (a view where it can be).  contiguous: the defect, channel c in group c // (C/G)."""
    C = t.shape[1]
    v = t.view(P, S, C).transpose(0, 1) if pos_major else t.view(S, P, C)
    if contiguous:
        return v.reshape(S, P, groups, C // groups).transpose(2, 3)
    return v.reshape(S, P, C // groups, groups)


def from_groups(g, pos_major=False, contiguous=False):
    """to_groups back: [S, P, C/G, G] -> [M, C]"""
    S, P = g.shape[:2]
    v = (g.transpose(2, 3) if contiguous else g).reshape(S, P, -1)
    return (v.transpose(0, 1) if pos_major else v).reshape(S * P, -1)


def _chan(v, groups):
    """a per-channel [C] vector as [1, 1, C/G, G]"""
    return v.view(1, 1, -1, groups)


def _live(mask, S, device):
    return torch.ones(S, dtype=torch.bool, device=device) if mask is None else (mask != 0)


def _eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32).double())


# ---------------------------------------------------------------- f64 references
def forward(x, w, b, eps, groups, P, relu, mask=None, pos_major=False):
    """mean, biased var, rstd [S, G] and y [M, C] in f64 of the f32 inputs; dead samples: zeros.  Also `pre` (y before
    the ReLU) and the magnitudes the bounds need, in the grouped shape [S, 1, 1, G]."""
    M, C = x.shape
    S = M // P
    xg = to_groups(x.double(), S, P, groups, pos_major)
    live = _live(mask, S, x.device)
    lv = live.view(S, 1, 1, 1)
    n = P * (C // groups)
    mean = xg.sum((1, 2), keepdim=True) / n
    var = ((xg - mean) ** 2).sum((1, 2), keepdim=True) / n
    absmean = xg.abs().sum((1, 2), keepdim=True) / n
    sqmean = (xg * xg).sum((1, 2), keepdim=True) / n
    eps = _eps32(eps)
    rstd = (var + eps) ** -0.5
    wg, bg = _chan(w.double(), groups), _chan(b.double(), groups)
    pre = (xg - mean) * rstd * wg + bg
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    pre = torch.where(lv, pre, zero)
    mean, var, rstd = (torch.where(lv, t, zero) for t in (mean, var, rstd))
    y = pre.clamp_min(0.0) if relu else pre
    return dict(mean=mean.view(S, groups), var=var.view(S, groups), rstd=rstd.view(S, groups),
                y=from_groups(y, pos_major), pre=from_groups(pre, pos_major), live=live, n=n, eps=eps,
                mean_g=mean, var_g=var, absmean=absmean, sqmean=sqmean, xg=xg, wg=wg, bg=bg, S=S, P=P,
                pos_major=pos_major)


def backward(x, dy, w, mean, rstd, groups, P, gate=None, mask=None, pos_major=False):
    """dx [M, C], dgamma, dbeta [C] in f64.  mean and rstd [S, G] are inputs of this entry point (the kernel's own f32
    values); gate (bool [M, C], or None without ReLU) is the ReLU mask, passed in as data."""
    M, C = x.shape
    S = M // P
    live = _live(mask, S, x.device)
    lv = live.view(S, 1, 1, 1)
    xg = to_groups(x.double(), S, P, groups, pos_major)
    g = dy.double() if gate is None else torch.where(gate, dy.double(), torch.zeros_like(dy, dtype=torch.float64))
    gg = to_groups(g, S, P, groups, pos_major) * lv
    mu, rs = mean.double().view(S, 1, 1, groups), rstd.double().view(S, 1, 1, groups)
    wg = _chan(w.double(), groups)
    n = P * (C // groups)
    xhat = (xg - mu) * rs
    ggw = gg * wg
    A = ggw.sum((1, 2), keepdim=True) / n
    B = (ggw * xhat).sum((1, 2), keepdim=True) / n
    dx = rs * (ggw - A - xhat * B) * lv
    gx = gg * xhat
    return dict(dx=from_groups(dx, pos_major), dgamma=gx.sum((0, 1)).reshape(C), dbeta=gg.sum((0, 1)).reshape(C),
                A=A, B=B, xhat=xhat, ggw=ggw, rs=rs, n=n, live=live, S=S, P=P, pos_major=pos_major,
                mA=ggw.abs().sum((1, 2), keepdim=True) / n, mB=(ggw * xhat).abs().sum((1, 2), keepdim=True) / n,
                sum_abs_g=gg.abs().sum((0, 1)).reshape(C), sum_abs_gx=gx.abs().sum((0, 1)).reshape(C))


# ---------------------------------------------------------------- bounds
def _f_mean(f):
    # f64: the sum of n terms and the product with 1/n, each e relative to at most mean|x|; 1/n itself (1 e)
    return (f["n"] + 2) * E * f["absmean"]


def _f_var(f):
    # f64, v = q/n - mu*mu: as rowbn_reference._f_var with n for M (and 1/n's own rounding)
    return (3 * f["n"] + 6) * E * f["sqmean"]


def _rs_hi(f):
    return ((f["var_g"] - _f_var(f)).clamp_min(0.0) + f["eps"]) ** -0.5


def _f_rstd(f):
    return 0.5 * _f_var(f) * _rs_hi(f) ** 3


def _dead_zero(t, f):
    return torch.where(f["live"].view(-1, 1, 1, 1), t, torch.zeros((), dtype=t.dtype, device=t.device))


def bound_mean(f):
    """[S, G].  mean = (float)(s / n): 1 rounding, u|mean|; the f64 sum and division.  Dead samples: exactly 0."""
    return _dead_zero(SLACK * (U * f["mean_g"].abs() + _f_mean(f)), f).view(f["S"], -1)


def bound_rstd(f):
    """[S, G].  rstd = (float)(1 / sqrt(v + eps)) from the f64 v: 1 rounding, u rstd; the f64 error of v times
    rstd^3 / 2 (both taken at the smallest v that error allows); 3 e rstd for the sum, root and quotient."""
    return _dead_zero(SLACK * ((U + 3 * E) * _rs_hi(f) + _f_rstd(f)), f).view(f["S"], -1)


def bound_y(f):
    """[M, C].  With s = |gamma| rstd: scale = rstd_f32 * gamma carries 2 roundings (2u|x s| and 2u|mean s|); mean ->
    f32 (u|mean s|); shift = fma(-mean, scale, beta), 1 rounding (u|mean s| + u|beta|); y = fma(x, scale, shift), 1
    rounding (u|x s| + u|mean s| + u|beta|):
        3u|x s| + 5u|mean s| + 2u|beta|
    plus the f64 parts (rstd's times (|x| + |mean|)|gamma|, mean's times s).  The ReLU does not increase a
    difference; dead samples are exactly 0."""
    wa = f["wg"].abs()
    s = wa * _rs_hi(f)
    ms = f["mean_g"].abs() * s
    bd = (f["xg"].abs() * (3 * U * s + wa * _f_rstd(f)) + 5 * U * ms + 2 * U * f["bg"].abs() + s * _f_mean(f)
          + f["mean_g"].abs() * wa * _f_rstd(f))
    return from_groups(_dead_zero(SLACK * bd, f), f["pos_major"])


def bound_dbeta(r):
    """[C].  dbeta = (float)sum g: 1 rounding, u|dbeta|; the f64 sums (sample, workgroup, slice), M e sum|g|."""
    F = (r["S"] * r["P"] + 2) * E * r["sum_abs_g"]
    return SLACK * (U * (r["dbeta"].abs() + F) + F)


def bound_dgamma(r):
    """[C].  dgamma = (float)sum g * xhat_f32, xhat_f32 = fl(fl(x - mean) * rstd): 2 roundings per term, 2u sum|g xhat|;
    the result's rounding, u|dgamma|; the f64 sums, M e sum|g xhat| (the products are exact in f64)."""
    F = 2 * U * r["sum_abs_gx"] + (r["S"] * r["P"] + 2) * E * r["sum_abs_gx"]
    return SLACK * (U * (r["dgamma"].abs() + F) + F)


def bound_dx(r):
    """[M, C].  With a = |g gamma|, xb = |xhat B|, mB = mean|g gamma xhat|:
      A -> f32: u|A|;  B -> f32: u|B|, and its terms carry xhat_f32's 2 roundings: 2u mB
      t1 = fma(g, gamma, -A): A's error + u(a + |A|)
      t2 = fma(-xhat_f32, B, t1): t1's error + |xhat| B's error + 2u xb (xhat_f32) + u(a + |A| + xb)
      dx = rstd * t2: rstd times t2's error + u rstd (a + |A| + xb)
    in all  rstd u (3a + 4|A| + 5xb + 2|xhat| mB), plus the f64 parts of A and B ((n + 2) e of their mean
    magnitudes, B's times |xhat|).  Dead samples are exactly 0."""
    a, A, xh = r["ggw"].abs(), r["A"].abs(), r["xhat"].abs()
    xb = xh * r["B"].abs()
    fA, fB = (r["n"] + 2) * E * r["mA"], (r["n"] + 2) * E * r["mB"]
    bd = r["rs"].abs() * (U * (3 * a + 4 * A + 5 * xb + 2 * xh * r["mB"]) + fA + xh * fB)
    bd = torch.where(r["live"].view(-1, 1, 1, 1), SLACK * bd, torch.zeros((), dtype=bd.dtype, device=bd.device))
    return from_groups(bd, r["pos_major"])


def forward_ratios(x, w, b, eps, groups, P, relu, got, mask=None, pos_major=False):
    """worst |error| / bound of y, mean, rstd in `got` against forward(); returns (ratios, the reference, y's bound)"""
    f = forward(x, w, b, eps, groups, P, relu, mask, pos_major)
    by = bound_y(f)
    r = dict(y=ratio(got["y"], f["y"], by), mean=ratio(got["mean"], f["mean"], bound_mean(f)),
             rstd=ratio(got["rstd"], f["rstd"], bound_rstd(f)))
    return r, f, by


def backward_ratios(x, dy, w, mean, rstd, groups, P, gate, got, mask=None, pos_major=False):
    b = backward(x, dy, w, mean, rstd, groups, P, gate, mask, pos_major)
    return dict(dx=ratio(got["dx"], b["dx"], bound_dx(b)), dgamma=ratio(got["dgamma"], b["dgamma"], bound_dgamma(b)),
                dbeta=ratio(got["dbeta"], b["dbeta"], bound_dbeta(b))), b


def check_ratios(case, ratios, log=None):
    """prints and asserts every worst |error| / bound of one case; log keeps the worst per output"""
    for name, r in ratios.items():
        print("gn-ratio %s %.4g %s" % (name, r, case))
        if log is not None:
            log[name] = max(log.get(name, 0.0), r)
    for name, r in ratios.items():
        assert r <= 1.0, "%s: %s misses its bound, worst |error| / bound = %.4g" % (case, name, r)


def check_gate(case, y, f, by):
    """the kernel's ReLU gate (y > 0) against f64 wherever |pre64| exceeds y's bound"""
    sure = f["pre"].abs() > by
    bad = sure & ((y > 0) != (f["pre"] > 0))
    assert not bool(bad.any()), "%s: %d gates differ from f64 outside the bound" % (case, int(bad.sum()))


# ---------------------------------------------------------------- a model of the kernels' arithmetic
def _f32(t):
    return t.float()


def _fma(a, b, c):
    """fl32(a * b + c) of f32 tensors: the product of two f32 is exact in f64, the sum is rounded there (e) and once
    more to f32"""
    return (a.double() * b.double() + c.double()).float()


def model_forward(x, w, b, eps, groups, P, relu, mask=None, pos_major=False, defect=None):
    """(y, mean [S, G], rstd [S, G]) as groupnorm.hip computes them: f64 sums, mean / rstd rounded to f32 once,
    scale = rstd * gamma, shift = fma(-mean, scale, beta), y = fma(x, scale, shift) in f32."""
    assert defect is None or defect in DEFECTS, defect
    M, C = x.shape
    S = M // P
    contiguous = defect == "contiguous"
    read_pm = pos_major and defect != "layout"
    xg = to_groups(x, S, P, groups, read_pm, contiguous)
    n = P * (C // groups)
    s = xg.double().sum((1, 2), keepdim=True)
    q = (xg.double() ** 2).sum((1, 2), keepdim=True)
    mu = s / n
    var = (q / n - mu * mu).clamp_min(0.0)
    if defect == "unbiased":
        var = var * n / max(n - 1, 1)
    e = 1e-3 if defect == "eps" else eps
    mean, rstd = _f32(mu), _f32((var + _eps32(e)) ** -0.5)
    wg = from_groups_inv(w, groups, contiguous)
    bg = from_groups_inv(b, groups, contiguous)
    sc = rstd * wg
    sh = _fma(-mean, sc, bg.expand_as(sc))
    y = _fma(xg, sc, sh)
    if relu:
        y = torch.where(y > 0, y, torch.zeros_like(y))
    live = _live(mask, S, x.device)
    lv = live.view(S, 1, 1, 1)
    y = torch.where(lv, y, torch.zeros_like(y))
    mean = torch.where(lv, mean, torch.zeros_like(mean)).view(S, groups)
    rstd = torch.where(lv, rstd, torch.zeros_like(rstd)).view(S, groups)
    return from_groups(y, read_pm, contiguous), mean, rstd


def from_groups_inv(v, groups, contiguous=False):
    """a per-channel [C] vector in the grouped shape [1, 1, C/G, G] of to_groups"""
    return to_groups(v.view(1, -1), 1, 1, groups, False, contiguous)


def model_backward(x, dy, w, b, mean, rstd, groups, P, relu, mask=None, pos_major=False, defect=None):
    """(dx, dgamma, dbeta) as groupnorm.hip computes them from the forward's f32 mean / rstd"""
    assert defect is None or defect in DEFECTS, defect
    M, C = x.shape
    S = M // P
    contiguous = defect == "contiguous"
    read_pm = pos_major and defect != "layout"
    xg = to_groups(x, S, P, groups, read_pm, contiguous)
    dg = to_groups(dy, S, P, groups, read_pm, contiguous)
    mu, rs = mean.view(S, 1, 1, groups), rstd.view(S, 1, 1, groups)
    wg, bg = from_groups_inv(w, groups, contiguous), from_groups_inv(b, groups, contiguous)
    sc = rs * wg
    sh = _fma(-mu, sc, bg.expand_as(sc))
    g = dg
    if relu and defect != "no_gate":
        g = torch.where(_fma(xg, sc, sh) > 0, dg, torch.zeros_like(dg))
    live = _live(mask, S, x.device)
    lv = live.view(S, 1, 1, 1)
    xhat = (xg - mu) * rs                                  # f32: two roundings
    n = P * (C // groups)
    gw = g.double() * wg.double()
    A = _f32((gw * lv).sum((1, 2), keepdim=True) / n)
    B = _f32((gw * xhat.double() * lv).sum((1, 2), keepdim=True) / n)
    t1 = _fma(g, wg.expand_as(g), -A.expand_as(g))
    dx = rs * _fma(-xhat, B.expand_as(xhat), t1)
    dx = torch.where(lv, dx, torch.zeros_like(dx))
    keep = torch.ones_like(lv) if defect == "dead_dgamma" else lv
    dgamma = _f32((g.double() * xhat.double() * keep).sum((0, 1)))
    dbeta = _f32((g.double() * lv).sum((0, 1)))
    back = (lambda t: t.transpose(0, 1).reshape(C)) if contiguous else (lambda t: t.reshape(C))
    return from_groups(dx, read_pm, contiguous), back(dgamma), back(dbeta)
