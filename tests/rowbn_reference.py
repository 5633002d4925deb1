"""Shared by test_rowbn_reference_cpu.py and test_gpu_rowbn_reference.py: a plain float64 statement of every entry
point of the row batch norm (csrc/plumbing/rowbn.hip, reached through networks/_plumbing.py), elementwise error
bounds counted from the kernels' roundings, inputs that stress them, and a model of the kernels' arithmetic with
switches that seed defects.  torch only, any device, no import of _plumbing.

THE RULE FOR BOUNDS.  u = 2^-24 is the unit roundoff of f32 (round to nearest: |fl(z) - z| <= u|z|), e = 2^-53 that
of f64.  Every f32 rounding on an output's path costs u times the magnitude of the term it rounds; a rounding of an
intermediate reaches the output multiplied by whatever the intermediate is multiplied by.  The column sums are f64:
a sum of M terms costs at most M * e * (sum of the terms' magnitudes).  Each bound's docstring lists the roundings
it counts; the constant in front of u is that count (the rule allows up to twice it; none is doubled here).  SLACK
= 1 + 2^-20 multiplies every bound: it covers the products of two error terms (second order in u) and the rounding
of the f64 reference itself, and is fixed in advance.  No constant was chosen by looking at what a GPU produced.
"""
import torch

U = 2.0 ** -24
E = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20
BLOCK = 256
MAX_PARTIAL_BLOCKS = 1024

# [M, C] and what each reaches (partial_blocks / shape_ok / apply_grid of rowbn.hip)
TABLE = [
    (1, 4),          # L=1, RS=256, one row: var = 0 exactly
    (259, 16),       # RS=64, fewer rows than two row steps for most phases
    (7, 256),        # RS=4, one partial slab
    (1041, 512),     # RS=2, 33 blocks, last slab odd (tail row)
    (4099, 1024),    # RS=1, 257 blocks (> 64 finish groups), last slab of 3 rows
    (16400, 1024),   # block count capped at 1024, rpb=17 (tail row in every slab), trailing empty blocks
    (1031, 2048),    # two column passes
    (67, 4096),      # four column passes
    (33000, 2048),   # second trip of the apply kernels' grid-stride loop, capped blocks
]
MASK_KINDS = ["random", "one_live", "all_dead", "dead_run"]
MASK_SPLITS = [(1, 16), (37, 49), (1500, 16), (2053, 1)]      # (n_rois, per); n_rois > 1024: live_rows loops


def geometry(M, C):
    """(L, RS, nb, rpb): Slab's thread mapping and partial_blocks' slabs for an [M, C] call."""
    C4 = C // 4
    L = min(C4, BLOCK)
    RS = BLOCK // L
    want = max((M + RS * 16 - 1) // (RS * 16), 1)
    nb = min(want, MAX_PARTIAL_BLOCKS)
    return L, RS, nb, (M + nb - 1) // nb


def row_live(mask, M, per=1, pos_major=False, roi_major_bug=False):
    """bool [M]: the live rows under mask [n_rois] (row r belongs to RoI r // per, or r % n_rois when
    position-major); None without a mask."""
    if mask is None:
        return None
    n_rois = mask.numel()
    r = torch.arange(M, device=mask.device)
    roi = r % n_rois if (pos_major and not roi_major_bug) else r // per
    return mask[roi] != 0


def _count(mask, M, per):
    return float(M) if mask is None else max(float(per * int((mask != 0).sum())), 1.0)


def _eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32).double())       # the entry points take a float


# ---------------------------------------------------------------- f64 references

def forward(x, w, b, eps, relu, mask=None, per=1, pos_major=False):
    """mean, biased var, rstd, scale, shift, y, count of the layer over the live rows, in f64 of the f32 inputs.
    y is zero on dead rows; count = per * live RoIs, at least 1; all dead: mean = var = 0.  Also `pre` (y before
    the ReLU), `live`, and the magnitudes the bounds need."""
    x, w, b = x.double(), w.double(), b.double()
    M, C = x.shape
    eps = _eps32(eps)
    live = row_live(mask, M, per, pos_major)
    n = _count(mask, M, per)
    xl = x if live is None else x[live]
    if xl.shape[0] == 0:
        mean = var = absmean = sqmean = torch.zeros((C,), dtype=torch.float64, device=x.device)
    else:
        mean = xl.sum(0) / n
        var = ((xl - mean) ** 2).sum(0) / n
        absmean = xl.abs().sum(0) / n
        sqmean = (xl * xl).sum(0) / n
    del xl
    rstd = (var + eps) ** -0.5
    scale = w * rstd
    shift = b - mean * scale
    pre = x * scale + shift
    if live is not None:
        pre[~live] = 0.0
    y = pre.clamp_min(0.0) if relu else pre
    return dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, y=y, pre=pre, count=n, live=live, M=M,
                eps=eps, absmean=absmean, sqmean=sqmean, w=w, b=b)


def backward(x, dy, w, mean, rstd, gate=None, mask=None, per=1, pos_major=False, g_err=None):
    """dx, dweight, dbias of the layer in f64.  mean and rstd are inputs of this entry point (the kernel's own f32
    values); gate (bool [M, C], or None without ReLU) is the ReLU mask, passed in as data.  Dead rows take dx = 0
    and add nothing to the sums.  g_err: elementwise bound on an error the gradient already carries (the entry
    gradient's one rounding), kept for the bounds."""
    x, dy, w, mean, rstd = x.double(), dy.double(), w.double(), mean.double(), rstd.double()
    M, C = x.shape
    live = row_live(mask, M, per, pos_major)
    n = _count(mask, M, per)
    g = dy if gate is None else torch.where(gate, dy, torch.zeros_like(dy))
    if live is not None:
        g = g * live.unsqueeze(1)
    xc = x - mean
    sg = g.sum(0)
    dw = (g * xc).sum(0) * rstd
    a = w * rstd
    k1 = a * rstd * dw / n
    k0 = a * sg / n - k1 * mean
    dx = a * (g - sg / n - xc * (rstd * dw / n))
    if live is not None:
        dx[~live] = 0.0
    r = dict(dx=dx, dweight=dw, dbias=sg, a=a, k0=k0, k1=k1, g=g, n=n, M=M, live=live, mean=mean, rstd=rstd,
             sum_abs_g=g.abs().sum(0), sum_abs_gx=(g * x).abs().sum(0))
    if g_err is not None:
        ge = g_err.double() * (g != 0)
        r["g_db"] = ge.sum(0)
        r["g_dw"] = rstd * (ge * xc.abs()).sum(0)
        r["g_dx"] = a.abs() * (ge + r["g_db"] / n + xc.abs() * rstd * r["g_dw"] / n)
    return r


def entry_total(dy, dys, possel, n_rois):
    """The gradient rowbn_backward_entry forms in registers, exactly: dy[r] + dys[possel[p] * R + roi] where
    possel[p] >= 0, r = roi * per + p."""
    per, C = possel.numel(), dy.shape[1]
    t = dy.double().view(n_rois, per, C).clone()
    sel = possel >= 0
    t[:, sel] += dys.double().view(-1, n_rois, C)[possel[sel].long()].transpose(0, 1)
    return t.view(-1, C)


def join_forward(x3, bn3, other, bns, bnn, mask=None, out_kernel=None):
    """out = bn3(x3) + (bns(other) if bns else other) over position-major rows, each bn a (weight, bias, eps)
    triple; on a dead row out is `other` in the identity form and 0 in the dual form.  Returns the three layers'
    forward() results (`f3`, `fs` or None, `fn`), `out` and its two addends `t`, `o`.  The next norm (ReLU on) is
    taken over out_kernel when given (the staged comparison: the kernel's own f32 out), else over out."""
    M = x3.shape[0]
    per = M // mask.numel() if mask is not None else 1
    f3 = forward(x3, bn3[0], bn3[1], bn3[2], False, mask, per, True)
    fs = forward(other, bns[0], bns[1], bns[2], False, mask, per, True) if bns is not None else None
    t, o = f3["y"], (fs["y"] if fs is not None else other.double())
    out = t + o
    fn = forward(out if out_kernel is None else out_kernel, bnn[0], bnn[1], bnn[2], True, mask, per, True)
    return dict(f3=f3, fs=fs, fn=fn, out=out, t=t, o=o)


def _mean_rstd(stats):
    """(mean, rstd) of a statistics block: the binding's [5, C] tensor or a dict by name"""
    return (stats["mean"], stats["rstd"]) if isinstance(stats, dict) else (stats[0], stats[2])


def join_backward(out, dy, dres, x3, xs, wn, stats_n, w3, stats3, ws, stats_s, gate, mask=None, g_kernel=None):
    """g = dx of the norm after the join (ReLU gate given as data) + dres; on a dead row g is dres, or 0 without
    it.  Then bn3's (and, with xs, the shortcut norm's) backward over g -- over g_kernel when given (the staged
    comparison).  stats_* are the kernel's statistics ([5, C] blocks: mean, var, rstd, scale, shift; or dicts by name).  Returns `bn`, `g`,
    `dxn` (g before dres is added), `b3`, `bs` or None."""
    M = out.shape[0]
    per = M // mask.numel() if mask is not None else 1
    (mn, rn), (m3, r3) = _mean_rstd(stats_n), _mean_rstd(stats3)
    bn = backward(out, dy, wn, mn, rn, gate, mask, per, True)
    g = bn["dx"] + dres.double() if dres is not None else bn["dx"]
    gu = g if g_kernel is None else g_kernel
    b3 = backward(x3, gu, w3, m3, r3, None, mask, per, True)
    bs = backward(xs, gu, ws, *_mean_rstd(stats_s), None, mask, per, True) if xs is not None else None
    return dict(bn=bn, g=g, dxn=bn["dx"], b3=b3, bs=bs)


def running(rm0, rv0, mean, var, n, momentum):
    """The updated buffers: the once-rounded f64 formula of rowbn.hip's running_update, from the f32 mean / var the
    kernel wrote and the row count n."""
    mom = float(torch.tensor(momentum, dtype=torch.float32).double())
    rm0, rv0, mean, var = (t.detach().double() for t in (rm0, rv0, mean, var))
    unbias = n / max(n - 1.0, 1.0)
    return (rm0 + mom * (mean - rm0)).float(), (rv0 + mom * (var * unbias - rv0)).float()


# ---------------------------------------------------------------- bounds

def _f_mean(f):
    # f64: the sum of M terms ((M-1) additions) and the division, each e relative to at most mean|x|
    return f["M"] * E * f["absmean"]


def _f_var(f):
    # f64, v = q/n - mu*mu: q's sum and division (M e mean(x^2)); mu's error M e mean|x| doubled by the square and
    # multiplied by |mu| (<= 2 M e mean(x^2), as |mu| mean|x| <= mean(x^2)); the roundings of mu*mu, of the
    # difference and of the clamp-free result (3 e mean(x^2)).  The clamp at 0 only moves v towards var64 >= 0.
    return (3 * f["M"] + 3) * E * f["sqmean"]


def _rs_hi(f):
    # rstd is decreasing and convex in v: the largest rstd (and slope) within the f64 error of v
    return ((f["var"] - _f_var(f)).clamp_min(0.0) + f["eps"]) ** -0.5


def _f_rstd(f):
    # |d rstd / d v| = rstd^3 / 2, taken at the smallest v the f64 error allows; rstd is computed from the f64 v
    return 0.5 * _f_var(f) * _rs_hi(f) ** 3


def bound_mean(f):
    """[C].  mean = (float)(s / n): 1 rounding, u|mean|; the f64 sum and division, M e mean|x|."""
    return SLACK * (U * f["mean"].abs() + _f_mean(f))


def bound_var(f):
    """[C].  var = (float)max(q/n - mu^2, 0): 1 rounding, u var (of the f64 value, itself within F of var64); the f64
    part F = (3M + 3) e mean(x^2) (see _f_var: cancellation of q/n against mu^2 is paid here)."""
    F = _f_var(f)
    return SLACK * (U * (f["var"] + F) + F)


def bound_rstd(f):
    """[C].  rstd = (float)(1 / sqrt(v + eps)) from the f64 v: 1 rounding, u rstd; the f64 error of v times
    rstd^3 / 2 (rstd and slope taken at the smallest v that error allows)."""
    return SLACK * (U * _rs_hi(f) + _f_rstd(f))


def bound_scale(f):
    """[C].  scale = rstd_f32 * w: 2 roundings (rstd -> f32, the product), 2u|w rstd|; plus |w| times rstd's f64 part."""
    w = f["w"].abs()
    return SLACK * (2 * U * w * _rs_hi(f) + w * _f_rstd(f))


def bound_shift(f):
    """[C].  shift = b - mean_f32 * scale, with s = |w| rstd: mean -> f32 (u|mean s|), scale's 2 roundings
    (2u|mean s|), the product (u|mean s|), the difference (u|b| + u|mean s|; one rounding less if the compiler
    fuses the two): 5u|mean s| + u|b|; plus the f64 parts of mean (times s) and rstd (times |mean w|)."""
    s = f["w"].abs() * _rs_hi(f)
    ms = f["mean"].abs() * s
    return SLACK * (5 * U * ms + U * f["b"].abs() + s * _f_mean(f) + f["mean"].abs() * f["w"].abs() * _f_rstd(f))


def bound_y(x, f):
    """[M, C].  y = act(fma(x, scale, shift)), s = |w| rstd.  x*scale carries scale's 2 roundings, shift the 5u|mean s|
    + u|b| of bound_shift, and the fma rounds once more, u(|x s| + |mean s| + |b|):
        3u|x s| + 6u|mean s| + 2u|b|
    plus the f64 parts (rstd's times (|x| + |mean|)|w|, mean's times s).  The ReLU does not increase a difference;
    dead rows are exactly 0 (bound 0)."""
    s = f["w"].abs() * _rs_hi(f)
    ms = f["mean"].abs() * s
    col = 6 * U * ms + 2 * U * f["b"].abs() + s * _f_mean(f) + f["mean"].abs() * f["w"].abs() * _f_rstd(f)
    bd = SLACK * (x.double().abs() * (3 * U * s + f["w"].abs() * _f_rstd(f)) + col)
    if f["live"] is not None:
        bd[~f["live"]] = 0.0
    return bd


def bound_apply(ref):
    """[M, C].  rowbn_apply: y = act(fma(x, scale, shift)) with given f32 scale / shift: 1 rounding, u|y|."""
    return SLACK * U * ref.abs()


def bound_dbias(r):
    """[C].  dbias = (float)sum g: 1 rounding, u|dbias|; the f64 sum, M e sum|g|; an error the gradient already
    carries sums up (g_db)."""
    F = r["M"] * E * r["sum_abs_g"] + r.get("g_db", 0.0)
    return SLACK * (U * (r["dbias"].abs() + F) + F)


def _f_dw(r):
    # f64, (sgx - mu*sg) * rs: sgx's sum (M e sum|g x|), sg's sum times |mu| (M e |mu| sum|g|), the roundings of the
    # product mu*sg, of the difference and of the product with rs (together <= 4 e (sum|g x| + |mu| sum|g|)).
    # The cancellation of sgx against mean * sum g is paid here: the term |mean sum g| rstd of the issue.
    return (r["M"] + 4) * E * r["rstd"] * (r["sum_abs_gx"] + r["mean"].abs() * r["sum_abs_g"])


def bound_dweight(r):
    """[C].  dweight = (float)((sgx - mean*sg) * rstd): 1 rounding, u|dweight|; the f64 part (M + 4) e rstd
    (sum|g x| + |mean| sum|g|); an error the gradient already carries (g_dw)."""
    F = _f_dw(r) + r.get("g_dw", 0.0)
    return SLACK * (U * (r["dweight"].abs() + F) + F)


def bound_dx(x, r):
    """[M, C].  dx = fma(-k1, x, fma(a, g, -k0)) with a, k0, k1 computed in f64 and rounded to f32: a -> f32 (u|a g|),
    k0 -> f32 (u|k0|), the inner fma (u|a g| + u|k0|), k1 -> f32 (u|k1 x|), the outer fma (u|a g| + u|k0| + u|k1 x|):
        3u|a g| + 3u|k0| + 2u|k1 x|
    plus the f64 parts of k1 (that of dweight times |a rstd| / n, and 4 e |k1| for its products) and of k0 (sum g's
    times |a| / n, k1's times |mean|, 4 e of its two terms), and an error the gradient already carries (g_dx).
    Dead rows are exactly 0 (bound 0)."""
    n, ax = r["n"], x.double().abs()
    d_k1 = (r["a"] * r["rstd"]).abs() / n * _f_dw(r) + 4 * E * r["k1"].abs()
    d_k0 = (r["a"].abs() / n * r["M"] * E * r["sum_abs_g"] + r["mean"].abs() * d_k1
            + 4 * E * ((r["a"] * r["dbias"]).abs() / n + (r["k1"] * r["mean"]).abs()))
    bd = (3 * U * (r["a"] * r["g"]).abs() + 3 * U * r["k0"].abs() + d_k0 + ax * (2 * U * r["k1"].abs() + d_k1))
    if "g_dx" in r:
        bd = bd + r["g_dx"]
    bd = SLACK * bd
    if r["live"] is not None:
        bd[~r["live"]] = 0.0
    return bd


def bound_out(x3, other, j):
    """[M, C].  out = y3 + (ys or other): the bounds of the addends that are norms (bound_y; the identity shortcut is
    exact) and the sum's 1 rounding, u(|y3| + |o|).  A dead row is a copy of `other` or 0 (bound 0)."""
    bd = bound_y(x3, j["f3"]) + SLACK * U * (j["t"].abs() + j["o"].abs())
    if j["fs"] is not None:
        bd = bd + bound_y(other, j["fs"])
    live = j["f3"]["live"]
    if live is not None:
        bd[~live] = 0.0
    return bd


def bound_g(out, dres, jb):
    """[M, C].  g = dx_n + dres: bound_dx of the norm after the join and, with dres, the sum's 1 rounding,
    u(|dx_n| + |dres|).  A dead row is a copy of dres or 0 (bound 0)."""
    bd = bound_dx(out, jb["bn"])
    if dres is not None:
        extra = SLACK * U * (jb["dxn"].abs() + dres.double().abs())
        live = jb["bn"]["live"]
        if live is not None:
            extra[~live] = 0.0
        bd = bd + extra
    return bd


def ratio(got, ref, bound):
    """worst |got - ref| / bound over all elements (0 where the error is 0, inf where a bound of 0 is missed)"""
    err = (got.double() - ref.double()).abs()
    if not torch.is_tensor(bound):
        bound = torch.full_like(err, float(bound))
    r = err / bound.clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where((err > 0) & (bound <= 0), torch.full_like(r, float("inf")), r)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def check(case, name, got, ref, bound, log=None):
    return check_ratios(case, {name: ratio(got, ref, bound)}, log)


def check_ratios(case, ratios, log=None):
    """prints and asserts every worst |error| / bound of one case; log keeps the worst per output"""
    for name, r in ratios.items():
        print("rowbn-ratio %s %.4g %s" % (name, r, case))
        if log is not None:
            log[name] = max(log.get(name, 0.0), r)
    for name, r in ratios.items():
        assert r <= 1.0, "%s: %s misses its bound, worst |error| / bound = %.4g" % (case, name, r)


def stat_ratios(got, f, prefix=""):
    """worst |error| / bound of the five statistic rows (got: mean, var, rstd, scale, shift) against forward()'s f"""
    bounds = dict(mean=bound_mean, var=bound_var, rstd=bound_rstd, scale=bound_scale, shift=bound_shift)
    return {prefix + k: ratio(got[k], f[k], fn(f)) for k, fn in bounds.items()}


def stats_dict(stats, y=None):
    """the [5, C] block the binding returns, by name"""
    d = dict(mean=stats[0], var=stats[1], rstd=stats[2], scale=stats[3], shift=stats[4])
    if y is not None:
        d["y"] = y
    return d


def forward_ratios(x, w, b, eps, relu, got, mask=None, per=1, pos_major=False):
    """worst |error| / bound of every forward output in `got` (mean, var, rstd, scale, shift, y as tensors) against
    forward(); returns (ratios, the reference, y's bound)."""
    f = forward(x, w, b, eps, relu, mask, per, pos_major)
    r = stat_ratios(got, f)
    by = bound_y(x, f)
    r["y"] = ratio(got["y"], f["y"], by)
    return r, f, by


def backward_ratios(x, dy, w, mean, rstd, gate, got, mask=None, per=1, pos_major=False, g_err=None, prefix=""):
    """the same for dx, dweight, dbias against backward()"""
    b = backward(x, dy, w, mean, rstd, gate, mask, per, pos_major, g_err)
    r = {prefix + "dx": ratio(got["dx"], b["dx"], bound_dx(x, b)),
         prefix + "dweight": ratio(got["dweight"], b["dweight"], bound_dweight(b)),
         prefix + "dbias": ratio(got["dbias"], b["dbias"], bound_dbias(b))}
    return r, b


def entry_ratios(x, dy, dys, possel, n_rois, w, mean, rstd, gate, got, mask=None):
    """rowbn_backward_entry's dx, dweight, dbias against backward() of entry_total().  The kernel rounds the summed
    gradient to f32 once: u|dy + dys| per element on top of the plain backward's bounds (g_err)."""
    total = entry_total(dy, dys, possel, n_rois)
    r, _ = backward_ratios(x, total, w, mean, rstd, gate, got, mask, possel.numel(), False,
                           g_err=U * total.abs(), prefix="entry_")
    return r


def join_forward_ratios(x3, bn3, other, bns, bnn, mask, out, y, s3, ss, sn):
    """The forward join judged in stages (s3 / ss / sn: dicts of the three norms' statistics, ss None in the identity
    form).  Stage 1: the two norms' statistics and out against f64 of (x3, other).  Stage 2: the next norm's
    statistics and y against f64 of the kernel's own out.  Returns (ratios, the next norm's reference, y's bound)."""
    j = join_forward(x3, bn3, other, bns, bnn, mask, out_kernel=out)
    r = stat_ratios(s3, j["f3"], "join3_")
    if bns is not None:
        r.update(stat_ratios(ss, j["fs"], "joins_"))
    r["join_out"] = ratio(out, j["out"], bound_out(x3, other, j))
    r.update(stat_ratios(sn, j["fn"], "joinn_"))
    byn = bound_y(out, j["fn"])
    r["joinn_y"] = ratio(y, j["fn"]["y"], byn)
    return r, j["fn"], byn


def join_backward_ratios(out, dy, dres, x3, xs, wn, sn, w3, s3, ws, ss, gate, mask, g, dx3, dxs, dwbn, dwb3, dwbs):
    """The backward join judged in stages (dwb*: (dweight, dbias) pairs).  Stage 3: g and the next norm's parameter
    gradients against f64 of (out, dy, dres, stats_n).  Stage 4: the input and parameter gradients of bn3 (and of the
    shortcut's norm) against f64 of the kernel's own g."""
    jb = join_backward(out, dy, dres, x3, xs, wn, sn, w3, s3, ws, ss, gate, mask, g_kernel=g)
    r = {"join_g": ratio(g, jb["g"], bound_g(out, dres, jb)),
         "joinn_dweight": ratio(dwbn[0], jb["bn"]["dweight"], bound_dweight(jb["bn"])),
         "joinn_dbias": ratio(dwbn[1], jb["bn"]["dbias"], bound_dbias(jb["bn"]))}
    for pre, xx, got_dx, dwb, b in (("join3_", x3, dx3, dwb3, jb["b3"]), ("joins_", xs, dxs, dwbs, jb["bs"])):
        if b is not None:
            r[pre + "dx"] = ratio(got_dx, b["dx"], bound_dx(xx, b))
            r[pre + "dweight"] = ratio(dwb[0], b["dweight"], bound_dweight(b))
            r[pre + "dbias"] = ratio(dwb[1], b["dbias"], bound_dbias(b))
    return r


def gate_mismatches(y_kernel, f, bound):
    """(elements where y_kernel > 0 disagrees with y64 > 0 although |y64| (before the ReLU) exceeds its bound,
    elements inside the bound, where the sign is the kernel's to decide)"""
    decided = f["pre"].abs() > bound
    bad = decided & ((y_kernel > 0) != (f["pre"] > 0))
    return int(bad.sum()), int((~decided).sum())


def check_gate(case, y_kernel, f, bound):
    bad, inside = gate_mismatches(y_kernel, f, bound)
    print("rowbn-gate %s: %d elements inside the bound, %d mismatches outside" % (case, inside, bad))
    assert bad == 0, "%s: the ReLU gate differs from f64 at %d elements outside y's bound" % (case, bad)


# ---------------------------------------------------------------- inputs

def make_mask(kind, n_rois, seed, device="cpu"):
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "all_dead":
        m = torch.zeros((n_rois,))
    elif kind == "one_live":
        m = torch.zeros((n_rois,))
        m[(2 * n_rois) // 3] = 1.0
    else:
        m = (torch.rand((n_rois,), generator=g) > 0.3).float()                 # about 70 % live
        if kind == "dead_run":
            m[n_rois // 5:n_rois // 5 + min(n_rois // 2, 300)] = 0.0           # longer than a row slab
            m[-3:] = 0.0                                                        # dead last rows
        m[0] = 1.0
    return m.to(device)


def make_case(seed, M, C, device="cpu", cols=None):
    """Inputs that stress the kernels: per-column mean spread over [-8, 8] and std over [0.05, 4] (in shuffled
    order); column 0 constant (var = 0, rstd = eps^-1/2), column 1 all zero; weights in [-1.5, 1.5] with exact zeros,
    column 2 with weight 0 and bias 0 (y = 0 exactly: the strict > keeps the gate closed); dy and dres with
    per-column scales over two decades.  cols: keep only the first `cols` columns of the C-wide case."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.linspace(-8.0, 8.0, C)[torch.randperm(C, generator=g)]
    sd = torch.logspace(-1.30103, 0.60206, C)[torch.randperm(C, generator=g)]      # 0.05 .. 4
    gs = torch.logspace(-1.0, 1.0, C)[torch.randperm(C, generator=g)]
    w = torch.rand((C,), generator=g) * 3.0 - 1.5
    b = torch.rand((C,), generator=g) - 0.5
    w[2::7] = 0.0
    w[3] = -0.75
    b[2] = 0.0
    k = C if cols is None else cols
    mu, sd, gs, w, b = (t[:k].clone() for t in (mu, sd, gs, w, b))
    x = torch.randn((M, k), generator=g) * sd + mu
    x[:, 0] = 5.3
    x[:, 1] = 0.0
    dy = torch.randn((M, k), generator=g) * gs
    dres = torch.randn((M, k), generator=g) * gs.flip(0)
    rm = torch.rand((k,), generator=g) * 0.2 - 0.1
    rv = torch.rand((k,), generator=g) * 1.5 + 0.5
    return {n: t.to(device) for n, t in dict(x=x, w=w, b=b, dy=dy, dres=dres, rm=rm, rv=rv).items()}


# ---------------------------------------------------------------- kernel model

def _r32(t):
    return t.float().double()          # one rounding to f32


def _fma32(a, b, c):
    return _r32(a * b + c)             # a, b f32 values held in f64: the product is exact, the sum rounds once


def _tail_rows(M, RS, rpb, device):
    """bool [M]: the rows a slab's one-row tail loop (for (; r < r1; r += RS)) takes"""
    r = torch.arange(M, device=device)
    blk = r // rpb
    off = r - blk * rpb
    rows_in = (M - blk * rpb).clamp_max(rpb)
    lr, k = off % RS, off // RS
    cnt = (rows_in - lr + RS - 1) // RS
    return (cnt % 2 == 1) & (k == cnt - 1)


def _slab_sums(s_vals, q_vals, include, M, geom, drop_last):
    """f64 column sums: one partial per slab, then the finish kernel's fixed order (64 groups of every 64th partial)"""
    L, RS, nb, rpb = geom
    blk = torch.arange(M, device=s_vals.device) // rpb
    part = torch.zeros((2, nb, s_vals.shape[1]), dtype=torch.float64, device=s_vals.device)
    part[0].index_add_(0, blk[include], s_vals[include])
    part[1].index_add_(0, blk[include], q_vals[include])
    if drop_last and nb == MAX_PARTIAL_BLOCKS:
        part[:, (M - 1) // rpb] = 0.0
    grp = torch.stack([part[:, k::64].sum(1) for k in range(min(64, nb))], 0)
    tot = grp.sum(0)
    return tot[0], tot[1]


def model_forward(x, w, b, eps, relu, mask=None, per=1, pos_major=False, geom_C=None, defects=""):
    """The forward kernels' arithmetic in torch: f64 sums per slab, the f32 roundings of rowbn_fwd_finish_kernel, fma
    as an f64 product-sum rounded once.  geom_C: the width the geometry is taken from when x holds only the first
    columns of a wider case.  defects: letters of the seeded defects (a, b, d, f, g here; see the issue list in
    test_rowbn_reference_cpu.py).  Returns mean, var, rstd, scale, shift, y (f32) and count."""
    M, Cd = x.shape
    geom = geometry(M, geom_C or Cd)
    x, w, b = x.double(), w.double(), b.double()
    live = row_live(mask, M, per, pos_major, roi_major_bug="d" in defects)
    inc = torch.ones((M,), dtype=torch.bool, device=x.device) if live is None else live.clone()
    if "a" in defects:
        inc &= ~_tail_rows(M, geom[1], geom[3], x.device)
    s, q = _slab_sums(x, x * x, inc, M, geom, "g" in defects)
    n = float(M) if (mask is None or "b" in defects) else _count(mask, M, per)
    mu = s / n
    v = (q / n - mu * mu).clamp_min(0.0)
    rs = _r32(1.0 / torch.sqrt(v + _eps32(eps)))
    scl = _r32(rs * w)
    if "f" in defects:
        scl = (scl.float().view(torch.int32) + 64).view(torch.float32).double()
    mean, var = _r32(mu), _r32(v)
    shift = _r32(b - _r32(mean * scl))
    y = _fma32(x, scl, shift)
    if relu:
        y = y.clamp_min(0.0)
    if live is not None:
        y[~live] = 0.0
    out = dict(mean=mean, var=var, rstd=rs, scale=scl, shift=shift, y=y)
    out = {k: t.float() for k, t in out.items()}
    out["count"] = _count(mask, M, per)
    return out


def model_backward(x, dy, w, stats, relu, mask=None, per=1, pos_major=False, geom_C=None, defects="", entry=None):
    """The backward kernels' arithmetic (stats: the forward's f32 mean, rstd, scale, shift as a dict).  entry =
    (dys, possel, n_rois): the entry gradient, summed in f32.  defects: a, b, c, d, e, g.  Returns dx, dweight,
    dbias (f32)."""
    M, Cd = x.shape
    geom = geometry(M, geom_C or Cd)
    L = geom[0]
    x, w = x.double(), w.double()
    mean, rstd, scale, shift = (stats[k].double() for k in ("mean", "rstd", "scale", "shift"))
    g = dy.double()
    if entry is not None:
        g = _r32(entry_total(dy, entry[0], entry[1], entry[2]))
    live = row_live(mask, M, per, pos_major, roi_major_bug="d" in defects)
    if relu:
        u = torch.where(_fma32(x, scale, shift) > 0, g, torch.zeros_like(g))
        us = u
        if "e" in defects and Cd > 4 * L:        # later column passes gate with the first pass's scale / shift
            col = torch.arange(Cd, device=x.device) % (4 * L)
            us = torch.where(_fma32(x, scale[col], shift[col]) > 0, g, torch.zeros_like(g))
    else:
        u = us = g
    inc = torch.ones((M,), dtype=torch.bool, device=x.device)
    if live is not None and "c" not in defects:
        inc = live.clone()
    if "a" in defects:
        inc &= ~_tail_rows(M, geom[1], geom[3], x.device)
    sg, sgx = _slab_sums(us, us * x, inc, M, geom, "g" in defects)
    n = float(M) if (mask is None or "b" in defects) else _count(mask, M, per)
    sum_g_xhat = (sgx - mean * sg) * rstd
    a = w * rstd
    k1 = a * rstd * sum_g_xhat / n
    k0 = a * sg / n - k1 * mean
    ka, k0, k1 = _r32(a), _r32(k0), _r32(k1)
    dx = _fma32(-k1, x, _fma32(ka, u, -k0))
    if live is not None:
        dx[~live] = 0.0
    return dict(dx=dx.float(), dweight=sum_g_xhat.float(), dbias=sg.float())


def model_apply(x, scale, shift, relu):
    """rowbn_apply: y = act(fma(x, scale, shift)) with given f32 scale / shift"""
    y = _fma32(x.double(), scale.double(), shift.double())
    return (y.clamp_min(0.0) if relu else y).float()


def model_join_forward(x3, bn3, other, bns, bnn, mask=None, geom_C=None):
    """rowbn_join_forward from the layer models: out = fl(y3 + o), y3 the bn3 model's output (no ReLU, zero on dead
    rows), o the shortcut norm's or `other` itself; then the next norm with ReLU over out.  Position-major rows.
    Returns out, y (f32) and the three norms' model_forward dicts (the shortcut's None in the identity form)."""
    M = x3.shape[0]
    per = M // mask.numel() if mask is not None else 1
    m3 = model_forward(x3, bn3[0], bn3[1], bn3[2], False, mask, per, True, geom_C)
    ms = model_forward(other, bns[0], bns[1], bns[2], False, mask, per, True, geom_C) if bns is not None else None
    out = (m3["y"].double() + (ms["y"] if ms is not None else other).double()).float()
    mn = model_forward(out, bnn[0], bnn[1], bnn[2], True, mask, per, True, geom_C)
    return out, mn["y"], m3, ms, mn


def model_join_backward(out, dy, dres, x3, xs, wn, sn, w3, s3, ws, ss, mask=None, geom_C=None):
    """rowbn_join_backward from the layer models: g = fl(dx_n + dres) (dx_n zero on dead rows), then bn3's and the
    shortcut norm's backward over g, neither with a ReLU.  sn / s3 / ss: model_forward dicts.  Returns g and the three
    model_backward dicts (the shortcut's None in the identity form)."""
    M = out.shape[0]
    per = M // mask.numel() if mask is not None else 1
    bn = model_backward(out, dy, wn, sn, True, mask, per, True, geom_C)
    g = bn["dx"] if dres is None else (bn["dx"].double() + dres.double()).float()
    b3 = model_backward(x3, g, w3, s3, False, mask, per, True, geom_C)
    bs = model_backward(xs, g, ws, ss, False, mask, per, True, geom_C) if xs is not None else None
    return g, bn, b3, bs
