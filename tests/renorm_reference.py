"""Shared by test_renorm_cpu.py and test_gpu_renorm.py: a plain float64 statement of batch renormalisation as the 'BN'
sites run it with cfg.TRAIN.USE_BRN (tf.layers.batch_normalization(renorm=True, renorm_clipping=None,
renorm_momentum=0.99), restated from the issue's text, not from the kernels), elementwise error bounds counted by THE
RULE of rowbn_reference.py (same U, E, SLACK), and switches that seed defects into the statement itself.  torch only,
any device, no import of the package.

Per channel a layer carries W = renorm_weight, Rm = renorm_mean, Rs = renorm_stddev (all zero at first) next to the
running statistics.  One training step over the n live rows, rho = renorm_momentum, m = momentum:

    mu, v       batch mean and biased variance;  sigma = sqrt(v + eps)
    r = sigma / (Rs + (1 - W) sigma);   d = (mu - (Rm + (1 - W) mu)) / (Rs + (1 - W) sigma)      from the OLD state
    y = w * ((x - mu) / sigma * r + d) + b        then the ReLU; dead rows are zero
    Rm' = Rm + (mu - Rm)(1 - rho);  Rs' = Rs + (sigma - Rs)(1 - rho);  W' = W + (1 - W)(1 - rho)
    running_mean += m (Rm' / W' - running_mean);   running_var += m ((Rs' / W')^2 - eps - running_var)
    backward (r, d constants; g the gated live-row gradient, xhat = (x - mu) / sigma):
    dbias = sum g;  dweight = r sum(g xhat) + d sum g;  dx = w r / sigma (g - sum g / n - xhat sum(g xhat) / n)

eps and m reach the layer as f32 values, rho as a double (1 - rho cancels: f32(0.99) would put 1e-6 of relative error
into every state update); the state is f32.  The references take them as they are stored.

DEFECTS (the `defects` argument, a string of letters):
    u   r and d formed from the UPDATED state
    w   d * sum g left out of dweight
    a   r left out of a (dx as a plain batch norm's)
    n   the n / (n - 1) factor applied to running_var
    e   new_var without - eps
"""
import torch

import rowbn_reference as R

U, E, SLACK = R.U, R.E, R.SLACK
RHO = 0.99
DEFECTS = {"u": "r, d from the updated state", "w": "d * sum g missing from dweight", "a": "r missing from a",
           "n": "n / (n - 1) on running_var", "e": "new_var without - eps"}


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32).double())


def fresh_state(C, device="cpu"):
    z = lambda: torch.zeros((C,), dtype=torch.float32, device=device)
    return dict(mean=z(), stddev=z(), weight=z())


def warm_state(C, weight, seed, device="cpu"):
    """renorm_weight = `weight` everywhere, random renorm_mean in [-2, 2] and renorm_stddev in [0.3, 2.3]: r and d far
    from 1 and 0."""
    g = torch.Generator().manual_seed(7000 + seed)
    return dict(mean=(torch.rand((C,), generator=g) * 4.0 - 2.0).to(device),
                stddev=(torch.rand((C,), generator=g) * 2.0 + 0.3).to(device),
                weight=torch.full((C,), float(weight), dtype=torch.float32).to(device))


# ---------------------------------------------------------------- f64 references

def forward(x, w, b, eps, relu, state, rm0, rv0, momentum, rho=RHO, mask=None, per=1, pos_major=False, defects=""):
    """One training step in f64 of the f32 inputs.  state: dict(mean, stddev, weight) BEFORE the step; rm0 / rv0 the
    running statistics before it.  Returns mean, var, rstd, r, d, scale, shift, y, pre, the new state (`state`), the
    new running statistics (`rm`, `rv`), count, live and the magnitudes the bounds need.  All dead: n = 1, mu = v = 0."""
    f = R.forward(x, w, b, eps, False, mask, per, pos_major)        # mu, v, n, the live rows and |x| magnitudes
    xd, wd, bd = x.double(), w.double(), b.double()
    mu, v, n = f["mean"], f["var"], f["count"]
    eps, rho, mom = f["eps"], float(rho), _f32(momentum)
    sigma = torch.sqrt(v + eps)
    W, Rm, Rs = state["weight"].double(), state["mean"].double(), state["stddev"].double()
    k = 1.0 - rho
    Rm1, Rs1, W1 = Rm + (mu - Rm) * k, Rs + (sigma - Rs) * k, W + (1.0 - W) * k
    Wu, Rmu, Rsu = (W1, Rm1, Rs1) if "u" in defects else (W, Rm, Rs)
    mixed_mean = Rmu + (1.0 - Wu) * mu
    mixed_std = Rsu + (1.0 - Wu) * sigma
    r = sigma / mixed_std
    d = (mu - mixed_mean) / mixed_std
    scale = wd * r / sigma
    shift = bd + wd * d - mu * scale
    pre = wd * ((xd - mu) / sigma * r + d) + bd
    if f["live"] is not None:
        pre[~f["live"]] = 0.0
    y = pre.clamp_min(0.0) if relu else pre
    new_mean = Rm1 / W1
    new_var = (Rs1 / W1) ** 2 - (0.0 if "e" in defects else eps)
    if "n" in defects:
        new_var = new_var * (n / max(n - 1.0, 1.0))
    rm = rm0.double() + mom * (new_mean - rm0.double())
    rv = rv0.double() + mom * (new_var - rv0.double())
    f.update(sigma=sigma, r=r, d=d, scale=scale, shift=shift, pre=pre, y=y, mixed_mean=mixed_mean, mixed_std=mixed_std,
             W=W, Rm=Rm, Rs=Rs, k=k, mom=mom, state=dict(mean=Rm1, stddev=Rs1, weight=W1), rm=rm, rv=rv,
             rm0=rm0.double(), rv0=rv0.double())
    return f


def backward(x, dy, w, mean, rstd, r, d, gate=None, mask=None, per=1, pos_major=False, defects=""):
    """dx, dweight, dbias in f64.  mean, rstd, r, d are inputs of the backward (the forward's own stored f32 values);
    gate (bool [M, C] or None) is the ReLU mask, given as data.  Dead rows: dx = 0, nothing added to the sums."""
    x, dy, w, mean, rstd, r, d = (t.double() for t in (x, dy, w, mean, rstd, r, d))
    M = x.shape[0]
    live = R.row_live(mask, M, per, pos_major)
    n = R._count(mask, M, per)
    g = dy if gate is None else torch.where(gate, dy, torch.zeros_like(dy))
    if live is not None:
        g = g * live.unsqueeze(1)
    xhat = (x - mean) * rstd
    sg = g.sum(0)
    sgx = (g * xhat).sum(0)
    dweight = r * sgx + (0.0 if "w" in defects else d * sg)
    a = w * rstd * (1.0 if "a" in defects else r)
    dx = a * (g - sg / n - xhat * sgx / n)
    if live is not None:
        dx[~live] = 0.0
    k1 = a * rstd * sgx / n
    k0 = a * sg / n - k1 * mean
    return dict(dx=dx, dweight=dweight, dbias=sg, a=a, k0=k0, k1=k1, g=g, n=n, M=M, live=live, mean=mean, rstd=rstd,
                r=r, d=d, sgx=sgx, sum_abs_g=g.abs().sum(0), sum_abs_gx=(g * x).abs().sum(0))


# ---------------------------------------------------------------- bounds
# The kernels' order (csrc/plumbing/rowbn.hip, struct Renorm): everything up to r, d, mixed_mean and the new state in
# f64 from the f64 mu / v; then in f32  scale = (rstd * r) * w  and  shift = fmaf(-scale, mixed_mean, b).  The stock
# route's f32 torch ops are not counted here: the CPU tests run it in f64.

def _d_sigma(f):
    # sigma = sqrt(v + eps): |d sigma / d v| = 1 / (2 sigma), at the smallest v the f64 error of v allows; one rounding
    return 0.5 * R._f_var(f) * R._rs_hi(f) + E * f["sigma"]


def _f_r(f):
    # f64 part of r = sigma / (Rs + (1 - W) sigma): d r / d sigma = Rs / mixed_std^2; 4 f64 operations on r's path
    return f["Rs"] / f["mixed_std"] ** 2 * _d_sigma(f) + 4 * E * f["r"].abs()


def _f_mm(f):
    # f64 part of mixed_mean = Rm + (1 - W) mu: mu's error times (1 - W), 3 roundings of terms <= |Rm| + |mu|
    return (1.0 - f["W"]).abs() * R._f_mean(f) + 3 * E * (f["Rm"].abs() + f["mean"].abs())


def _f_d(f):
    # f64 part of d = (mu - mixed_mean) / mixed_std: numerator W mu - Rm (mu's error times W, the roundings of
    # mixed_mean and of the difference, which cancel at the size of |Rm| + |mu|), the divisor's error times |d| /
    # mixed_std, the division
    num = f["W"].abs() * R._f_mean(f) + 4 * E * (f["Rm"].abs() + f["mean"].abs())
    return (num + f["d"].abs() * (1.0 - f["W"]).abs() * _d_sigma(f)) / f["mixed_std"] + 2 * E * f["d"].abs()


def bound_r(f):
    """[C].  r = (float)(sigma / mixed_std): 1 rounding, u|r|; the f64 part (_f_r)."""
    return SLACK * (U * f["r"].abs() + _f_r(f))


def bound_d(f):
    """[C].  d = (float)((mu - mixed_mean) / mixed_std): 1 rounding, u|d|; the f64 part (_f_d)."""
    return SLACK * (U * f["d"].abs() + _f_d(f))


def _f_scale(f):
    return f["w"].abs() * (f["r"].abs() * R._f_rstd(f) + R._rs_hi(f) * _f_r(f))


def bound_scale(f):
    """[C].  scale = (rstd_f32 * r_f32) * w in f32: 4 roundings (rstd -> f32, r -> f32, two products), 4u|scale|; plus
    |w| times the f64 parts of rstd (times r) and of r (times rstd)."""
    return SLACK * (4 * U * f["scale"].abs() + _f_scale(f))


def bound_shift(f):
    """[C].  shift = fmaf(-scale, mixed_mean_f32, b), s = |scale|: mixed_mean -> f32 (u|mm s|), scale's 4 roundings
    (4u|mm s|), the product and the sum (u|mm s| + u(|b| + |mm s|), one less when fused): 7u|mm s| + u|b|; plus the
    f64 parts of mixed_mean (times s) and of scale (times |mm|)."""
    s, mm = f["scale"].abs(), f["mixed_mean"].abs()
    return SLACK * (7 * U * mm * s + U * f["b"].abs() + s * _f_mm(f) + mm * _f_scale(f))


def bound_y(x, f):
    """[M, C].  y = act(fma(x, scale, shift)): x * scale carries scale's 4 roundings, shift the 7u|mm s| + u|b| of
    bound_shift, the fma rounds once more, u(|x s| + |mm s| + |b|):  5u|x s| + 8u|mm s| + 2u|b|  plus the f64 parts.
    The ReLU does not increase a difference; dead rows are exactly 0."""
    s, mm = f["scale"].abs(), f["mixed_mean"].abs()
    col = 8 * U * mm * s + 2 * U * f["b"].abs() + s * _f_mm(f) + mm * _f_scale(f)
    bd = SLACK * (x.double().abs() * (5 * U * s + _f_scale(f)) + col)
    if f["live"] is not None:
        bd[~f["live"]] = 0.0
    return bd


def _state_errs(f):
    """(err Rm', err Rs', err W'): 1 rounding to f32 each, u|.|; the f64 parts: (1 - rho) times the error of mu /
    sigma, 3 roundings of terms of the size of the operands."""
    k, st = f["k"], f["state"]
    em = U * st["mean"].abs() + k * R._f_mean(f) + 3 * E * (f["Rm"].abs() + f["mean"].abs())
    es = U * st["stddev"].abs() + k * _d_sigma(f) + 3 * E * (f["Rs"].abs() + f["sigma"])
    ew = U * st["weight"].abs() + 3 * E
    return em, es, ew


def bound_state(f):
    """dict of [C] bounds for the new renorm_mean / renorm_stddev / renorm_weight (see _state_errs)."""
    em, es, ew = _state_errs(f)
    return dict(mean=SLACK * em, stddev=SLACK * es, weight=SLACK * ew)


def bound_running(f):
    """([C], [C]) for running_mean / running_var, which the kernel forms from its ROUNDED new state:
    new_mean = Rm' / W' carries err(Rm') / W' + |new_mean| err(W') / W'; q = Rs' / W' likewise and new_var = q^2 - eps
    twice |q| times that; each enters times m; the result rounds once, u|running|; 6 f64 roundings of terms of the
    size of |running| + m |new|."""
    em, es, ew = _state_errs(f)
    st, m = f["state"], f["mom"]
    nm = st["mean"] / st["weight"]
    q = st["stddev"] / st["weight"]
    e_nm = (em + nm.abs() * ew) / st["weight"]
    e_q = (es + q.abs() * ew) / st["weight"]
    bm = U * f["rm"].abs() + m * e_nm + 6 * E * (f["rm0"].abs() + nm.abs())
    bv = U * f["rv"].abs() + m * 2 * q.abs() * e_q + 6 * E * (f["rv0"].abs() + q * q + f["eps"])
    return SLACK * bm, SLACK * bv


def bound_dbias(r):
    """[C].  dbias = (float)sum g: rowbn_reference.bound_dbias (1 rounding, the f64 sum)."""
    return R.bound_dbias(r)


def bound_dweight(r):
    """[C].  dweight = (float)(r * t + d * sg), t = sum(g xhat) = (sgx - mean sg) rstd in f64: 1 rounding, u|dweight|;
    the f64 parts |r| times t's (rowbn_reference._f_dw) and |d| times sg's (M e sum|g|), and the 3 roundings of the two
    products and the sum, 3e(|r t| + |d sg|)."""
    F = (r["r"].abs() * R._f_dw(r) + r["d"].abs() * r["M"] * E * r["sum_abs_g"]
         + 3 * E * ((r["r"] * r["sgx"]).abs() + (r["d"] * r["dbias"]).abs()))
    return SLACK * (U * (r["dweight"].abs() + F) + F)


def bound_dx(x, r):
    """[M, C].  dx = fma(-k1, x, fma(a, g, -k0)) with a = (w r) rstd, k1, k0 in f64 rounded to f32 once: the count of
    rowbn_reference.bound_dx (3u|a g| + 3u|k0| + 2u|k1 x| and the f64 parts of k1, k0), and one more f64 product (w r)
    on the path of all three coefficients: e(|a g| + |k0| + |k1 x|)."""
    extra = SLACK * E * ((r["a"] * r["g"]).abs() + r["k0"].abs() + (r["k1"] * x.double()).abs())
    if r["live"] is not None:
        extra[~r["live"]] = 0.0
    return R.bound_dx(x, r) + extra


def stat_ratios(got, f, prefix=""):
    """worst |error| / bound of the seven statistic rows (got: mean, var, rstd, scale, shift, r, d by name)"""
    bounds = dict(mean=R.bound_mean, var=R.bound_var, rstd=R.bound_rstd, scale=bound_scale, shift=bound_shift, r=bound_r,
                  d=bound_d)
    return {prefix + k: R.ratio(got[k], f[k], fn(f)) for k, fn in bounds.items()}


def stats_dict(stats):
    """the [7, C] block of a renorm call, by name"""
    return dict(mean=stats[0], var=stats[1], rstd=stats[2], scale=stats[3], shift=stats[4], r=stats[5], d=stats[6])


def forward_ratios(x, f, got, state, rm, rv, prefix=""):
    """worst |error| / bound of every forward output: `got` (the seven statistics and y by name), the new state (dict)
    and the running statistics, against forward()'s f."""
    out = stat_ratios(got, f, prefix)
    out[prefix + "y"] = R.ratio(got["y"], f["y"], bound_y(x, f))
    bs = bound_state(f)
    for k in ("mean", "stddev", "weight"):
        out[prefix + "renorm_" + k] = R.ratio(state[k], f["state"][k], bs[k])
    bm, bv = bound_running(f)
    out[prefix + "running_mean"] = R.ratio(rm, f["rm"], bm)
    out[prefix + "running_var"] = R.ratio(rv, f["rv"], bv)
    return out


def backward_ratios(x, b, got, prefix=""):
    """the same for dx, dweight, dbias (got by name) against backward()'s b"""
    return {prefix + "dx": R.ratio(got["dx"], b["dx"], bound_dx(x, b)),
            prefix + "dweight": R.ratio(got["dweight"], b["dweight"], bound_dweight(b)),
            prefix + "dbias": R.ratio(got["dbias"], b["dbias"], bound_dbias(b))}


def make_steps(seed, M, C, steps=3, device="cpu"):
    """`steps` batches of one layer whose mean and spread change from step to step (rowbn_reference.make_case per
    step, shifted by 1.5 per step and scaled by 1, 0.6, 1.7, ...), sharing weight, bias and running statistics."""
    cases = [R.make_case(seed + 31 * i, M, C, device) for i in range(steps)]
    scale = [1.0, 0.6, 1.7, 0.9, 1.3]
    for i, c in enumerate(cases):
        c["x"] = (c["x"] * scale[i % len(scale)] + 1.5 * i).contiguous()
        for k in ("w", "b", "rm", "rv"):
            c[k] = cases[0][k]
    return cases
