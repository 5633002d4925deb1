"""Shared by test_optim_cpu.py and test_gpu_optim.py: a plain numpy float64 statement of the three optimiser updates
of wssdl_bus_amd/fast_rcnn/optim.py (csrc/plumbing/optim.hip) and of the two learning-rate schedules, with an
elementwise error bound for every output, counted from the f32 roundings on its path, and the comparison of an
optimiser object with it (snapshot, check_step).  numpy only, no import of the package.

THE UPDATES (inputs are f32 data: p, g, the state, and the scalars lr, eps, mu, b1, b2 rounded to f32; alpha_t is
computed in f64 from the f32 lr and the f64 betas 0.9 / 0.999 and rounded to f32 once -- that rounding is part of the
specification, so alpha_t is data too, like 1 - b1 and 1 - b2, which are exact in f32 by Sterbenz's lemma):

  Adam      d1 = g - m;  t1 = d1 * (1 - b1);  m' = m + t1
            gg = g * g;  d2 = gg - v;  t2 = d2 * (1 - b2);  v' = v + t2
            s = sqrt(v');  den = s + eps;  num = m' * alpha_t;  q = num / den;  p' = p - q
  AMSGrad   m', v' as above;  w = max(vhat, v') (the new vhat);  s = sqrt(w);  the rest as above
  Nesterov  a1 = accum * mu;  acc' = a1 + g;  t0 = g * lr;  t1 = acc' * mu;  t2 = t1 * lr;  sm = t0 + t2;  p' = p - sm

THE RULE FOR BOUNDS (as in loss_reference.py and rowbn_reference.py).  u = 2^-24 is the unit roundoff of f32.  Every
f32 rounding on an output's path costs u times the magnitude of the term it rounds; the error of an intermediate
reaches the output multiplied by whatever the intermediate is multiplied by.  sqrt and the division are allowed 1 ulp
each (the compile default is correctly rounded, half an ulp); an ulp is at most 2 u relative.  Counted, with E(x) the
bound of x's error:

  E(m')   = u |m'| + 2 u |t1|                    3 roundings: d1 (reaches t1 as u |d1| (1 - b1) = u |t1|), t1, m'
  E(v')   = u |v'| + 2 u |t2| + u (1 - b2) gg    4 roundings: gg (reaches t2 times (1 - b2)), d2, t2, v'
  E(w)    = E(v') where v' + E(v') >= vhat, else 0     max is 1-Lipschitz; below vhat by more than E(v') the stored
                                                       vhat is returned unchanged, exactly
  E(s)    = 2 u s + min(E(w) / s, sqrt(E(w)))    1 ulp, plus |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b) and <= sqrt|a - b|
  E(den)  = u den + E(s)
  E(num)  = u |num| + alpha_t E(m')
  E(q)    = 2 u |q| + E(num) / den + |q| E(den) / den          1 ulp, plus the quotient's two first-order terms
  E(p')   = u |p'| + E(q)                        12 roundings on the path in all (13 with AMSGrad's exact max: none added)

  E(acc') = u |acc'| + u |a1|                    2 roundings
  E(t1)   = u |t1| + mu E(acc');  E(t2) = u |t2| + lr E(t1);  E(sm) = u |sm| + u |t0| + E(t2)
  E(p')   = u |p'| + E(sm)                       7 roundings on the path

Every bound is multiplied by SLACK = 1 + 2^-20 (products of two error terms, the rounding of this f64 reference
itself) and gets FLOOR = 2^-149 per rounding on the path added (a result in the subnormal range is rounded to a
multiple of 2^-149, not to u relative).  No number was chosen by looking at what a GPU or the code under test
produced: the bounds come from the count.

THE SCHEDULES.  piecewise_lr: TensorFlow's piecewise_constant(global_step, [int(0.75 * max_iters)], [lr, 0.1 * lr]),
which keeps the first value while global_step <= boundary.  plateau_lrs: the rate after each validation loss under the
reference's ReduceLROnPlateau (mode 'min', no cool-down), written as a fold over the losses.
"""
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
FLOOR = 2.0 ** -149
B1, B2 = 0.9, 0.999


def f32(x):
    return float(np.float32(x))


def alpha_t(lr, t, b1=B1, b2=B2):
    """lr (rounded to f32) * sqrt(1 - b2^t) / (1 - b1^t) in f64, rounded to f32 once"""
    return f32(f32(lr) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def _d(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def _out(x, e, n):
    return x, e * SLACK + n * FLOOR


def adam(p, g, m, v, lr, t, eps=0.1, b1=B1, b2=B2, vhat=None):
    """One step of Adam (vhat None) or AMSGrad from f32 arrays.  -> {name: (f64 value, bound)} for p, m, v (, vhat)."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    omb1, omb2 = 1.0 - f32(b1), 1.0 - f32(b2)
    assert f32(omb1) == omb1 and f32(omb2) == omb2             # exact in f32
    al, eps = alpha_t(lr, t, b1, b2), f32(eps)
    t1 = (g - m) * omb1
    m1 = m + t1
    e_m = U * np.abs(m1) + 2 * U * np.abs(t1)
    gg = g * g
    t2 = (gg - v) * omb2
    v1 = v + t2
    e_v = U * np.abs(v1) + 2 * U * np.abs(t2) + U * omb2 * gg
    out = dict(m=_out(m1, e_m, 3), v=_out(v1, e_v, 4))
    w, e_w = v1, e_v
    if vhat is not None:
        vh = _d(vhat)
        w = np.maximum(vh, v1)
        e_w = np.where(v1 + e_v >= vh, e_v, 0.0)
        out["vhat"] = _out(w, e_w, 4)
    assert (w >= 0).all()
    s = np.sqrt(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(s > 0, np.minimum(e_w / np.where(s > 0, s, 1.0), np.sqrt(e_w)), np.sqrt(e_w))
    e_s = 2 * U * s + prop
    den = s + eps
    e_den = U * den + e_s
    num = m1 * al
    e_num = U * np.abs(num) + al * e_m
    q = num / den
    e_q = 2 * U * np.abs(q) + e_num / den + np.abs(q) * e_den / den
    p1 = p - q
    out["p"] = _out(p1, U * np.abs(p1) + e_q, 12)
    return out


def nesterov(p, g, accum, lr, mu):
    """One step of Nesterov momentum from f32 arrays.  -> {name: (f64 value, bound)} for p, accum."""
    p, g, acc = _d(p), _d(g), _d(accum)
    lr, mu = f32(lr), f32(mu)
    a1 = acc * mu
    acc1 = a1 + g
    e_acc = U * np.abs(acc1) + U * np.abs(a1)
    t0 = g * lr
    t1 = acc1 * mu
    e_t1 = U * np.abs(t1) + mu * e_acc
    t2 = t1 * lr
    e_t2 = U * np.abs(t2) + lr * e_t1
    sm = t0 + t2
    e_sm = U * np.abs(sm) + U * np.abs(t0) + e_t2
    p1 = p - sm
    return dict(accum=_out(acc1, e_acc, 2), p=_out(p1, U * np.abs(p1) + e_sm, 7))


def nesterov_f32(p, g, accum, lr, mu):
    """The same operation order evaluated by numpy in f32 (no contraction): what every route must equal bit for bit.
    -> (p', accum') as f32 arrays."""
    p, g, acc = (np.asarray(a) for a in (p, g, accum))
    assert p.dtype == g.dtype == acc.dtype == np.float32
    lr, mu = np.float32(lr), np.float32(mu)
    acc1 = acc * mu + g
    t0 = g * lr
    t2 = (acc1 * mu) * lr
    return p - (t0 + t2), acc1


def step(kind, p, g, state, lr, t, eps=0.1, mu=0.9):
    """kind 'adam' | 'amsgrad' | 'sgd'; state {slot: f32 array} -> {name: (value, bound)} (names: p and the slots)"""
    if kind == "sgd":
        return nesterov(p, g, state["accum"], lr, mu)
    return adam(p, g, state["m"], state["v"], lr, t, eps, vhat=state["vhat"] if kind == "amsgrad" else None)


# ---------------------------------------------------------------- schedules

def piecewise_lr(lr, global_step, max_iters):
    return lr if global_step <= int(max_iters * 0.75) else lr * 0.1


def plateau_lrs(losses, lr, factor=0.5, patience=5, epsilon=1e-3, min_lr=0.0):
    """The rate after each loss.  A loss below best - epsilon is a new best and clears the wait; any other loss first
    reduces the rate if the wait has reached `patience` and the rate is above min_lr (clearing the wait), then adds
    one to the wait."""
    best, wait, out = math.inf, 0, []
    for x in losses:
        if x < best - epsilon:
            best, wait = x, 0
        else:
            if wait >= patience and lr > min_lr:
                lr, wait = max(lr * factor, min_lr), 0
            wait += 1
        out.append(lr)
    return out


# ---------------------------------------------------------------- comparing an optimiser object with the reference

def to_numpy(t):
    return t.detach().cpu().numpy().copy()


def snapshot(opt):
    """per parameter of a ReferenceOptimizer: f32 copies of p, its gradient (None when it has none) and its state"""
    return [dict(p=to_numpy(p), g=None if p.grad is None else to_numpy(p.grad),
                 **{s: to_numpy(v[i]) for s, v in opt.views.items()}) for i, p in enumerate(opt.params)]


def check_step(opt, before, t, lr, mu=0.9, what="", scale=1.0):
    """Every element of every parameter and state tensor after step t against the f64 reference applied to the f32
    snapshot taken before it, inside `scale` times the counted bound; a parameter without a gradient must be bit-
    identical, state included.  -> the worst error-to-bound ratio."""
    worst = 0.0
    for i, (p, b) in enumerate(zip(opt.params, before)):
        now = dict(p=to_numpy(p), **{s: to_numpy(v[i]) for s, v in opt.views.items()})
        if b["g"] is None:
            for k in now:
                assert np.array_equal(now[k], b[k]), (what, i, k)
            continue
        ref = step(opt.kind, b["p"], b["g"], {s: b[s] for s in opt.views}, lr, t, opt.eps, mu)
        assert sorted(ref) == sorted(now)
        for k, (want, bound) in ref.items():
            err = np.abs(now[k].astype(np.float64) - want)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert ratio <= scale, (what, opt.kind, t, i, k, ratio)
    return worst
