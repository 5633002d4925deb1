"""-m gpu: batch renormalisation (cfg.TRAIN.USE_BRN) on the fused row-norm kernels (csrc/plumbing/rowbn.hip: the renorm
forms of the two finish kernels; networks/_plumbing.py: the `renorm` argument of the fused calls).

* Every output of a renorm layer -- y, the [7, C] statistic block (mean, var, rstd, scale, shift, r, d), dx, dweight,
  dbias, the three state vectors, the running statistics -- against the f64 statement of tests/renorm_reference.py
  within its counted bounds; the counter exactly.  The backward is staged as in test_gpu_rowbn_reference.py: its
  reference takes the forward's own f32 mean, rstd, r, d and the kernel's ReLU gate as data.
* The state, the running statistics, r, d, scale and shift EXACTLY against a host restatement (numpy float64, every
  operation rounded on its own) of the finish kernel's documented order, from the f64 partial sums the slab kernel
  left in the workspace (as test_gpu_rowbn_finish.py does for the plain layer):
      mu = s / n;  v = max(fma(-mu, mu, q / n), 0);  sigma = sqrt(v + eps);  rstd = (float)(1 / sqrt(v + eps))
      omw = 1 - W;  mm = Rm + omw * mu;  ms = Rs + omw * sigma;  r = (float)(sigma / ms);  d = (float)((mu - mm) / ms)
      scale = (rstd * r) * w  (f32);  shift = fmaf(-scale, (float)mm, b)
      k = 1 - rho;  Rm' = (float)(Rm + (mu - Rm) * k);  Rs' = (float)(Rs + (sigma - Rs) * k);  W' = (float)(W + (1 - W) * k)
      running_mean = (float)(rm + (Rm' / W' - rm) * m);  q = Rs' / W';  running_var = (float)(rv + ((q * q - eps) - rv) * m)
* Three steps on one layer, the state carried by the kernels.
* A fresh layer's first step is the plain fused layer bit for bit.
* The fused routes in renorm mode -- the join in every form, block 1's entry, the stats-only call in front of the
  patch gather -- against the separate fused renorm layers, torch.equal on outputs, gradients and every buffer.
* ResNetTrunk(18) and the ResNet-18 head with cfg.TRAIN.USE_BRN = True, two steps: fused routes against the unfused
  switches with torch.equal, and against the stock-PyTorch route by the criterion of tests/network_reference.py
  (H the fused route, S the stock route in f32 on the GPU, D the stock route in f64 on the CPU; K = 16 as in
  test_gpu_network_reference.py, the largest value that criterion admits).
* The plain fused layer substituted for the renorm layer falls outside the bounds from a warm state and at step 2.

Shapes from rowbn_reference.TABLE / MASK_SPLITS: (1, 4) one row, variance exactly 0; (259, 16); (1041, 512) odd last
slab; (4099, 1024) more partial blocks than finish groups; (1031, 2048) two column passes; masks (37, 49) and
(1500, 16) at C = 256, kinds random and all_dead, both layouts."""
import copy
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import network_reference as NR
import renorm_reference as N
import rowbn_reference as R

pytestmark = pytest.mark.gpu

EPS, MOM, RHO = 1e-3, 0.01, 0.99
DEV = "cuda"
K_NET = 16.0
LOG = {}
SHAPES = [(1, 4), (259, 16), (1041, 512), (4099, 1024), (1031, 2048)]


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None, "plumbing library not built"
    yield _plumbing
    for k in sorted(LOG):
        print("renorm-worst %s %.4g" % (k, LOG[k]))


@functools.lru_cache(maxsize=4)
def _steps(seed, M, C):
    return N.make_steps(seed, M, C, 3, DEV)


def _state(kind, C, seed=3):
    if kind == "fresh":
        return N.fresh_state(C, DEV)
    return N.warm_state(C, {"warm": 0.875, "w001": 0.01, "w1": 1.0}[kind], seed, DEV)


def _buffers(c, state):
    """fresh copies of everything the forward updates: (running, renorm) as the binding takes them"""
    run = (c["rm"].clone(), c["rv"].clone(), MOM, torch.tensor([5], dtype=torch.int64, device=DEV))
    ren = (state["mean"].clone(), state["stddev"].clone(), state["weight"].clone(), RHO)
    return run, ren


def _layer(P, case, c, relu, state, mask=None, per=1, pm=False, run=None, ren=None, nbt=6):
    """one forward and backward of a renorm layer from `state`, every output against its bound"""
    x, w, b, dy = c["x"], c["w"], c["b"], c["dy"]
    if run is None:
        run, ren = _buffers(c, state)
    rm0, rv0 = run[0].clone(), run[1].clone()
    y, stats, count = P.rowbn_forward(x, w, b, EPS, relu, mask, pm, running=run, renorm=ren)
    assert stats.shape == (7, x.shape[1])
    f = N.forward(x, w, b, EPS, relu, state, rm0, rv0, MOM, RHO, mask, per, pm)
    got = N.stats_dict(stats)
    got["y"] = y
    r = N.forward_ratios(x, f, got, dict(mean=ren[0], stddev=ren[1], weight=ren[2]), run[0], run[1])
    R.check_ratios(case, r, LOG)
    R.check_gate(case, y, f, N.bound_y(x, f))
    assert int(run[3]) == nbt, "%s: num_batches_tracked is %d" % (case, int(run[3]))
    assert torch.equal(ren[2], ren[2][0].expand_as(ren[2])), "%s: renorm_weight is not one value per channel" % case
    if mask is not None:
        assert float(count[0]) == f["count"] and not bool(y[~f["live"]].any()), case
    gate = (y > 0) if relu else None
    dx, dw, db = P.rowbn_backward(x, dy, w, stats, relu, mask, pm)
    bw = N.backward(x, dy, w, stats[0], stats[2], stats[5], stats[6], gate, mask, per, pm)
    R.check_ratios(case, N.backward_ratios(x, bw, dict(dx=dx, dweight=dw, dbias=db)), LOG)
    if mask is not None:
        assert not bool(dx[~f["live"]].any()), "%s: dx is not zero on dead rows" % case
    return y, stats, (dx, dw, db), run, ren, f


@pytest.mark.parametrize("state", ["fresh", "warm"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", SHAPES)
def test_single_norm(P, M, C, relu, state):
    c = _steps(41, M, C)[1]
    case = "renorm %dx%d relu=%d %s" % (M, C, relu, state)
    _, stats, _, _, _, f = _layer(P, case, c, relu, _state(state, C))
    if M == 1:
        assert not bool(stats[1].any()), "%s: one row, var is not 0" % case
    if state == "warm":
        assert float((f["r"] - 1).abs().max()) > 0.2 and float(f["d"].abs().max()) > 0.2


@pytest.mark.parametrize("weight", ["w001", "w1"])
def test_single_norm_other_warm_weights(P, weight):
    c = _steps(41, 1041, 512)[2]
    _layer(P, "renorm 1041x512 %s" % weight, c, True, _state(weight, 512, 5))


@pytest.mark.parametrize("pm", [False, True], ids=["roi_major", "pos_major"])
@pytest.mark.parametrize("kind", ["random", "all_dead"])
@pytest.mark.parametrize("n_rois,per", [(37, 49), (1500, 16)])
def test_masked_both_layouts(P, n_rois, per, kind, pm):
    C = 256
    c = _steps(42, n_rois * per, C)[1]
    mask = R.make_mask(kind, n_rois, n_rois, DEV)
    case = "renorm masked %dx%d %s pm=%d" % (n_rois, per, kind, pm)
    _, stats, (dx, dw, db), _, _, f = _layer(P, case, c, True, _state("warm", C), mask, per, pm)
    if kind == "all_dead":
        assert f["count"] == 1.0 and not bool(stats[0].any()) and not bool(stats[1].any()), case
        assert not bool(dw.any()) and not bool(db.any()) and not bool(dx.any()), case


def test_three_steps_state_carried_by_the_kernels(P):
    M, C = 1041, 512
    steps = _steps(43, M, C)
    run, ren = _buffers(steps[0], N.fresh_state(C, DEV))
    for i, c in enumerate(steps):
        state = dict(mean=ren[0].clone(), stddev=ren[1].clone(), weight=ren[2].clone())
        _layer(P, "renorm sequence step %d" % (i + 1), c, True, state, run=run, ren=ren, nbt=6 + i)
    want = torch.tensor(1.0 - RHO ** 3)
    assert abs(float(ren[2][0]) - float(want)) <= 4 * R.U, "renorm_weight after three steps"


def test_fresh_first_step_is_the_plain_layer_bit_for_bit(P):
    c = _steps(41, 1041, 512)[0]
    run, ren = _buffers(c, N.fresh_state(512, DEV))
    y, stats, _ = P.rowbn_forward(c["x"], c["w"], c["b"], EPS, True, running=run, renorm=ren)
    yp, sp, _ = P.rowbn_forward(c["x"], c["w"], c["b"], EPS, True)
    assert torch.equal(y, yp) and torch.equal(stats[:5], sp)
    assert torch.equal(stats[5], torch.ones_like(stats[5])) and not bool(stats[6].any())
    got, want = P.rowbn_backward(c["x"], c["dy"], c["w"], stats, True), P.rowbn_backward(c["x"], c["dy"], c["w"], sp, True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("how", ["warm", "step2"])
def test_the_plain_layer_in_its_place_misses_the_bounds(P, how):
    """what the parent commit computes: plain batch norm, whatever the renorm state says"""
    C = 512
    steps = _steps(43, 1041, C)
    if how == "warm":
        c, state = steps[1], _state("warm", C)
    else:
        f0 = N.forward(steps[0]["x"], steps[0]["w"], steps[0]["b"], EPS, True, N.fresh_state(C, DEV), steps[0]["rm"],
                       steps[0]["rv"], MOM, RHO)
        c, state = steps[1], {k: v.float() for k, v in f0["state"].items()}
    y, stats, _ = P.rowbn_forward(c["x"], c["w"], c["b"], EPS, True)
    f = N.forward(c["x"], c["w"], c["b"], EPS, True, state, c["rm"], c["rv"], MOM, RHO)
    ry = R.ratio(y, f["y"], N.bound_y(c["x"], f))
    rs = R.ratio(stats[3], f["scale"], N.bound_scale(f))
    print("renorm-plain-substituted %s: y %.3g scale %.3g" % (how, ry, rs))
    assert ry > 1.0 and rs > 1.0


# ---------------------------------------------------------------- the finish kernel restated on the host

FIN_GROUPS, MAX_PARTIAL_BLOCKS = 64, 1024


def _round_f32(fr):
    if fr == 0:
        return np.float32(0.0)
    e = math.frexp(abs(float(fr)))[1]
    scaled = abs(fr) * Fraction(2) ** (24 - e)
    if scaled < 2 ** 23:
        e -= 1
        scaled *= 2
    return np.float32(math.copysign(math.ldexp(float(round(scaled)), e - 24), float(fr)))


def _fma64(a, b, c):
    return np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    dtype=np.float64)


def _fma32(a, b, c):
    return np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    dtype=np.float32)


def _finish_sums(Pt):
    nb, C2 = Pt.shape
    red = np.zeros((FIN_GROUPS, C2), dtype=np.float64)
    for k in range(MAX_PARTIAL_BLOCKS // FIN_GROUPS):
        b = np.arange(FIN_GROUPS) + k * FIN_GROUPS
        on = b < nb
        red[on] = red[on] + Pt[b[on]]
    tot = np.zeros((C2,), dtype=np.float64)
    for g in range(FIN_GROUPS):
        tot = tot + red[g]
    return tot[:C2 // 2], tot[C2 // 2:]


def _host_finish(Pt, n, w, b, rm, rv, Rm, Rs, W):
    f64 = lambda t: t.astype(np.float64)
    eps, mom, rho = float(np.float32(EPS)), float(np.float32(MOM)), RHO       # rho reaches the kernel as a double
    s, q = _finish_sums(Pt)
    mu = s / n
    v = _fma64(-mu, mu, q / n)
    v = np.where(v < 0.0, 0.0, v)
    sigma = np.sqrt(v + eps)
    rstd = (1.0 / np.sqrt(v + eps)).astype(np.float32)
    Rm, Rs, W = f64(Rm), f64(Rs), f64(W)
    omw = 1.0 - W
    mm = Rm + omw * mu
    ms = Rs + omw * sigma
    r = (sigma / ms).astype(np.float32)
    d = ((mu - mm) / ms).astype(np.float32)
    scale = (rstd * r) * w
    shift = _fma32(-scale, mm.astype(np.float32), b)
    k = 1.0 - rho
    lerp = lambda s0, x1, kk: s0 + (x1 - s0) * kk
    Rm1, Rs1, W1 = (lerp(Rm, mu, k).astype(np.float32), lerp(Rs, sigma, k).astype(np.float32),
                    lerp(W, 1.0, k).astype(np.float32))
    qq = f64(Rs1) / f64(W1)
    return dict(mean=mu.astype(np.float32), var=v.astype(np.float32), rstd=rstd, scale=scale, shift=shift, r=r, d=d,
                renorm_mean=Rm1, renorm_stddev=Rs1, renorm_weight=W1,
                running_mean=lerp(f64(rm), f64(Rm1) / f64(W1), mom).astype(np.float32),
                running_var=lerp(f64(rv), qq * qq - eps, mom).astype(np.float32))


@pytest.mark.parametrize("M,C,masked,state", [(259, 16, None, "fresh"), (259, 16, None, "warm"),
                                              (4099, 1024, None, "warm"), (37 * 49, 256, "random", "warm"),
                                              (37 * 49, 256, "all_dead", "warm"), (1, 4, None, "w1")])
def test_state_and_running_statistics_exactly(P, M, C, masked, state):
    c = _steps(44, M, C)[1]
    st = _state(state, C, 9)
    run, ren = _buffers(c, st)
    mask, n_rois, per, pm = None, 0, 1, 0
    n = float(M)
    if masked:
        n_rois, per, pm = 37, 49, 1
        mask = R.make_mask(masked, n_rois, 3, DEV)
        n = max(float(per * int((mask != 0).sum())), 1.0)
    nbytes = P.lib().wsplumb_rowbn_workspace_bytes(M, C)
    nb = R.geometry(M, C)[2]
    assert nbytes == nb * 2 * C * 8
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    y = torch.empty_like(c["x"])
    stats = torch.empty((7, C), dtype=torch.float32, device=DEV)
    count = torch.full((1,), -7.0, device=DEV)
    P._call("wsplumb_rowbn_forward_renorm", c["x"].device, P._p(c["x"]), M, C, P._p(c["w"]), P._p(c["b"]), EPS, 1,
            P._pn(mask), n_rois, per, pm, P._p(y), *[P._p(stats[i]) for i in range(5)], P._p(count), P._p(ws), ws.numel(),
            tail=(P._p(run[0]), P._p(run[1]), MOM, P._p(run[3]), P._p(ren[0]), P._p(ren[1]), P._p(ren[2]), RHO,
                  P._p(stats[5]), P._p(stats[6])))
    torch.cuda.synchronize()
    part = ws.view(torch.float64).view(nb, 2 * C).cpu().numpy().copy()
    cpu = lambda t: t.cpu().numpy()
    want = _host_finish(part, n, cpu(c["w"]), cpu(c["b"]), cpu(c["rm"]), cpu(c["rv"]), cpu(st["mean"]), cpu(st["stddev"]),
                        cpu(st["weight"]))
    got = N.stats_dict(stats)
    got.update(renorm_mean=ren[0], renorm_stddev=ren[1], renorm_weight=ren[2], running_mean=run[0], running_var=run[1])
    for name, wnt in want.items():
        g = got[name].cpu()
        wt = torch.from_numpy(np.ascontiguousarray(wnt))
        bad = int((g != wt).sum())
        print("renorm-finish %dx%d %s %s: %d of %d differ" % (M, C, state, name, bad, g.numel()))
        assert torch.equal(g, wt), "%s differs from the host restatement at %d elements" % (name, bad)
    assert int(run[3]) == 6
    assert float(count[0]) == (n if masked else -7.0)


# ---------------------------------------------------------------- fused routes against the separate renorm layers

def _norm_set(C, seed, kinds=("warm", "w001", "warm")):
    """three norms' (weight, bias, eps), running and renorm buffers"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, kind in enumerate(kinds):
        w = (torch.rand((C,), generator=g) * 2.0 - 1.0).to(DEV)
        b = (torch.rand((C,), generator=g) - 0.5).to(DEV)
        c = dict(rm=(torch.rand((C,), generator=g) * 0.2 - 0.1).to(DEV), rv=(torch.rand((C,), generator=g) + 0.5).to(DEV))
        out.append(((w, b, EPS), c, _state(kind, C, seed + i)))
    return out


def _same(case, a, b):
    for i, (s, t) in enumerate(zip(a, b)):
        if s is None and t is None:
            continue
        assert torch.equal(s, t), "%s: output %d differs at %d elements" % (case, i, int((s != t).sum()))


@pytest.mark.parametrize("masked", [False, True], ids=["all_live", "masked"])
@pytest.mark.parametrize("form", ["identity", "dual", "identity_dres", "dual_dres", "exit_identity", "exit_dual"])
def test_join_equals_separate_renorm_layers(P, form, masked):
    from wssdl_bus_amd.networks import rownorm
    n_rois, n_slots, C = 37, 16, 512
    M = n_rois * n_slots
    dual, dres, ex = "dual" in form, "dres" in form, "exit" in form
    c, c2 = R.make_case(51, M, C, DEV), R.make_case(52, M, C, DEV)
    x3, other = c["x"], c2["x"]
    mask = R.make_mask("random", n_rois, 5, DEV) if masked else None
    pm = mask is not None
    (bn3, k3, s3), (bns, ks, ss), (bnn, kn, sn) = _norm_set(C, 60)
    # separate fused renorm layers and torch's adds
    bufs = [_buffers(k, s) for k, s in ((k3, s3), (ks, ss), (kn, sn))]
    t3, st3, _ = P.rowbn_forward(x3, *bn3, False, mask, pm, running=bufs[0][0], renorm=bufs[0][1])
    sts = None
    if dual:
        ts, sts, _ = P.rowbn_forward(other, *bns, False, mask, pm, running=bufs[1][0], renorm=bufs[1][1])
    out = t3 + (ts if dual else other)
    y, stn, cnt = P.rowbn_forward(out, *bnn, True, mask, pm, running=bufs[2][0], renorm=bufs[2][1])
    # the join
    jb = [_buffers(k, s) for k, s in ((k3, s3), (ks, ss), (kn, sn))]
    jout, jy, jst3, jsts, jstn, jcnt = P.rowbn_join_forward(
        x3, bn3, other, bns if dual else None, bnn, mask, running=(jb[0][0], jb[1][0] if dual else None, jb[2][0]),
        renorm=(jb[0][1], jb[1][1] if dual else None, jb[2][1]), exit_slots=n_slots if ex else None)
    assert jst3.shape == (7, C)
    _same(form + " forward", (jout, jst3, jstn, jcnt), (out, st3, stn, cnt))
    _same(form + " y", (jy,), (P.slot_mean(y, n_slots) if ex else y,))
    if dual:
        assert torch.equal(jsts, sts)
    for k in (0, 1, 2) if dual else (0, 2):
        _same(form + " buffers of norm %d" % k, jb[k][0][:2] + (jb[k][0][3],) + jb[k][1][:3],
              bufs[k][0][:2] + (bufs[k][0][3],) + bufs[k][1][:3])
        assert not torch.equal(jb[k][1][0], (s3, ss, sn)[k]["mean"]), "norm %d: the state did not move" % k
    if not dual:
        assert torch.equal(jb[1][1][2], ss["weight"]) and int(jb[1][0][3]) == 5     # no shortcut norm: untouched
    # backward
    dy_full = c["dy"]
    dfeat = c2["dy"][:n_rois].contiguous()
    dyy = rownorm._slot_mean_grad(dfeat, n_slots).contiguous() if ex else dy_full
    dr = c["dres"] if dres else None
    dxn, dwn, dbn = P.rowbn_backward(out, dyy, bnn[0], stn, True, mask, pm)
    g = dxn + dr if dres else dxn
    dx3, dw3, db3 = P.rowbn_backward(x3, g, bn3[0], st3, False, mask, pm)
    bits = P.renorm_bits((jb[0][1], jb[1][1] if dual else None, jb[2][1]))
    assert bits == (7 if dual else 5)
    jg, jdx3, jdxs, jdwbn, jdwb3, jdwbs = P.rowbn_join_backward(
        jout, dfeat if ex else dy_full, dr, x3, other if dual else None, bnn[0], jstn, bn3[0], jst3,
        bns[0] if dual else None, jsts if dual else None, mask, exit_slots=n_slots if ex else None, renorm=bits)
    _same(form + " backward", (jg, jdx3, jdwbn[0], jdwbn[1], jdwb3[0], jdwb3[1]), (g, dx3, dwn, dbn, dw3, db3))
    if dual:
        dxs, dws, dbs = P.rowbn_backward(other, g, bns[0], sts, False, mask, pm)
        _same(form + " shortcut backward", (jdxs, jdwbs[0], jdwbs[1]), (dxs, dws, dbs))


@pytest.mark.parametrize("masked", [False, True], ids=["all_live", "masked"])
def test_entry_equals_separate_renorm_layer(P, masked):
    n_rois, C = 37, 256
    plan = P.tap_plan(7, 7, 2)
    per, ns = 49, len(plan.slots)
    c = R.make_case(53, n_rois * per, C, DEV)
    dys = R.make_case(54, ns * n_rois, C, DEV)["dy"]
    possel = plan.subsample_slots(7, 7, 2, c["x"].device)
    mask = R.make_mask("random", n_rois, 6, DEV) if masked else None
    st = _state("warm", C, 8)
    (run_a, ren_a), (run_b, ren_b) = _buffers(c, st), _buffers(c, st)
    y0, st0, cnt0 = P.rowbn_forward(c["x"], c["w"], c["b"], EPS, True, mask, False, running=run_a, renorm=ren_a)
    y, ys, st1, cnt = P.rowbn_forward_entry(c["x"], c["w"], c["b"], EPS, possel, ns, mask, running=run_b, renorm=ren_b)
    sel = (possel >= 0).nonzero().flatten()
    want_ys = torch.empty_like(ys).view(ns, n_rois, C)
    want_ys[possel[sel].long()] = y0.view(n_rois, per, C)[:, sel].transpose(0, 1)
    _same("entry forward", (y, ys, st1, cnt), (y0, want_ys.view(-1, C), st0, cnt0))
    _same("entry buffers", run_b[:2] + (run_b[3],) + ren_b[:3], run_a[:2] + (run_a[3],) + ren_a[:3])
    total = c["dy"].view(n_rois, per, C).clone()
    total[:, sel] += dys.view(ns, n_rois, C)[possel[sel].long()].transpose(0, 1)
    want = P.rowbn_backward(c["x"], total.view(-1, C).contiguous(), c["w"], st0, True, mask, False)
    got = P.rowbn_backward_entry(c["x"], c["dy"], dys, possel, ns, c["w"], st1, mask)
    _same("entry backward", got, want)


@pytest.mark.parametrize("masked", [False, True], ids=["all_live", "masked"])
def test_stats_only_call_feeds_the_patch_gather(P, masked):
    n_rois, C = 37, 256
    plan = P.tap_plan(4, 4, 1)
    c = R.make_case(55, 16 * n_rois, C, DEV)
    mask = R.make_mask("random", n_rois, 7, DEV) if masked else None
    st = _state("warm", C, 10)
    (run_a, ren_a), (run_b, ren_b) = _buffers(c, st), _buffers(c, st)
    y, stats_a, count_a = P.rowbn_forward(c["x"], c["w"], c["b"], EPS, True, mask, True, running=run_a, renorm=ren_a)
    stats_b, count_b = P.rowbn_stats(c["x"], c["w"], c["b"], EPS, mask, True, running=run_b, renorm=ren_b)
    _same("stats-only", (stats_b, count_b), (stats_a, count_a))
    _same("stats-only buffers", run_b[:2] + (run_b[3],) + ren_b[:3], run_a[:2] + (run_a[3],) + ren_a[:3])
    cols_a = P.tap_gather(y, plan, True, n_rois)
    cols_b = P.tap_gather_norm(c["x"], plan, True, n_rois, stats_b[3], stats_b[4], mask)
    assert torch.equal(cols_a, cols_b)


# ---------------------------------------------------------------- the two networks with cfg.TRAIN.USE_BRN = True

@pytest.fixture
def use_brn(monkeypatch):
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.networks import _plumbing
    old = cfg.TRAIN.USE_BRN
    cfg.TRAIN.USE_BRN = True
    monkeypatch.setattr(_plumbing, "TAPS_MIN_ROIS", 1)
    for s in _plumbing.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    cudnn = torch.backends.cudnn
    det = cudnn.deterministic
    cudnn.deterministic = True
    yield
    cudnn.deterministic = det
    cfg.TRAIN.USE_BRN = old


def _two_steps(module, xs, dys, monkeypatch, switches):
    for s in switches:
        monkeypatch.setenv(s, "1")
    outs = []
    try:
        for x, dy in zip(xs, dys):
            module.zero_grad(set_to_none=True)
            p = next(module.parameters())
            xx = x.to(p.device, p.dtype).clone().requires_grad_(True)
            y = module(xx)
            (y * dy.to(y.device, y.dtype)).sum().backward()
            outs.append({k: v.to(DEV) for k, v in NR.module_outputs(module, y, xx).items()})
    finally:
        for s in switches:
            monkeypatch.delenv(s, raising=False)
    return outs


def _judge(case, a, b, s, d):
    """a (fused) == b (unfused switches) bit for bit; a against the stock route by network_reference's criterion"""
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs between the fused and the unfused route" % (case, k)
        if k.endswith("num_batches_tracked"):
            assert int(a[k]) == int(s[k]) == int(d[k]), k
    NR.check_nonzero(d)
    rat = NR.ratios(a, s, d)
    worst = max(rat, key=rat.get)
    print("renorm-netref %s worst %.3f %s" % (case, rat[worst], worst))
    over = {k: round(v, 2) for k, v in rat.items() if not v <= K_NET}
    assert not over, (case, over)
    assert any("renorm_weight" in k for k in a)


def _run_network(make, xs, dys, monkeypatch, unfused, n_joins):
    from wssdl_bus_amd.networks import roi_head
    torch.manual_seed(18)
    a = NR.prepare(make()).cuda()
    b, s = copy.deepcopy(a), copy.deepcopy(a)
    d = copy.deepcopy(a).double().cpu()             # the stock route in f64, on the CPU
    calls = []
    real = roi_head._JoinFn.apply
    monkeypatch.setattr(roi_head._JoinFn, "apply", lambda *args: (calls.append(len(args)), real(*args))[1])
    oa = _two_steps(a, xs, dys, monkeypatch, ())
    assert len(calls) == 2 * n_joins and all(n == 15 for n in calls), calls     # every join, with its renorm state
    ob = _two_steps(b, xs, dys, monkeypatch, unfused)
    assert len(calls) == 2 * n_joins, "the unfused switches still ran the join kernels"
    os_ = _two_steps(s, xs, dys, monkeypatch, ("WSSDL_DISABLE_FUSED_BN",))
    od = _two_steps(d, xs, dys, monkeypatch, ("WSSDL_DISABLE_FUSED_BN",))
    return oa, ob, os_, od


def test_trunk_with_use_brn(P, use_brn, monkeypatch):
    from wssdl_bus_amd.networks import backbones
    g = torch.Generator(device=DEV).manual_seed(7)
    xs = [(torch.randn((2, 3, 64, 96), device=DEV, generator=g) * (1.0 + i) + 0.5 * i).contiguous(
        memory_format=torch.channels_last) for i in range(2)]
    make = lambda: backbones.ResNetTrunk(18).to(memory_format=torch.channels_last)
    probe = make()(xs[0].cpu())
    dys = [torch.randn(probe.shape, device=DEV, generator=g) for _ in range(2)]
    oa, ob, os_, od = _run_network(make, xs, dys, monkeypatch, ("WSSDL_TRUNK_UNFUSED_JOIN",), 6)
    for i in range(2):
        _judge("trunk18 step %d" % (i + 1), oa[i], ob[i], os_[i], od[i])
        assert int(oa[i]["b.norm.num_batches_tracked"]) == i + 1


def test_head_with_use_brn(P, use_brn, monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    g = torch.Generator(device=DEV).manual_seed(8)
    xs = [torch.relu(torch.randn((37, 7, 7, 256), device=DEV, generator=g) * (1.0 + i)).contiguous() for i in range(2)]
    dys = [torch.randn((37, 512), device=DEV, generator=g) for _ in range(2)]
    unfused = ("WSSDL_HEAD_UNFUSED_JOIN", "WSSDL_HEAD_UNFUSED_EXIT", "WSSDL_HEAD_UNFUSED_ENTRY",
               "WSSDL_HEAD_UNFUSED_TAPNORM")
    oa, ob, os_, od = _run_network(lambda: roi_head.ResNetHeadNHWC(18), xs, dys, monkeypatch, unfused, 2)
    for i in range(2):
        _judge("head18 step %d" % (i + 1), oa[i], ob[i], os_[i], od[i])
