"""-m gpu: the two finish kernels of the row batch norm (csrc/plumbing/rowbn.hip: rowbn_fwd_finish_kernel,
rowbn_bwd_finish_kernel) restated on the host, bit for bit.

The exports are called through ctypes with a workspace tensor of the test's own.  After a call the workspace still
holds the f64 partial sums [nb, 2C] the slab kernel left for the finish kernel (nothing after it writes there), so the
test reads them back and redoes the finish in numpy float64, in the documented order and with the documented formulas:

  sums     64 groups; group g adds the partials g, g + 64, g + 128, ... in that order into 0.0; then the 64 group sums
           are added in order into 0.0
  rows     n = M, or max(per * (number of live RoIs), 1) with a mask            (count[0] = (float)n)
  forward  mu = s / n;  v = max(fma(-mu, mu, q / n), 0);  rstd = (float)(1 / sqrt(v + eps));  scale = rstd * w (f32);
           mean = (float)mu;  var = (float)v;  shift = fmaf(-scale, mean, bias)
           running <- (float)(r + mom * (stat * unbias - r)), every f64 operation rounded on its own,
           unbias = 1 for the mean, n / max(n - 1, 1) for the variance
  backward t = fma(-mu, sg, sgx) * rstd;  a = w * rstd;  k1 = a * rstd * t / n;  k0 = fma(-k1, mu, a * sg / n);
           dweight = (float)t;  dbias = (float)sg;  coef = (float)(a, k0, k1)

Every fused multiply-add is evaluated exactly (fractions) and rounded once.  All comparisons are torch.equal.

Shapes: C = 4 (one finish workgroup with 12 idle columns), 32 (two workgroups), 1024; M such that the number of
partial blocks nb = min(1024, ceil(M / (16 * RS))) is 1, 63, 64, 65 and 1024 (one partial, one short of / exactly / one
more than the 64 groups, every thread's 16 steps).  Masks: n_rois = 1, 1023, 1024, 1025, 3000 (the live-row count's
loop: one entry, one short of / exactly / one more than a workgroup's threads, several trips) with no, some and all
RoIs dead (all dead: the clamp to 1), roi-major and position-major."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK, MAX_PARTIAL_BLOCKS, FIN_GROUPS = 256, 1024, 64
EPS, MOM = 1e-3, 0.01


@pytest.fixture(scope="module")
def plumbing():
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None, "plumbing library not built"
    return _plumbing


def _geometry(M, C):
    L = min(C // 4, BLOCK)
    RS = BLOCK // L
    return RS, min(MAX_PARTIAL_BLOCKS, max(1, -(-M // (16 * RS))))


def _rows_for(nb, C):
    """an M (not a multiple of the slab height) that gives nb partial blocks"""
    RS, _ = _geometry(1, C)
    M = 16 * RS * nb - min(5, 16 * RS - 1)
    assert _geometry(M, C)[1] == nb
    return M


# ---------------------------------------------------------------- host arithmetic

def _fma64(a, b, c):
    """fl64(a * b + c), the exact value rounded once (Fraction -> float is correctly rounded)"""
    return np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], dtype=np.float64)


def _round_f32(fr):
    """a Fraction rounded to the nearest f32 (ties to even; normal range)"""
    if fr == 0:
        return np.float32(0.0)
    e = math.frexp(abs(float(fr)))[1]
    scaled = abs(fr) * Fraction(2) ** (24 - e)
    if scaled < 2 ** 23:                        # float() rounded up across a power of two
        e -= 1
        scaled *= 2
    n = round(scaled)                           # half to even
    return np.float32(math.copysign(math.ldexp(float(n), e - 24), float(fr)))


def _fma32(a, b, c):
    return np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], dtype=np.float32)


def _finish_sums(P):
    """The finish kernels' fixed order over the partials P [nb, 2C]: (s [C], q [C])."""
    nb, C2 = P.shape
    red = np.zeros((FIN_GROUPS, C2), dtype=np.float64)
    for k in range(MAX_PARTIAL_BLOCKS // FIN_GROUPS):
        b = np.arange(FIN_GROUPS) + k * FIN_GROUPS
        on = b < nb
        red[on] = red[on] + P[b[on]]
    tot = np.zeros((C2,), dtype=np.float64)
    for g in range(FIN_GROUPS):
        tot = tot + red[g]
    return tot[:C2 // 2], tot[C2 // 2:]


def _rows(M, mask, per):
    if mask is None:
        return float(M)
    return max(float(per) * float(int((mask != 0).sum())), 1.0)


def _running(r, stat, unbias, mom):
    t = stat.astype(np.float64) * unbias
    d = t - r.astype(np.float64)
    p = mom * d
    return (r.astype(np.float64) + p).astype(np.float32)


def _host_forward(P, n, w, b, rm, rv):
    s, q = _finish_sums(P)
    mu = s / n
    v = _fma64(-mu, mu, q / n)
    v = np.where(v < 0.0, 0.0, v)
    eps = float(np.float32(EPS))
    rstd = (1.0 / np.sqrt(v + eps)).astype(np.float32)
    scale = rstd * w
    mean, var = mu.astype(np.float32), v.astype(np.float32)
    shift = _fma32(-scale, mean, b)
    mom = float(np.float32(MOM))
    return dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift,
                rm=_running(rm, mean, 1.0, mom), rv=_running(rv, var, n / max(n - 1.0, 1.0), mom))


def _host_backward(P, n, w, mean, rstd):
    sg, sgx = _finish_sums(P)
    mu, rs, w = mean.astype(np.float64), rstd.astype(np.float64), w.astype(np.float64)
    t = _fma64(-mu, sg, sgx) * rs
    a = w * rs
    k1 = a * rs * t / n
    k0 = _fma64(-k1, mu, a * sg / n)
    return dict(dweight=t.astype(np.float32), dbias=sg.astype(np.float32),
                coef=np.stack([a, k0, k1]).astype(np.float32))


# ---------------------------------------------------------------- the calls

def _inputs(M, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.rand(shape, device="cuda", generator=g)
    mu, sd = r(C) * 8.0 - 4.0, r(C) * 3.0 + 0.05
    x = torch.randn((M, C), device="cuda", generator=g) * sd + mu
    dy = torch.randn((M, C), device="cuda", generator=g) * (r(C) * 4.0 + 0.1)
    return dict(x=x, dy=dy, w=r(C) * 3.0 - 1.5, b=r(C) - 0.5, rm=r(C) * 0.2 - 0.1, rv=r(C) * 1.5 + 0.5)


def _partials(ws, nb, C):
    return ws[:nb * 2 * C * 8].view(torch.float64).view(nb, 2 * C).cpu().numpy().copy()


def _same(case, name, got, want):
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    bad = int((got != want).sum())
    print("finish %s %s: %d of %d elements differ" % (case, name, bad, got.numel()))
    assert torch.equal(got, want), "%s: %s differs from the host restatement at %d elements" % (case, name, bad)


def _run(P, case, M, C, mask, per, pos_major, relu, seed):
    nb = _geometry(M, C)[1]
    c = _inputs(M, C, seed)
    x, w, b = c["x"], c["w"], c["b"]
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    n = _rows(M, mask, per)
    n_rois = mask.shape[0] if mask is not None else 0
    margs = (P._p(mask) if mask is not None else None, n_rois, per if mask is not None else 1)
    nbytes = P.lib().wsplumb_rowbn_workspace_bytes(M, C)
    assert nbytes == nb * 2 * C * 8
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")

    # forward
    y, stats, count = f32(M, C), f32(5, C), torch.full((1,), -7.0, device="cuda")
    rm, rv, nbt = c["rm"].clone(), c["rv"].clone(), torch.full((1,), 5, dtype=torch.int64, device="cuda")
    P._call("wsplumb_rowbn_forward", x.device, P._p(x), M, C, P._p(w), P._p(b), EPS, int(relu), *margs,
            int(pos_major), P._p(y), *[P._p(stats[i]) for i in range(5)], P._p(count), P._p(ws), ws.numel(),
            tail=(P._p(rm), P._p(rv), MOM, P._p(nbt)))
    torch.cuda.synchronize()
    want = _host_forward(_partials(ws, nb, C), n, w.cpu().numpy(), b.cpu().numpy(), c["rm"].cpu().numpy(),
                         c["rv"].cpu().numpy())
    for i, name in enumerate(("mean", "var", "rstd", "scale", "shift")):
        _same(case, name, stats[i], want[name])
    if mask is not None:
        _same(case, "count", count, np.array([n], dtype=np.float32))
    else:
        assert float(count[0]) == -7.0, "%s: count written without a mask" % case
    _same(case, "running_mean", rm, want["rm"])
    _same(case, "running_var", rv, want["rv"])
    assert int(nbt[0]) == 6, "%s: num_batches_tracked advanced by %d" % (case, int(nbt[0]) - 5)

    # backward, from the forward's own f32 statistics
    dx, dwb, coef = f32(M, C), f32(2, C), f32(3, C)
    ws.zero_()
    P._call("wsplumb_rowbn_backward", x.device, P._p(x), P._p(c["dy"]), M, C, P._p(w), P._p(stats[0]), P._p(stats[2]),
            P._p(stats[3]), P._p(stats[4]), int(relu), *margs, int(pos_major), P._p(dx), P._p(dwb[0]), P._p(dwb[1]),
            P._p(coef), P._p(ws), ws.numel())
    torch.cuda.synchronize()
    wantb = _host_backward(_partials(ws, nb, C), n, w.cpu().numpy(), stats[0].cpu().numpy(), stats[2].cpu().numpy())
    _same(case, "dweight", dwb[0], wantb["dweight"])
    _same(case, "dbias", dwb[1], wantb["dbias"])
    _same(case, "coef", coef, wantb["coef"])


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 1024])
@pytest.mark.parametrize("C", [4, 32, 1024])
def test_finish_block_counts(plumbing, C, nb):
    M = _rows_for(nb, C)
    _run(plumbing, "C=%d nb=%d M=%d" % (C, nb, M), M, C, None, 1, False, relu=bool(nb & 1), seed=17 * C + nb)


def _mask(kind, n_rois, seed):
    if kind == "none_dead":
        m = torch.ones((n_rois,))
    elif kind == "all_dead":
        m = torch.zeros((n_rois,))
    else:
        m = (torch.rand((n_rois,), generator=torch.Generator().manual_seed(seed)) > 0.3).float()
        m[-1] = 0.0
        m[0] = 1.0                  # (n_rois = 1: one live RoI)
    return m.cuda()


@pytest.mark.parametrize("pos_major", [False, True], ids=["roi_major", "pos_major"])
@pytest.mark.parametrize("kind", ["none_dead", "some_dead", "all_dead"])
@pytest.mark.parametrize("n_rois", [1, 1023, 1024, 1025, 3000])
def test_finish_live_row_count(plumbing, n_rois, kind, pos_major):
    per, C = 4, 32
    mask = _mask(kind, n_rois, n_rois)
    _run(plumbing, "n_rois=%d %s %s" % (n_rois, kind, "pm" if pos_major else "rm"), n_rois * per, C, mask, per,
         pos_major, relu=True, seed=n_rois)


def test_finish_masked_wide(plumbing):
    """C = 1024 (64 finish workgroups, each counting the live RoIs on its own) with 1025 RoIs of 16 position-major rows"""
    n_rois, per, C = 1025, 16, 1024
    _run(plumbing, "wide n_rois=%d" % n_rois, n_rois * per, C, _mask("some_dead", n_rois, 3), per, True, relu=True,
         seed=5)
