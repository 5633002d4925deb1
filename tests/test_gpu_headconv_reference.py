"""-m gpu: the per-RoI head's convolutions (csrc/plumbing/taps.hip and im2col.hip through TapConv3x3Fn, Im2Col3x3Fn,
ConvNHWC.forward and ConvNHWC.forward_pm) against the plain f64 convolution of tests/headconv_reference.py, computed
on the host: every element of y, dx, dW and db inside its bound gamma(n) sum|terms| (counted terms, see that module;
test_headconv_reference_cpu.py shows on the CPU that a model of the class-packed algorithm stays inside the bounds and
that seeded defects miss them at least tenfold).

The route-against-route comparisons of test_gpu_head_taps.py and test_gpu_head_entry.py and their 1e-4 tolerance
stand on this module.  Shapes are the smallest that reach each path of taps.hip (headconv_reference.CASES), one
geometry with asymmetric padding included.  The bounds assume GEMMs that accumulate in f32; test_gemm_* measures that
first, on the cases' own class operands built by plain indexing, with torch.mm / torch.bmm called on the same
transposed views as TapConv3x3Fn calls them.  Position-major tensors are mapped to and from the reference's roi-major
layout with plan.slots, which is checked to be a permutation of all positions; that the two plans of the head agree
on the slot order is what the two-stage test is for.  Two convolutions in a row are judged in stages, as the joins
are in the row batch norm suite: the second against f64 of the kernel's own first output."""
import pytest
import torch

import headconv_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = "cuda"
LOG = {}            # worst |error| / bound per output and route over the module (printed at the end: pytest -s)


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None, "plumbing library not built"
    yield _plumbing
    for k in sorted(LOG):
        print("headconv-worst %s %.4g" % (k, LOG[k]))


def _index(slots, ww):
    n = len(slots)
    assert sorted(slots) == [(y, x) for y in range(n // ww) for x in range(ww)], "slots are no permutation"
    return torch.tensor([y * ww + x for y, x in slots], dtype=torch.long)


def to_pm(t, slots):
    """roi-major [R, hh, ww, ch] -> position-major rows slot * R + roi"""
    R_, hh, ww, ch = t.shape
    assert len(slots) == hh * ww
    idx = _index(slots, ww).to(t.device)
    return t.reshape(R_, hh * ww, ch)[:, idx].transpose(0, 1).reshape(-1, ch).contiguous()


def from_pm(rows, slots, hh, ww):
    """position-major rows -> roi-major [R, hh, ww, ch]: every row lands, none twice"""
    n = hh * ww
    assert len(slots) == n and rows.shape[0] % n == 0
    R_, ch = rows.shape[0] // n, rows.shape[1]
    out = torch.full((R_, n, ch), float("nan"), dtype=rows.dtype, device=rows.device)
    out[:, _index(slots, ww).to(rows.device)] = rows.detach().view(n, R_, ch).transpose(0, 1)
    return out.view(R_, hh, ww, ch)


def _leaf(t):
    return t.to(DEV).clone().requires_grad_(True)


# ---------------------------------------------------------------- 1. the GEMMs themselves

def _gemm_ratio(got, lhs, rhs):
    """f32 product on the device against f64 of the same operands, bound gamma(K) sum|terms|"""
    l64, r64 = lhs.double().cpu(), rhs.double().cpu()
    return R.ratio(got, l64 @ r64, R.gamma(lhs.shape[-1]) * (l64.abs() @ r64.abs()) * R.SLACK)


@pytest.mark.parametrize("pair", R.PAIRS, ids=R.pair_id)
def test_gemm_accumulates_in_f32(pair):
    """torch.mm per class and torch.bmm per group of equal-shape classes, forward, data gradient and weight gradient,
    on the views TapConv3x3Fn hands them.  Measures whether the BLAS solutions torch picks for f32 on this device
    accumulate in plain f32: the premise of every bound below."""
    assert torch.cuda.is_available()
    c = R.make_case(*pair)
    ops = [tuple(t.to(DEV) for t in op) for op in R.class_operands(c)]
    worst = dict(gemm_mm=0.0, gemm_bmm=0.0)
    for a, b, g in ops:
        for got, lhs, rhs in ((torch.mm(a, b.t()), a, b.t()), (torch.mm(g, b), g, b), (torch.mm(g.t(), a), g.t(), a)):
            worst["gemm_mm"] = max(worst["gemm_mm"], _gemm_ratio(got, lhs, rhs))
    k = 0
    while k < len(ops):
        j = k
        while j < len(ops) and ops[j][0].shape == ops[k][0].shape:
            j += 1
        if j - k > 1:
            A, B, G = (torch.stack([op[i] for op in ops[k:j]]) for i in range(3))
            for got, lhs, rhs in ((torch.bmm(A, B.transpose(1, 2)), A, B.transpose(1, 2)), (torch.bmm(G, B), G, B),
                                  (torch.bmm(G.transpose(1, 2), A), G.transpose(1, 2), A)):
                worst["gemm_bmm"] = max(worst["gemm_bmm"], _gemm_ratio(got, lhs, rhs))
        k = j
    R.check_ratios("gemm " + R.pair_id(pair), worst, LOG)


# ---------------------------------------------------------------- 2. the class-packed route

def _run_taps(P, c, plan, in_pm, bias):
    x, W = _leaf(c["x"]), _leaf(c["W"])
    b = _leaf(c["b"]) if bias else None
    src = to_pm(x.detach(), plan.slots).requires_grad_(True) if in_pm else x
    y = P.TapConv3x3Fn.apply(src, W, b, plan, in_pm, c["R"])
    assert y.shape == (plan.oh * plan.ow * c["R"], c["co"])
    y.backward(to_pm(c["dy"].to(DEV), plan.slots))
    dx = from_pm(src.grad, plan.slots, plan.h, plan.w) if in_pm else x.grad
    got = dict(y=from_pm(y, plan.slots, plan.oh, plan.ow), dx=dx, dW=W.grad)
    if bias:
        got["db"] = b.grad
    return got


@pytest.mark.parametrize("pair", R.PAIRS, ids=R.pair_id)
def test_tap_conv_inside_every_bound(P, pair, monkeypatch):
    """TapConv3x3Fn forward and backward from a roi-major input and, where the map keeps its size, from a
    position-major one (its dx comes back position-major and is mapped back like y); with and without bias;
    TAP_GEMM_GROUPED both ways."""
    c = R.make_case(*pair)
    plan = P.tap_plan(c["h"], c["w"], c["s"])
    assert (plan.oh, plan.ow) == (c["oh"], c["ow"])
    for in_pm in ([False, True] if plan.h == plan.oh else [False]):
        for bias in (True, False):
            ref = R.case_reference(pair[0], pair[1], bias)
            for grouped in (True, False):
                monkeypatch.setattr(P, "TAP_GEMM_GROUPED", grouped)
                got = _run_taps(P, c, plan, in_pm, bias)
                case = "%s pm=%d bias=%d grouped=%d" % (R.pair_id(pair), in_pm, bias, grouped)
                R.check_ratios(case, R.ratios(ref, got, prefix="taps_pm_" if in_pm else "taps_"), LOG)


# ---------------------------------------------------------------- 3. the dense route

@pytest.mark.parametrize("pair", [p for p in R.PAIRS if p[0] in ("sharp", "flight")], ids=R.pair_id)
def test_dense_conv_inside_every_bound(P, pair):
    """ConvNHWC.forward on device tensors: Im2Col3x3Fn + F.linear, which multiplies the padding's zeros too"""
    from wssdl_bus_amd.networks import roi_head
    c = R.make_case(*pair)
    conv = roi_head.ConvNHWC(c["C"], c["co"], 3, c["s"], norm=None, relu=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(c["W"])
        conv.bias.copy_(c["b"])
    x = _leaf(c["x"])
    assert P.im2col_usable(x), "the patch kernels would not run"
    y = conv(x)
    y.backward(c["dy"].to(DEV))
    got = dict(y=y, dx=x.grad, dW=conv.weight.grad, db=conv.bias.grad)
    R.check_ratios("dense " + R.pair_id(pair), R.ratios(R.case_reference(*pair), got, dense=True, prefix="dense_"), LOG)


# ---------------------------------------------------------------- 4. two convolutions in a row

def test_two_tap_convs_in_a_row_judged_in_stages(P):
    """(7, 7, 2) from a roi-major input, its position-major output into (4, 4, 1) with in_pm, C = 8 -> 12 -> 8,
    R = 37.  Everything that passes between the stages is un-permuted with the STRIDE-2 plan's slots while the second
    kernel reads it through the STRIDE-1 plan's tables: a disagreement between the two slot orders shows up."""
    c = R.make_case("sharp", (7, 7, 2))
    Rn, C1, C2 = c["R"], c["co"], 8
    p2, p1 = P.tap_plan(7, 7, 2), P.tap_plan(4, 4, 1)
    g = torch.Generator().manual_seed(4242)
    W2 = torch.randn((C2, 9 * C1), generator=g) * 0.1
    b2 = torch.randn((C2,), generator=g) * 0.5 + 1.0
    dy2 = torch.randn((Rn, 4, 4, C2), generator=g) * (0.5 + torch.arange(16.0).view(1, 4, 4, 1) / 16)

    x, W1, b1 = _leaf(c["x"]), _leaf(c["W"]), _leaf(c["b"])
    y1 = P.TapConv3x3Fn.apply(x, W1, b1, p2, False, Rn)
    y1_in, W2d, b2d = y1.detach().clone().requires_grad_(True), _leaf(W2), _leaf(b2)
    y2 = P.TapConv3x3Fn.apply(y1_in, W2d, b2d, p1, True, Rn)
    y2.backward(to_pm(dy2.to(DEV), p1.slots))
    y1.backward(y1_in.grad)

    y1_rm = from_pm(y1, p2.slots, 4, 4).cpu()
    ref2 = R.reference(y1_rm, W2, b2, dy2, 1)
    got2 = dict(y=from_pm(y2, p1.slots, 4, 4), dx=from_pm(y1_in.grad, p2.slots, 4, 4), dW=W2d.grad, db=b2d.grad)
    R.check_ratios("chain stage 2", R.ratios(ref2, got2, prefix="chain2_"), LOG)
    dy1_rm = from_pm(y1_in.grad, p2.slots, 4, 4).cpu()
    ref1 = R.reference(c["x"], c["W"], c["b"], dy1_rm, 2)
    got1 = dict(y=y1_rm, dx=x.grad, dW=W1.grad, db=b1.grad)
    R.check_ratios("chain stage 1", R.ratios(ref1, got1, prefix="chain1_"), LOG)


# ---------------------------------------------------------------- 5. 1x1 at stride 2 on the position-major route

def test_one_by_one_stride_two_position_major(P):
    """ConvNHWC.forward_pm with k = 1, s = 2 on the 7x7 roi-major map (_pm_rows / subsample_index) against the f64
    1x1 stride-2 convolution; the input positions no slot reads have no term and must get an exactly zero dx"""
    from wssdl_bus_amd.networks import roi_head
    c = R.make_case("sharp", (7, 7, 2))
    plan = P.tap_plan(7, 7, 2)
    g = torch.Generator().manual_seed(1111)
    W = torch.randn((c["co"], c["C"]), generator=g) * 0.3
    conv = roi_head.ConvNHWC(c["C"], c["co"], 1, 2, norm=None, relu=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(W)
        conv.bias.copy_(c["b"])
    x = _leaf(c["x"])
    y = conv.forward_pm(x, plan, c["R"])
    assert y.shape == (16 * c["R"], c["co"])
    y.backward(to_pm(c["dy"].to(DEV), plan.slots))
    ref = R.reference(c["x"], W, c["b"], c["dy"], 2, k=1)
    assert int((ref["m_dx"] == 0).sum()) >= (49 - 16) * c["R"] * c["C"]
    got = dict(y=from_pm(y, plan.slots, 4, 4), dx=x.grad, dW=conv.weight.grad, db=conv.bias.grad)
    R.check_ratios("1x1 stride 2", R.ratios(ref, got, prefix="pm1x1_"), LOG)
