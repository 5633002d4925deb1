"""-m gpu: the head's exit inside the last join (csrc/plumbing/rowbn.hip: rowbn_slot_mean_kernel, DY_EXIT;
networks/rownorm.py: _JoinFn's exit form, _SlotMeanFn) and block 1's shortcut rows from the entry norm's apply pass
(EntryRows; _EntryNormFn).

The exit.  The plain join writes y = relu(bn_n(out)) [n_slots * R, C]; the head then only averages y over the slots.
The exit form writes feat [R, C] instead.  THE ORDER of the mean (csrc/plumbing/bn_math.hip.h): the slots in slot
order in chunks of 16, a balanced binary tree over a chunk's 16 places (+0 in a place past the last slot, which cannot
change a sum of values >= +0), the chunk sums added in order, the total times the f32 quotient 1 / n_slots.  For 16
(4) slots every addend goes through 4 (2) additions and the one multiplication: ROUNDINGS = log2(n_slots) + 1 = 5 (3)
roundings, each at most 2^-24 relative, and every term is >= 0 (ReLU outputs), so
    |feat - mean64| <= ROUNDINGS * 2^-24 * mean64
with mean64 the f64 mean of the same f32 values.  (The multiplication is exact for these counts; it is counted anyway,
which also covers the second-order terms of the four additions.)
  * feat is torch.equal to wsplumb_slot_mean of the y the plain join writes, and within that bound of mean64;
  * the backward fed dfeat equals, bit for bit, the plain backward fed dfeat * (1 / n_slots) repeated over the slots --
    g, dx3, both parameter-gradient blocks.  1 / n_slots is exact for 4 and 16; nothing is claimed for other counts.
The head: output, input gradient, every parameter gradient and every buffer are torch.equal between the default route
and WSSDL_HEAD_UNFUSED_EXIT=1, with three _JoinFn calls in both.

The entry.  ys is torch.equal to _pm_rows(y), with and without dead RoIs (tests/test_gpu_head_entry.py holds the head
to its WSSDL_HEAD_UNFUSED_ENTRY=1 route; it is repeated here at one size for the forward's new kernel)."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None, "plumbing library not built"
    return _plumbing


def _mask(kind, R, n_slots, C, g):
    """None; scattered dead RoIs; or a dead run that crosses a boundary between two row slabs of the partial kernels
    (position-major rows: slab b holds the rows [b * rpb, (b + 1) * rpb), row r belongs to RoI r % R)."""
    if kind == "none":
        return None
    if kind == "scattered":
        m = (torch.rand((R,), device="cuda", generator=g) > 0.3).float()
        m[0] = 1.0
        if R > 2:
            m[R // 2] = 0.0
        return m
    M = n_slots * R
    L = min(C // 4, 256)
    nb = min(1024, max(1, -(-M // (16 * (256 // L)))))
    rpb = -(-M // nb)
    edge = rpb % R if nb > 1 else R // 2                   # the RoI of the first row of slab 1
    m = torch.ones((R,), device="cuda")
    m[max(edge - 2, 0):edge + 3] = 0.0
    if not bool(m.any()):
        m[-1] = 1.0                                        # (R = 1: nothing to kill)
    return m


def _bn(C, g):
    w = torch.rand((C,), device="cuda", generator=g) + 0.5
    b = torch.rand((C,), device="cuda", generator=g) * 0.4 - 0.2
    return w, b, 1e-3


@pytest.mark.parametrize("mask_kind", ["none", "scattered", "dead_run"])
@pytest.mark.parametrize("R", [1, 37, 259])
@pytest.mark.parametrize("n_slots", [16, 4])
@pytest.mark.parametrize("C", [64, 2048])
def test_exit_join_equals_plain_join_and_slot_mean(P, C, n_slots, R, mask_kind):
    g = torch.Generator(device="cuda").manual_seed(C + 31 * n_slots + R)
    M = n_slots * R
    mask = _mask(mask_kind, R, n_slots, C, g)
    x3 = torch.randn((M, C), device="cuda", generator=g)
    other = torch.randn((M, C), device="cuda", generator=g) * 1.5 + 0.3
    bn3, bnn = _bn(C, g), _bn(C, g)
    dfeat = torch.randn((R, C), device="cuda", generator=g)

    out, y, st3, _, stn, cnt = P.rowbn_join_forward(x3, bn3, other, None, bnn, mask)
    eout, feat, est3, _, estn, ecnt = P.rowbn_join_forward(x3, bn3, other, None, bnn, mask, exit_slots=n_slots)
    torch.cuda.synchronize()
    assert feat.shape == (R, C)
    assert torch.equal(eout, out) and torch.equal(est3, st3) and torch.equal(estn, stn)
    if mask is not None:
        assert torch.equal(ecnt, cnt)
        assert not bool(feat[mask == 0].any()), "the row of a dead RoI is not zero"

    want = P.slot_mean(y, n_slots)
    assert torch.equal(feat, want), "feat differs from wsplumb_slot_mean(y): max |d| = %g" % float((feat - want).abs().max())
    ROUNDINGS = int(math.log2(n_slots)) + 1                # the tree's additions on an addend's path + the scaling
    mean64 = y.double().view(n_slots, R, C).mean(0)
    assert float(y.min()) >= 0.0
    err, bound = (feat.double() - mean64).abs(), ROUNDINGS * 2.0 ** -24 * mean64
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("exit C=%d n_slots=%d R=%d %s: worst |feat - mean64| / bound = %.4g" % (C, n_slots, R, mask_kind, worst))
    assert bool((err <= bound).all()), worst

    # backward: dfeat into the exit form against the materialised gradient into the plain form
    dy = (dfeat * (1.0 / n_slots)).repeat(n_slots, 1)
    assert torch.equal(dy * n_slots, dfeat.repeat(n_slots, 1))            # the reciprocal is exact
    pg, pdx3, _, pdwbn, pdwb3, _ = P.rowbn_join_backward(out, dy, None, x3, None, bnn[0], stn, bn3[0], st3, None, None,
                                                         mask)
    eg, edx3, _, edwbn, edwb3, _ = P.rowbn_join_backward(eout, dfeat, None, x3, None, bnn[0], estn, bn3[0], est3, None,
                                                         None, mask, exit_slots=n_slots)
    torch.cuda.synchronize()
    for name, a, b in (("g", eg, pg), ("dx3", edx3, pdx3), ("dwb_n", edwbn, pdwbn), ("dwb3", edwb3, pdwb3)):
        assert torch.equal(a, b), "%s differs: max |d| = %g" % (name, float((a - b).abs().max()))


def test_exit_join_dual_form(P):
    """the projection-shortcut form of the exit (a head whose group is a single block), at one size"""
    C, n_slots, R = 256, 16, 37
    g = torch.Generator(device="cuda").manual_seed(9)
    M = n_slots * R
    mask = _mask("scattered", R, n_slots, C, g)
    x3, xs = torch.randn((M, C), device="cuda", generator=g), torch.randn((M, C), device="cuda", generator=g)
    bn3, bns, bnn = _bn(C, g), _bn(C, g), _bn(C, g)
    dfeat = torch.randn((R, C), device="cuda", generator=g)
    out, y, st3, sts, stn, _ = P.rowbn_join_forward(x3, bn3, xs, bns, bnn, mask)
    eout, feat, est3, ests, estn, _ = P.rowbn_join_forward(x3, bn3, xs, bns, bnn, mask, exit_slots=n_slots)
    assert torch.equal(eout, out) and torch.equal(feat, P.slot_mean(y, n_slots))
    dy = (dfeat * (1.0 / n_slots)).repeat(n_slots, 1)
    plain = P.rowbn_join_backward(out, dy, None, x3, xs, bnn[0], stn, bn3[0], st3, bns[0], sts, mask)
    ex = P.rowbn_join_backward(eout, dfeat, None, x3, xs, bnn[0], estn, bn3[0], est3, bns[0], ests, mask,
                               exit_slots=n_slots)
    for a, b in zip(ex, plain):
        assert torch.equal(a, b)


def test_slot_mean_function_gradient(P):
    """_SlotMeanFn's backward: dfeat * (1 / n_slots) for every slot"""
    from wssdl_bus_amd.networks import rownorm
    g = torch.Generator(device="cuda").manual_seed(2)
    y = torch.rand((16 * 5, 64), device="cuda", generator=g).requires_grad_(True)
    feat = rownorm._SlotMeanFn.apply(y, 16)
    d = torch.randn((5, 64), device="cuda", generator=g)
    feat.backward(d)
    assert torch.equal(y.grad, (d / 16).repeat(16, 1))
    # against torch's own f32 mean: 5 roundings here, at most 16 there, every term >= 0
    assert torch.allclose(feat, y.detach().view(16, 5, 64).mean(0), rtol=21 * 2.0 ** -24, atol=0)


# ---------------------------------------------------------------- the head

def _head(depth=50):
    from wssdl_bus_amd.networks import roi_head
    torch.manual_seed(depth)
    a = roi_head.ResNetHeadNHWC(depth).cuda()
    with torch.no_grad():
        for m in a.modules():
            if isinstance(m, roi_head.RowBatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    return a


def _run_head(head, x, mask, switch, on, monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    if on:
        monkeypatch.setenv(switch, "1")
    else:
        monkeypatch.delenv(switch, raising=False)
    xx = x.clone().requires_grad_(True)
    roi_head.set_roi_mask(mask)
    try:
        y = head(xx)
    finally:
        roi_head.set_roi_mask(None)
    return xx, y


def _compare_heads(switch, R, mode, monkeypatch, joins=None):
    from wssdl_bus_amd.networks import _plumbing, roi_head
    if R < _plumbing.TAPS_MIN_ROIS:
        monkeypatch.setattr(_plumbing, "TAPS_MIN_ROIS", 1)
    for s in ("WSSDL_HEAD_DENSE_3X3", "WSSDL_HEAD_UNFUSED_JOIN", "WSSDL_HEAD_UNFUSED_ENTRY", "WSSDL_HEAD_UNFUSED_EXIT"):
        monkeypatch.delenv(s, raising=False)
    a = _head()
    b = copy.deepcopy(a)
    g = torch.Generator(device="cuda").manual_seed(R)
    x = torch.relu(torch.randn((R, 7, 7, 1024), device="cuda", generator=g))
    assert a._tap_plans(x) is not None
    mask = None
    if mode == "masked":
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.25).float()
        mask[R // 20:R // 20 + R // 3] = 0.0
        mask[0] = 1.0
        x = x * mask.view(-1, 1, 1, 1)
    calls = []
    real = roi_head._JoinFn.apply
    monkeypatch.setattr(roi_head._JoinFn, "apply", lambda *args: (calls.append(args), real(*args))[1])
    xa, ya = _run_head(a, x, mask, switch, False, monkeypatch)
    n_a = len(calls)
    xb, yb = _run_head(b, x, mask, switch, True, monkeypatch)
    if joins is not None:
        assert (n_a, len(calls) - n_a) == (joins, joins), (n_a, len(calls) - n_a)
    assert ya.shape == (R, 2048) and torch.equal(ya, yb), float((ya - yb).abs().max())
    dy = torch.randn(ya.shape, device="cuda", generator=g)
    if mask is not None:
        dy = dy * mask.unsqueeze(1)
    ya.backward(dy)
    yb.backward(dy)
    assert torch.equal(xa.grad, xb.grad)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pa.grad is not None and pb.grad is not None, k
        assert torch.equal(pa.grad, pb.grad), k
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(ba, bb), k
    return calls, n_a


@pytest.mark.parametrize("mode", ["train", "masked"])
@pytest.mark.parametrize("R", [37, 2051])
def test_head_exit_equals_unfused_exit(P, R, mode, monkeypatch):
    calls, n_a = _compare_heads("WSSDL_HEAD_UNFUSED_EXIT", R, mode, monkeypatch, joins=3)
    # the default route's last join took the exit form (a trailing n_slots), the switch's did not
    assert len(calls[n_a - 1]) == 14 and calls[n_a - 1][13] == 16
    assert all(len(c) == 13 for c in calls[:n_a - 1] + calls[n_a:])
    assert "WSSDL_HEAD_UNFUSED_EXIT" in P.SWITCHES


# ---------------------------------------------------------------- the entry

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("R,C", [(37, 64), (259, 1024)])
def test_entry_rows_equal_index_select(P, R, C, masked):
    from wssdl_bus_amd.networks import rownorm
    g = torch.Generator(device="cuda").manual_seed(R + C + masked)
    h = w = 7
    plan = P.tap_plan(h, w, 2)
    x = torch.randn((R * h * w, C), device="cuda", generator=g)
    wt, b, eps = _bn(C, g)
    mask = None
    if masked:
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.3).float()
        mask[0], mask[-1] = 1.0, 0.0
    y0, st0, cnt0 = P.rowbn_forward(x, wt, b, eps, True, mask, False)
    y, ys, st, cnt = P.rowbn_forward_entry(x, wt, b, eps, plan.subsample_slots(h, w, 2, x.device), len(plan.slots), mask)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(st, st0) and (mask is None or torch.equal(cnt, cnt0))
    want = rownorm._pm_rows(y0.view(R, h, w, C), plan, 2)
    assert ys.shape == want.shape == (len(plan.slots) * R, C)
    assert torch.equal(ys, want), float((ys - want).abs().max())
    if masked:
        assert not bool(ys.view(-1, R, C)[:, mask == 0].any())


def test_head_entry_equals_unfused_entry(P, monkeypatch):
    _compare_heads("WSSDL_HEAD_UNFUSED_ENTRY", 37, "masked", monkeypatch)
