"""-m gpu: the per-RoI head's 3x3 convolutions over their valid taps only (csrc/plumbing/taps.hip,
networks/_plumbing.py: TapPlan / TapConv3x3Fn, networks/roi_head.py: the position-major 4x4 section).
Kernels against the dense patch route (im2col.hip) they replace; the head against its dense route
(WSSDL_HEAD_DENSE_3X3=1).

These route-against-route comparisons and their 1e-4 tolerance stand on test_gpu_headconv_reference.py, which holds
both routes to a plain f64 convolution element by element, within bounds counted from the arithmetic."""
import copy

import pytest

pytestmark = pytest.mark.gpu

GEOMS = [(7, 7, 2), (4, 4, 1)]          # the two shapes the head runs: 7x7 -> 4x4 at stride 2, 4x4 -> 4x4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None
    return torch


@pytest.fixture(autouse=True)
def taps_at_any_r(monkeypatch):
    """The head takes the class-packed route from _plumbing.TAPS_MIN_ROIS RoIs on; here at every R."""
    from wssdl_bus_amd.networks import _plumbing
    monkeypatch.setattr(_plumbing, "TAPS_MIN_ROIS", 1)


def _pack_index(torch, plan, R):
    """Indices into the dense patches viewed as [R, oh*ow, 9] units, in class-packed order."""
    idx = []
    for taps, poss in plan.classes:
        for (y, x) in poss:
            p = y * plan.ow + x
            for r in range(R):
                idx.extend((r * plan.oh * plan.ow + p) * 9 + t for t in taps)
    return torch.tensor(idx, dtype=torch.long, device="cuda")


def _to_pm(x, plan):
    """roi-major [R, h, w, C] -> position-major rows in the plan's slot order (h = oh)."""
    R, h, w, C = x.shape
    return x.reshape(R, h * w, C)[:, [y * w + xx for y, xx in plan.slots]].transpose(0, 1).reshape(-1, C).contiguous()


def _dense(torch, x, plan):
    from wssdl_bus_amd.networks import _plumbing
    return _plumbing.Im2Col3x3Fn.apply(x, plan.s, plan.oh, plan.ow, plan.pt, plan.pl)


@pytest.mark.parametrize("h,w,s", GEOMS)
@pytest.mark.parametrize("R,C", [(5, 64), (37, 512)])
def test_gather_equals_dense_im2col_without_padding_columns(torch_cuda, h, w, s, R, C):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    plan = _plumbing.tap_plan(h, w, s)
    g = torch.Generator(device="cuda").manual_seed(h * 10 + R)
    x = torch.randn((R, h, w, C), device="cuda", generator=g)
    want = _dense(torch, x, plan).view(-1, C)[_pack_index(torch, plan, R)].reshape(-1)
    got = _plumbing.tap_gather(x, plan, False, R)
    assert got.shape == want.shape and torch.equal(got, want)
    if plan.h == plan.oh:                                   # position-major source (blocks 2 and 3)
        got_pm = _plumbing.tap_gather(_to_pm(x, plan), plan, True, R)
        assert torch.equal(got_pm, want)


@pytest.mark.parametrize("h,w,s", GEOMS)
@pytest.mark.parametrize("R,C", [(5, 64), (37, 512)])
def test_col2im_equals_dense_col2im_with_zero_padding_columns(torch_cuda, h, w, s, R, C):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    plan = _plumbing.tap_plan(h, w, s)
    g = torch.Generator(device="cuda").manual_seed(100 + h * 10 + R)
    packed = torch.randn((plan.units * R * C,), device="cuda", generator=g)
    dense = torch.zeros((R * plan.oh * plan.ow * 9, C), device="cuda")
    dense[_pack_index(torch, plan, R)] = packed.view(-1, C)
    x = torch.zeros((R, h, w, C), device="cuda", requires_grad=True)
    _dense(torch, x, plan).backward(dense.view(R * plan.oh * plan.ow, 9 * C))
    want = x.grad
    got = _plumbing.tap_col2im(packed, plan, False, R, C)
    assert torch.equal(got, want)
    if plan.h == plan.oh:
        got_pm = _plumbing.tap_col2im(packed, plan, True, R, C)
        assert torch.equal(got_pm, _to_pm(want, plan))


@pytest.mark.parametrize("h,w,s", GEOMS)
def test_weight_gather_and_scatter(torch_cuda, h, w, s):
    """The packed weight is a copy of the class columns; the dW scatter of the class GEMMs' wgrads equals
    the dense wgrad (f32 reordering), and the weight scatter is the exact adjoint of the gather on a
    one-class-per-tap input."""
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    plan = _plumbing.tap_plan(h, w, s)
    g = torch.Generator(device="cuda").manual_seed(7)
    CO, C, R = 96, 128, 211
    W = torch.randn((CO, 9 * C), device="cuda", generator=g)
    wp = _plumbing.tap_weight_gather(W, plan)
    off = 0
    for taps, _ in plan.classes:
        n = CO * len(taps) * C
        want = W.view(CO, 9, C)[:, taps].reshape(-1)
        assert torch.equal(wp[off:off + n], want)
        off += n
    # scatter: dense wgrad of a random dy against the class-packed one
    x = torch.randn((R, h, w, C), device="cuda", generator=g)
    dy = torch.randn((R * plan.oh * plan.ow, CO), device="cuda", generator=g)
    cols = _dense(torch, x, plan)
    want = dy.t() @ cols
    dy_pm = dy.view(R, plan.oh * plan.ow, CO)[:, [y * plan.ow + xx for y, xx in plan.slots]].transpose(0, 1)
    dy_pm = dy_pm.reshape(-1, CO).contiguous()
    xr = x.clone().requires_grad_(False)
    Wr = W.clone().requires_grad_(True)
    _plumbing.TapConv3x3Fn.apply(xr, Wr, None, plan, False, R).backward(dy_pm)
    err = float((Wr.grad - want).abs().max())
    assert err <= 1e-4 * float(want.abs().max()), err
    # exactness of the scatter's fixed order: only one class holds each tap's column where it is non-zero
    dwp = torch.zeros_like(wp)
    off = 0
    for k, (taps, _) in enumerate(plan.classes):
        n = CO * len(taps) * C
        if k == 0:
            dwp[off:off + n] = wp[off:off + n]
        off += n
    centre = plan.classes[0][0]
    got = _plumbing.tap_weight_scatter(dwp, plan, CO, C).view(CO, 9, C)
    assert torch.equal(got[:, centre], W.view(CO, 9, C)[:, centre])


@pytest.mark.parametrize("h,w,s", GEOMS)
@pytest.mark.parametrize("grouped", [True, False])
def test_tap_conv_matches_dense_conv(torch_cuda, h, w, s, grouped, monkeypatch):
    torch = torch_cuda
    import torch.nn.functional as F
    from wssdl_bus_amd.networks import _plumbing
    monkeypatch.setattr(_plumbing, "TAP_GEMM_GROUPED", grouped)
    plan = _plumbing.tap_plan(h, w, s)
    g = torch.Generator(device="cuda").manual_seed(11)
    R, C, CO = 300, 256, 128
    x = torch.randn((R, h, w, C), device="cuda", generator=g)
    W = torch.randn((CO, 9 * C), device="cuda", generator=g) * 0.05
    b = torch.randn((CO,), device="cuda", generator=g)
    xa, Wa, ba = (t.clone().requires_grad_(True) for t in (x, W, b))
    xb, Wb, bb = (t.clone().requires_grad_(True) for t in (x, W, b))
    ya = F.linear(_dense(torch, xa, plan), Wa, ba)                  # [R*oh*ow, CO] roi-major
    src = _to_pm(xb, plan) if plan.h == plan.oh else xb
    yb = _plumbing.TapConv3x3Fn.apply(src, Wb, bb, plan, plan.h == plan.oh, R)
    ya_pm = ya.view(R, -1, CO)[:, [y * plan.ow + xx for y, xx in plan.slots]].transpose(0, 1).reshape(-1, CO)
    _close(torch, yb, ya_pm)
    d = torch.randn(yb.shape, device="cuda", generator=g)
    yb.backward(d)
    ya_pm.backward(d)
    for a, bref in ((xb.grad, xa.grad), (Wb.grad, Wa.grad), (bb.grad, ba.grad)):
        _close(torch, a, bref)


def _close(torch, a, b, rel=1e-4):
    assert a.shape == b.shape
    err = float((a - b).abs().max())
    assert err <= rel * max(float(b.abs().max()), 1e-30), (err, float(b.abs().max()))


def test_position_major_masked_batch_norm(torch_cuda):
    """wsplumb_rowbn_forward / _backward with a mask and pos_major on position-major rows = the same exports
    without pos_major on the same rows reordered (same statistics, same outputs and gradients)."""
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    g = torch.Generator(device="cuda").manual_seed(5)
    R, P, C = 93, 16, 512
    x = torch.randn((R, P, C), device="cuda", generator=g)
    dy = torch.randn((R, P, C), device="cuda", generator=g)
    mask = (torch.rand((R,), device="cuda", generator=g) > 0.3).float()
    w = torch.rand((C,), device="cuda", generator=g) + 0.5
    bias = torch.randn((C,), device="cuda", generator=g)
    for relu in (False, True):
        ya, sa, ca = _plumbing.rowbn_forward(x.reshape(-1, C), w, bias, 1e-3, relu, mask)
        xp = x.transpose(0, 1).reshape(-1, C).contiguous()
        yb, sb, cb = _plumbing.rowbn_forward(xp, w, bias, 1e-3, relu, mask, pos_major=True)
        assert torch.equal(ca, cb)
        _close(torch, sb, sa, 1e-6)
        _close(torch, yb, ya.view(R, P, C).transpose(0, 1).reshape(-1, C), 1e-5)
        assert not bool(yb.view(P, R, C)[:, mask == 0].any())
        dxa, dwa, dba = _plumbing.rowbn_backward(x.reshape(-1, C), dy.reshape(-1, C), w, sa, relu, mask)
        dyp = dy.transpose(0, 1).reshape(-1, C).contiguous()
        dxb, dwb, dbb = _plumbing.rowbn_backward(xp, dyp, w, sb, relu, mask, pos_major=True)
        _close(torch, dxb, dxa.view(R, P, C).transpose(0, 1).reshape(-1, C), 1e-5)
        _close(torch, dwb, dwa, 1e-5)
        _close(torch, dbb, dba, 1e-5)


def _run_head(torch, head, x, mask=None, dense=False, monkeypatch=None, grad=True):
    from wssdl_bus_amd.networks import roi_head
    if dense:
        monkeypatch.setenv("WSSDL_HEAD_DENSE_3X3", "1")
    else:
        monkeypatch.delenv("WSSDL_HEAD_DENSE_3X3", raising=False)
    xx = x.clone().requires_grad_(grad)
    roi_head.set_roi_mask(mask)
    try:
        y = head(xx)
    finally:
        roi_head.set_roi_mask(None)
    return xx, y


def _compare_heads(torch, depth, R, mode, monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    torch.manual_seed(depth + R)
    a = roi_head.ResNetHeadNHWC(depth).cuda()
    e = a.group3[0].expansion
    with torch.no_grad():                                    # non-trivial BN parameters and statistics
        for m in a.modules():
            if isinstance(m, roi_head.RowBatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    b = copy.deepcopy(a)
    assert a._tap_plans(torch.zeros((1, 7, 7, 256 * e), device="cuda")) is not None
    g = torch.Generator(device="cuda").manual_seed(R)
    x = torch.relu(torch.randn((R, 7, 7, 256 * e), device="cuda", generator=g))
    mask = None
    if mode == "masked":
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.25).float()
        x = x * mask.view(R, 1, 1, 1)
    train = mode != "eval"
    a.train(train)
    b.train(train)
    xa, ya = _run_head(torch, a, x, mask, False, monkeypatch)
    xb, yb = _run_head(torch, b, x, mask, True, monkeypatch)
    assert ya.shape == (R, 512 * e)
    _close(torch, ya, yb)
    dy = torch.randn(ya.shape, device="cuda", generator=g)
    if mask is not None:
        dy = dy * mask.unsqueeze(1)
    ya.backward(dy)
    yb.backward(dy)
    _close(torch, xa.grad, xb.grad)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pa.grad is not None, k
        _close(torch, pa.grad, pb.grad)
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        _close(torch, ba, bb, 1e-5)
    if mask is not None:
        assert not bool(xa.grad[mask == 0].any())
    # inference (no autograd): rowbn_apply on the position-major rows
    a.eval()
    b.eval()
    with torch.no_grad():
        _, ia = _run_head(torch, a, x, None, False, monkeypatch, grad=False)
        _, ib = _run_head(torch, b, x, None, True, monkeypatch, grad=False)
    _close(torch, ia, ib)


@pytest.mark.parametrize("depth", [18, 50])
@pytest.mark.parametrize("R", [300, 2000])
@pytest.mark.parametrize("mode", ["train", "eval", "masked"])
def test_head_taps_match_dense_route(torch_cuda, depth, R, mode, monkeypatch):
    """The position-major route against the dense route of the same head, at 1e-4 of each tensor's largest value.
    Both sides share the head's wiring (shortcut inputs, the norm a join applies, slot order, the final mean, the
    buffers' n / eps / momentum); that wiring, and the tolerance's footing, stand on
    test_gpu_network_reference.py, which holds both routes to the f64 statement of tests/network_reference.py."""
    _compare_heads(torch_cuda, depth, R, mode, monkeypatch)


def _masked_vs_compact(torch, depth, dense, monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    if dense:
        monkeypatch.setenv("WSSDL_HEAD_DENSE_3X3", "1")
    else:
        monkeypatch.delenv("WSSDL_HEAD_DENSE_3X3", raising=False)
    torch.manual_seed(0)
    head = roi_head.ResNetHeadNHWC(depth).cuda().train()
    c = 256 * head.group3[0].expansion
    R, Rp = 48, 70
    x_live = torch.relu(torch.randn((R, 7, 7, c), device="cuda"))
    mask = torch.zeros(Rp, device="cuda")
    idx = torch.randperm(Rp, device="cuda")[:R].sort().values
    mask[idx] = 1.0
    x_pad = torch.zeros((Rp, 7, 7, c), device="cuda")
    x_pad[idx] = x_live
    xa = x_live.clone().requires_grad_(True)
    xb = x_pad.clone().requires_grad_(True)
    ya = head(xa)
    roi_head.set_roi_mask(mask)
    try:
        yb = head(xb)
    finally:
        roi_head.set_roi_mask(None)
    w = torch.randn_like(ya)
    (ya * w).sum().backward()
    wb = torch.randn_like(yb)
    wb[idx] = w
    (yb * wb * mask.unsqueeze(1)).sum().backward()
    assert not bool(xb.grad[mask == 0].any())
    return ya, yb[idx], xa.grad, xb.grad[idx]


@pytest.mark.parametrize("depth", [18, 50])
def test_head_taps_masked_matches_compact_rows(torch_cuda, depth, monkeypatch):
    """As test_head_masked_batch_norm_matches_compact_rows, on the class-packed route: dead rows get zero
    gradients and the live rows match the compacted batch.  At depth 50 only the outputs are compared: the
    input gradient of a freshly initialised depth-50 head is ill-conditioned in f32 (dense route, f32 against
    f64: ~2e-2 of its largest value at R = 48), so masked and compacted runs, whose GEMMs differ in M and so
    in rounding, cannot be held to 5e-3; test_head_taps_match_dense_route compares it route against route."""
    torch = torch_cuda
    ya, yb, ga, gb = _masked_vs_compact(torch, depth, False, monkeypatch)
    assert torch.allclose(yb, ya, rtol=2e-3, atol=2e-4)
    if depth == 18:
        assert torch.allclose(gb, ga, rtol=5e-3, atol=1e-5)
