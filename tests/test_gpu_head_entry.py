"""-m gpu: the start of the per-RoI head on the position-major route.

* The patch kernels of csrc/plumbing/taps.hip (one workgroup per (position, tap) unit or input position and
  RoI chunk) against the dense patch route (im2col.hip): the gather is a copy and the adjoint keeps the dense
  adjoint's (ky, kx) order, so both are compared with torch.equal.
* Block 1's entry gradient (csrc/plumbing/rowbn.hip: wsplumb_rowbn_backward_entry, networks/roi_head.py:
  _EntryNormFn) against the sequence it replaces -- torch's zero-fill, index_add and add, then the plain
  backward -- and the head against its WSSDL_HEAD_UNFUSED_ENTRY=1 route.  torch.equal throughout: the kernels
  keep every operand and the order of every sum.

These route-against-route comparisons stand on test_gpu_headconv_reference.py, which holds both patch routes to a
plain f64 convolution element by element."""
import copy

import pytest

pytestmark = pytest.mark.gpu

GEOMS = [(7, 7, 2), (4, 4, 1)]          # the two shapes the head runs


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None
    return torch


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
    R, h, w, C = x.shape
    return x.reshape(R, h * w, C)[:, [y * w + xx for y, xx in plan.slots]].transpose(0, 1).reshape(-1, C).contiguous()


def _dense(x, plan):
    from wssdl_bus_amd.networks import _plumbing
    return _plumbing.Im2Col3x3Fn.apply(x, plan.s, plan.oh, plan.ow, plan.pt, plan.pl)


# R: below one RoI chunk, not a multiple of either chunk (16 / 32 RoIs) or of the rows a workgroup walks per
# pass; C = 40: C/4 does not divide 256 (the one-row-per-pass form of the thread mapping).
SHAPES = [(37, 256), (37, 512), (131, 256), (131, 512), (7, 40)]


@pytest.mark.parametrize("h,w,s", GEOMS)
@pytest.mark.parametrize("R,C", SHAPES)
def test_gather_equals_dense_patches_in_the_valid_columns(torch_cuda, h, w, s, R, C):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    plan = _plumbing.tap_plan(h, w, s)
    g = torch.Generator(device="cuda").manual_seed(h * 1000 + R + C)
    x = torch.randn((R, h, w, C), device="cuda", generator=g)
    want = _dense(x, plan).view(-1, C)[_pack_index(torch, plan, R)].reshape(-1)
    got = _plumbing.tap_gather(x, plan, False, R)
    assert got.shape == want.shape and torch.equal(got, want)
    if plan.h == plan.oh:                                   # position-major source (blocks 2 and 3)
        assert torch.equal(_plumbing.tap_gather(_to_pm(x, plan), plan, True, R), want)


@pytest.mark.parametrize("h,w,s", GEOMS)
@pytest.mark.parametrize("R,C", SHAPES)
def test_adjoint_equals_dense_adjoint(torch_cuda, h, w, s, R, C):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    plan = _plumbing.tap_plan(h, w, s)
    g = torch.Generator(device="cuda").manual_seed(7 + h * 1000 + R + C)
    packed = torch.randn((plan.units * R * C,), device="cuda", generator=g)
    dense = torch.zeros((R * plan.oh * plan.ow * 9, C), device="cuda")
    dense[_pack_index(torch, plan, R)] = packed.view(-1, C)
    x = torch.zeros((R, h, w, C), device="cuda", requires_grad=True)
    _dense(x, plan).backward(dense.view(R * plan.oh * plan.ow, 9 * C))
    want = x.grad
    assert torch.equal(_plumbing.tap_col2im(packed, plan, False, R, C), want)
    if plan.h == plan.oh:
        assert torch.equal(_plumbing.tap_col2im(packed, plan, True, R, C), _to_pm(want, plan))


def _mask(torch, kind, R, g):
    if kind == "none":
        return None
    m = (torch.rand((R,), device="cuda", generator=g) > 0.3).float()
    if kind == "dead_slabs":
        m[R // 5:R // 5 + min(R // 2, 300)] = 0.0            # a dead run longer than a row slab
        m[-3:] = 0.0
    m[0] = 1.0
    return m


@pytest.mark.parametrize("mask_kind", ["none", "random", "dead_slabs"])
@pytest.mark.parametrize("R,C", [(37, 1024), (611, 1024), (301, 256)])
def test_entry_backward_equals_scatter_add_then_plain_backward(torch_cuda, mask_kind, R, C):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing as P
    plan = P.tap_plan(7, 7, 2)
    per, ns = 49, len(plan.slots)
    g = torch.Generator(device="cuda").manual_seed(R + C)
    mask = _mask(torch, mask_kind, R, g)
    x = torch.randn((R * per, C), device="cuda", generator=g)
    w = torch.rand((C,), device="cuda", generator=g) + 0.5
    b = torch.rand((C,), device="cuda", generator=g) * 0.4 - 0.2
    dy = torch.randn((R * per, C), device="cuda", generator=g)
    dys = torch.randn((ns * R, C), device="cuda", generator=g)
    # signed zeros in both parts: the scatter into a zero tensor turns the shortcut's -0 into +0
    dy.view(R, per, C)[::3, :, ::5] = -0.0
    dys.view(ns, R, C)[:, ::3, ::5] = -0.0
    dys.view(ns, R, C)[:, 1::4, 1::7] = 0.0
    y, stats, _ = P.rowbn_forward(x, w, b, 1e-3, True, mask)

    # the separate ops, as autograd runs them for _pm_rows and the sum of the two consumers' gradients
    idx = plan.subsample_index(7, 2, x.device)
    z = torch.zeros((per, R, C), device="cuda").index_add_(0, idx, dys.view(ns, R, C))
    total = (dy.view(R, per, C) + z.transpose(0, 1)).contiguous().view(-1, C)
    dx, dw, db = P.rowbn_backward(x, total, w, stats, True, mask)

    edx, edw, edb = P.rowbn_backward_entry(x, dy, dys, plan.subsample_slots(7, 7, 2, x.device), ns, w, stats, mask)
    torch.cuda.synchronize()
    for name, a, want in (("dx", edx, dx), ("dweight", edw, dw), ("dbias", edb, db)):
        assert torch.equal(a, want), "%s differs: max |d| = %g" % (name, float((a - want).abs().max()))
    # bit patterns too (torch.equal holds -0 == +0)
    assert torch.equal(edx.view(torch.int32), dx.view(torch.int32))
    if mask is not None:
        assert not bool(edx.view(R, per, C)[mask == 0].any())


def _run_head(head, x, mask, unfused, monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    if unfused:
        monkeypatch.setenv("WSSDL_HEAD_UNFUSED_ENTRY", "1")
    else:
        monkeypatch.delenv("WSSDL_HEAD_UNFUSED_ENTRY", raising=False)
    xx = x.clone().requires_grad_(True)
    roi_head.set_roi_mask(mask)
    try:
        y = head(xx)
    finally:
        roi_head.set_roi_mask(None)
    return xx, y


@pytest.mark.parametrize("mode", ["train", "masked"])
def test_head_entry_equals_unfused_route(torch_cuda, mode, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing, roi_head
    R = 2051                                                  # >= TAPS_MIN_ROIS: the position-major route
    assert R >= _plumbing.TAPS_MIN_ROIS
    monkeypatch.delenv("WSSDL_HEAD_DENSE_3X3", raising=False)
    torch.manual_seed(50)
    a = roi_head.ResNetHeadNHWC(50).cuda()
    with torch.no_grad():
        for m in a.modules():
            if isinstance(m, roi_head.RowBatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    b = copy.deepcopy(a)
    g = torch.Generator(device="cuda").manual_seed(R)
    x = torch.relu(torch.randn((R, 7, 7, 1024), device="cuda", generator=g))
    assert a._tap_plans(x) is not None
    mask = None
    if mode == "masked":
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.25).float()
        mask[100:900] = 0.0
        x = x * mask.view(-1, 1, 1, 1)

    calls = []
    real = roi_head._EntryNormFn.apply
    monkeypatch.setattr(roi_head._EntryNormFn, "apply", lambda *args: (calls.append(1), real(*args))[1])
    xa, ya = _run_head(a, x, mask, False, monkeypatch)
    assert len(calls) == 1, "block 1 did not take the entry Function"
    xb, yb = _run_head(b, x, mask, True, monkeypatch)
    assert len(calls) == 1, "WSSDL_HEAD_UNFUSED_ENTRY=1 still ran the entry Function"
    assert torch.equal(ya, yb)
    dy = torch.randn(ya.shape, device="cuda", generator=g)
    if mask is not None:
        dy = dy * mask.unsqueeze(1)
    ya.backward(dy)
    yb.backward(dy)
    assert torch.equal(xa.grad, xb.grad)
    if mask is not None:
        assert not bool(xa.grad[mask == 0].any())
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pa.grad is not None and pb.grad is not None, k
        assert torch.equal(pa.grad, pb.grad), k
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(ba, bb), k
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
