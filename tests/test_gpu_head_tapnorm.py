"""-m gpu: a bottleneck's conv1 norm + ReLU inside the 3x3 patch gather (csrc/plumbing/taps.hip:
tap_gather_kernel<true>, csrc/plumbing/rowbn.hip: wsplumb_rowbn_stats, networks/_plumbing.py: TapConv3x3Fn's norm
form) against the separate layers it replaces.  torch.equal throughout: the statistics come from the layer's own
partial and finish kernels, the gather applies bn_affine and the ReLU exactly as rowbn_apply_fwd_kernel does
(bn_math.hip.h), and the backward is the two layers' own.

* kernel level: tap_gather_norm(x) == tap_gather(rowbn_forward(x).y), statistics and running statistics included,
  for the two geometries the head runs, both source layouts, the shapes of test_gpu_head_entry.py (RoI counts that
  are no multiple of the workgroup's chunk or of its rows per pass, C/4 that does not divide 256), without a mask
  and with dead RoIs (whose rows hold finite garbage the kernel must not read into the result).
* head level: ResNet-50 head at R = 2051 against WSSDL_HEAD_UNFUSED_TAPNORM=1: output, every gradient, every buffer."""
import copy

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None
    return torch


def _entry():
    import test_gpu_head_entry as E
    return E


def _shapes():
    return _entry().SHAPES


# both geometries from a roi-major source; a position-major source keeps the map's size (blocks 2 and 3)
LAYOUTS = [(7, 7, 2, False), (4, 4, 1, False), (4, 4, 1, True)]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("h,w,s,in_pm", LAYOUTS, ids=["7x7s2-roi_major", "4x4s1-roi_major", "4x4s1-pos_major"])
@pytest.mark.parametrize("R,C", _shapes())
def test_gather_with_norm_equals_layer_then_gather(torch_cuda, R, C, h, w, s, in_pm, masked):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing as P
    plan = P.tap_plan(h, w, s)
    g = torch.Generator(device="cuda").manual_seed(h * 1000 + R + C + 7 * in_pm)
    x = torch.randn((R, h, w, C), device="cuda", generator=g) * 1.5 + 0.3
    mask = None
    if masked:
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.3).float()
        mask[0], mask[R - 1] = 1.0, 0.0
        x = torch.where(mask.view(R, 1, 1, 1) > 0, x, 1e3 * torch.randn(x.shape, device="cuda", generator=g))
    rows = (_entry()._to_pm(x, plan) if in_pm else x.reshape(-1, C)).contiguous()
    wn = torch.rand((C,), device="cuda", generator=g) + 0.5
    bn = torch.rand((C,), device="cuda", generator=g) * 0.4 - 0.2

    def buffers():
        return (torch.full((C,), 0.25, device="cuda"), torch.full((C,), 1.5, device="cuda"), 0.01,
                torch.zeros((1,), dtype=torch.int64, device="cuda"))

    if not P.usable(rows):
        # C = 40: the statistics kernels do not take C/4 = 10 (it neither divides 256 nor is a multiple of it), so no
        # norm layer of this width exists; the gather itself takes any C % 4 == 0 and is held to the elementwise
        # apply kernel (any C % 4 == 0 too) under given scale / shift, dead RoIs zeroed as the layer writes them
        assert C == 40
        scale = torch.randn((C,), device="cuda", generator=g)
        shift = torch.randn((C,), device="cuda", generator=g) * 0.5
        y = P.rowbn_apply(rows, scale, shift, True)
        if mask is not None:
            live = (mask.repeat(h * w) if in_pm else mask.repeat_interleave(h * w)).unsqueeze(1) > 0
            y = torch.where(live, y, torch.zeros_like(y))
        want = P.tap_gather(y if in_pm else y.view(R, h, w, C), plan, in_pm, R)
        got = P.tap_gather_norm(rows, plan, in_pm, R, scale, shift, mask)
    else:
        run_a, run_b = buffers(), buffers()
        y, stats_a, count_a = P.rowbn_forward(rows, wn, bn, 1e-3, True, mask, in_pm, running=run_a)
        want = P.tap_gather(y if in_pm else y.view(R, h, w, C), plan, in_pm, R)
        stats_b, count_b = P.rowbn_stats(rows, wn, bn, 1e-3, mask, in_pm, running=run_b)
        got = P.tap_gather_norm(rows, plan, in_pm, R, stats_b[3], stats_b[4], mask)
        assert torch.equal(stats_a, stats_b)
        assert (count_a is None and count_b is None) or torch.equal(count_a, count_b)
        for a, b in zip(run_a, run_b):
            assert not torch.is_tensor(a) or torch.equal(a, b)
        assert int(run_b[3]) == 1
    assert got.shape == want.shape and torch.equal(got, want)
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) > 0.0


@pytest.mark.parametrize("in_pm", [False, True], ids=["roi_major", "pos_major"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_function_equals_separate_layers(torch_cuda, in_pm, masked):
    """TapConv3x3Fn's norm form against _FusedRowBatchNormFn then TapConv3x3Fn: output and the four gradients."""
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing as P, rownorm
    R, C, CO = 131, 64, 24
    plan = P.tap_plan(4, 4, 1) if in_pm else P.tap_plan(7, 7, 2)
    g = torch.Generator(device="cuda").manual_seed(5 + in_pm)
    mask = None
    if masked:
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.3).float()
        mask[0] = 1.0
    leaves = lambda: [t.clone().requires_grad_() for t in base]
    base = [torch.randn((plan.h * plan.w * R, C), device="cuda", generator=g),
            torch.rand((C,), device="cuda", generator=g) + 0.5, torch.rand((C,), device="cuda", generator=g) - 0.5,
            torch.randn((CO, 9 * C), device="cuda", generator=g) * 0.1]
    dy = torch.randn((plan.oh * plan.ow * R, CO), device="cuda", generator=g)
    xa, wa, ba, Wa = leaves()
    y1 = rownorm._FusedRowBatchNormFn.apply(xa, wa, ba, 1e-3, True, mask, in_pm and mask is not None, None)[0]
    ya = P.TapConv3x3Fn.apply(y1 if in_pm else y1.view(R, plan.h, plan.w, C), Wa, None, plan, in_pm, R)
    ya.backward(dy)
    xb, wb, bb, Wb = leaves()
    yb, mean, var, _ = P.TapConv3x3Fn.apply(xb, Wb, None, plan, in_pm, R, wb, bb, 1e-3, mask, None)
    assert not mean.requires_grad and not var.requires_grad
    yb.backward(dy)
    assert torch.equal(ya, yb)
    for a, b in ((xa, xb), (wa, wb), (ba, bb), (Wa, Wb)):
        assert a.grad is not None and torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("mode", ["train", "masked"])
def test_head_equals_unfused_tapnorm_route(torch_cuda, mode, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing, roi_head
    R = 2051                                                  # >= TAPS_MIN_ROIS: the position-major route
    assert R >= _plumbing.TAPS_MIN_ROIS
    for s in ("WSSDL_HEAD_DENSE_3X3", "WSSDL_HEAD_UNFUSED_TAPNORM"):
        monkeypatch.delenv(s, raising=False)
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
    mask = None
    if mode == "masked":
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.25).float()
        mask[100:900] = 0.0
        x = x * mask.view(-1, 1, 1, 1)

    normed = []
    real = _plumbing.TapConv3x3Fn.apply
    monkeypatch.setattr(_plumbing.TapConv3x3Fn, "apply", lambda *args: (normed.append(len(args) > 6), real(*args))[1])

    def run(head, unfused):
        if unfused:
            monkeypatch.setenv("WSSDL_HEAD_UNFUSED_TAPNORM", "1")
        else:
            monkeypatch.delenv("WSSDL_HEAD_UNFUSED_TAPNORM", raising=False)
        xx = x.clone().requires_grad_(True)
        roi_head.set_roi_mask(mask)
        try:
            y = head(xx)
        finally:
            roi_head.set_roi_mask(None)
        return xx, y

    xa, ya = run(a, False)
    assert normed == [True] * 3, "the bottlenecks did not take the norm form of the tap convolution"
    xb, yb = run(b, True)
    assert normed == [True] * 3 + [False] * 3, "WSSDL_HEAD_UNFUSED_TAPNORM=1 still ran the norm form"
    assert torch.equal(ya, yb)
    dy = torch.randn(ya.shape, device="cuda", generator=g)
    if mask is not None:
        dy = dy * mask.unsqueeze(1)
    ya.backward(dy)
    yb.backward(dy)
    assert torch.equal(xa.grad, xb.grad)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), n
    for (n, p), q in zip(a.named_buffers(), b.buffers()):
        assert torch.equal(p, q), n
