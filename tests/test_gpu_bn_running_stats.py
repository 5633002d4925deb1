"""-m gpu: running statistics inside the forward finish kernel (csrc/plumbing/rowbn.hip, struct Running) for
RowBatchNorm and BatchNormAct2d, and the backward without materialised gradients of the statistic outputs.

The kernel evaluates, per column, in f64 from the f32 mean / var it has just written and the row count n,
    running_mean <- (float)(rm + mom * (mean - rm))
    running_var  <- (float)(rv + mom * (var * (n / max(n - 1, 1)) - rv))
each rounded once, so (a) the buffers equal that formula restated on the host (torch.equal).  (b) The torch route
(WSSDL_BN_TORCH_RUNNING_STATS=1: an unbias product and lerp_'s difference-product and sum, three f32 roundings of at
most half an ulp of the larger operand each) lies within 2 * 3 * 2^-24 * max(|r|, |stat * unbias|) per element, the
factor 2 being margin.  (c) num_batches_tracked advances by exactly 1 per forward; (d) y and the batch statistics
do not depend on the switch."""
import copy

import pytest

pytestmark = pytest.mark.gpu

# [M, C] with the RoI split of the masked cases (M = n_rois * per) and the NCHW shape of the 2-d layer
SHAPES = {(70, 64): (10, (2, 64, 5, 7)), (1030, 256): (103, (2, 256, 5, 103)), (515, 1024): (103, (1, 1024, 5, 103))}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    if _plumbing.lib() is None:
        pytest.skip("plumbing library not built")
    return torch


def _init(torch, bn, g):
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.weight.shape, device="cuda", generator=g) + 0.5)
        bn.bias.copy_(torch.rand(bn.bias.shape, device="cuda", generator=g) * 0.4 - 0.2)
        bn.running_mean.copy_(torch.rand(bn.bias.shape, device="cuda", generator=g) * 0.2 - 0.1)   # uniform(-0.1, 0.1)
        bn.running_var.copy_(torch.rand(bn.bias.shape, device="cuda", generator=g) * 1.5 + 0.5)    # uniform(0.5, 2)


def _capture(monkeypatch):
    """Records what _FusedRowBatchNormFn returns: (y, mean, var, count)."""
    from wssdl_bus_amd.networks import roi_head
    seen = []
    real = roi_head._FusedRowBatchNormFn.apply

    def apply(*args):
        out = real(*args)
        seen.append(out)
        return out

    monkeypatch.setattr(roi_head._FusedRowBatchNormFn, "apply", apply)
    return seen


def _expected(torch, rm0, rv0, mean, var, n, momentum):
    """the once-rounded f64 formula on the host"""
    mom = float(torch.tensor(momentum, dtype=torch.float32).double())
    rm0, rv0, mean, var = (t.detach().cpu().double() for t in (rm0, rv0, mean, var))
    unbias = n / max(n - 1.0, 1.0)
    stat_v = var * unbias
    rm = (rm0 + mom * (mean - rm0)).float()
    rv = (rv0 + mom * (stat_v - rv0)).float()
    return rm, rv, mean.abs(), stat_v.abs()


def _check(torch, new, old, seen_new, seen_old, rm0, rv0, n, momentum, masked):
    y_n, mean_n, var_n, cnt_n = seen_new
    y_o, mean_o, var_o, cnt_o = seen_old
    # (d) nothing but the buffers depends on the switch
    assert torch.equal(y_n, y_o) and torch.equal(mean_n, mean_o) and torch.equal(var_n, var_o)
    if masked:
        assert torch.equal(cnt_n, cnt_o) and float(cnt_n[0]) == n
    # (a) exact
    rm, rv, s_m, s_v = _expected(torch, rm0, rv0, mean_n, var_n, float(n), momentum)
    print("max |running_mean - formula| = %g, max |running_var - formula| = %g"
          % (float((new.running_mean.cpu() - rm).abs().max()), float((new.running_var.cpu() - rv).abs().max())))
    assert torch.equal(new.running_mean.cpu(), rm)
    assert torch.equal(new.running_var.cpu(), rv)
    assert not torch.equal(new.running_mean, rm0) and not torch.equal(new.running_var, rv0)
    # (b) against torch's ops
    for name, a, b, r0, s in (("running_mean", new.running_mean, old.running_mean, rm0, s_m),
                              ("running_var", new.running_var, old.running_var, rv0, s_v)):
        bound = 2 * 3 * 2.0 ** -24 * torch.maximum(r0.cpu().double().abs(), s)
        d = (a.cpu().double() - b.cpu().double()).abs()
        print("%s: max |new - old| / bound = %g" % (name, float((d / bound).max())))
        assert bool((d <= bound).all()), name


def _mask(torch, kind, n_rois, g):
    if kind == "plain":
        return None
    if kind == "all_dead":
        return torch.zeros((n_rois,), device="cuda")
    m = (torch.rand((n_rois,), device="cuda", generator=g) > 0.3).float()
    m[0], m[1] = 1.0, 0.0                                   # some live, some dead
    return m


@pytest.mark.parametrize("momentum", [0.01, 0.1])
@pytest.mark.parametrize("kind", ["plain", "masked", "masked_pm", "all_dead"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_row_batch_norm_running_stats(torch_cuda, shape, kind, momentum, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.networks import roi_head
    M, C = shape
    n_rois = SHAPES[shape][0]
    g = torch.Generator(device="cuda").manual_seed(M + C)
    new = roi_head.RowBatchNorm(C, momentum=momentum).cuda().train()
    _init(torch, new, g)
    old = copy.deepcopy(new)
    rm0, rv0 = new.running_mean.clone(), new.running_var.clone()
    x = torch.randn((M, C), device="cuda", generator=g) * 1.7 + 0.4
    mask = _mask(torch, kind, n_rois, g)
    pm = kind == "masked_pm"
    n = M if mask is None else max(float(mask.sum()) * (M // n_rois), 1.0)
    seen = _capture(monkeypatch)
    roi_head.set_roi_mask(mask)
    try:
        monkeypatch.delenv("WSSDL_BN_TORCH_RUNNING_STATS", raising=False)
        new(x, relu=True, pos_major=pm)
        monkeypatch.setenv("WSSDL_BN_TORCH_RUNNING_STATS", "1")
        old(x, relu=True, pos_major=pm)
    finally:
        roi_head.set_roi_mask(None)
    assert len(seen) == 2
    _check(torch, new, old, seen[0], seen[1], rm0, rv0, n, momentum, mask is not None)


@pytest.mark.parametrize("momentum", [0.01, 0.1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_batch_norm_act_2d_running_stats(torch_cuda, shape, momentum, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.networks import backbones
    M, C = shape
    nchw = SHAPES[shape][1]
    g = torch.Generator(device="cuda").manual_seed(M + C + 1)
    new = backbones.BatchNormAct2d(C, eps=1e-3, momentum=momentum).cuda().train()
    _init(torch, new, g)
    old = copy.deepcopy(new)
    rm0, rv0 = new.running_mean.clone(), new.running_var.clone()
    x = (torch.randn(nchw, device="cuda", generator=g) * 1.7 + 0.4).contiguous(memory_format=torch.channels_last)
    assert x.permute(0, 2, 3, 1).is_contiguous() and x.numel() == M * C
    seen = _capture(monkeypatch)
    monkeypatch.delenv("WSSDL_BN_TORCH_RUNNING_STATS", raising=False)
    new(x, relu=True)
    monkeypatch.setenv("WSSDL_BN_TORCH_RUNNING_STATS", "1")
    old(x, relu=True)
    assert len(seen) == 2, "the fused row kernels did not run"
    _check(torch, new, old, seen[0], seen[1], rm0, rv0, M, momentum, False)
    # (c) the counter: exactly 1 per forward on either route
    assert int(new.num_batches_tracked) == 1 and int(old.num_batches_tracked) == 1
    monkeypatch.delenv("WSSDL_BN_TORCH_RUNNING_STATS", raising=False)
    new(x, relu=False)
    assert int(new.num_batches_tracked) == 2


def test_no_materialised_stat_gradients(torch_cuda, monkeypatch):
    """One RowBatchNorm forward + backward launches no fill kernel (autograd used to zero-fill gradients for the
    mean / var / count outputs), and its gradients are those of rowbn_backward called directly."""
    torch = torch_cuda
    from torch.profiler import ProfilerActivity, profile
    from wssdl_bus_amd.networks import _plumbing as P, roi_head
    monkeypatch.delenv("WSSDL_BN_TORCH_RUNNING_STATS", raising=False)
    M, C = 1030, 256
    g = torch.Generator(device="cuda").manual_seed(5)
    bn = roi_head.RowBatchNorm(C).cuda().train()
    _init(torch, bn, g)
    x = torch.randn((M, C), device="cuda", generator=g)
    dy = torch.randn((M, C), device="cuda", generator=g)

    def step():
        xx = x.clone().requires_grad_(True)
        bn.weight.grad = bn.bias.grad = None
        bn(xx, relu=True).backward(dy)
        return xx

    step()                                                  # warm-up: nothing lazy inside the profiled region
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        xx = step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert any("rowbn_" in n for n in names), "the profiler saw no kernel of the layer"
    fills = [n for n in names if "FillFunctor" in n]
    assert not fills, fills

    _, stats, _ = P.rowbn_forward(x, bn.weight.detach(), bn.bias.detach(), bn.eps, True)
    dx, dw, db = P.rowbn_backward(x, dy, bn.weight.detach(), stats, True)
    assert torch.equal(xx.grad, dx) and torch.equal(bn.weight.grad, dw) and torch.equal(bn.bias.grad, db)
