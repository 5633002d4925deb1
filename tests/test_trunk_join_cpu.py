"""CPU: the wiring of the trunk's residual joins (networks/backbones.py: _walk / _join) with a torch stand-in for the
join kernels: every block hands its successor the pre-activation its join computed, the both_preact successors and
the final norm consume only y, running statistics are tracked once per norm, and the result is that of the separate
layers.  Without the stand-in (the real CPU route) no join is attempted and the module state keys are unchanged."""
import copy

import pytest
import torch
import torch.nn.functional as F

from wssdl_bus_amd.networks import _plumbing, backbones, roi_head


def _bn(x, w, b, eps):
    var, mean = torch.var_mean(x, dim=0, unbiased=False)
    return (x - mean) * torch.rsqrt(var + eps) * w + b, mean.detach(), var.detach()


def _standin(calls):
    def apply(x3, other, w3, b3, ws, bs, wn, bn, eps3, eps_s, eps_n, mask, run):
        assert mask is None and run is None and x3.shape == other.shape and x3.dim() == 2
        calls.append(ws is not None)
        t3, m3, v3 = _bn(x3, w3, b3, eps3)
        if ws is not None:
            ts, ms, vs = _bn(other, ws, bs, eps_s)
        else:
            ts, ms, vs = other, None, None
        out = t3 + ts
        y, mn, vn = _bn(out, wn, bn, eps_n)
        return out, F.relu(y), (m3, v3), (ms, vs), (mn, vn), None
    return apply


@pytest.mark.parametrize("depth", [18, 50])
def test_trunk_join_wiring_matches_separate_layers(depth, monkeypatch):
    torch.manual_seed(depth)
    # f64: the stand-in orders its sums differently, and at 1e-16 that stays far below the tolerances
    a = backbones.ResNetTrunk(depth).double().to(memory_format=torch.channels_last).train()
    b = copy.deepcopy(a)
    x = torch.randn(2, 3, 70, 102, dtype=torch.float64).contiguous(memory_format=torch.channels_last)
    xb = x.clone().requires_grad_(True)
    yb = b(xb)                                               # the CPU route: separate layers
    yb.square().mean().backward()

    calls = []
    monkeypatch.setattr(_plumbing, "usable", lambda t: t.dim() == 2 and t.is_contiguous())
    monkeypatch.setattr(_plumbing, "fused_running_stats", lambda: False)
    monkeypatch.setattr(roi_head._JoinFn, "apply", _standin(calls))
    # the single norms stay on stock ops: only _join may see the patched `usable`
    monkeypatch.setattr(backbones.BatchNormAct2d, "forward",
                        lambda self, t, relu=False: (F.relu if relu else (lambda v: v))(
                            torch.nn.BatchNorm2d.forward(self, t)))
    xa = x.clone().requires_grad_(True)
    ya = a(xa)
    ya.square().mean().backward()
    assert len(calls) == {18: 6, 50: 13}[depth] and sum(calls) == {18: 2, 50: 3}[depth]
    assert ya.shape == yb.shape
    assert torch.allclose(ya, yb, rtol=1e-8, atol=1e-10)
    assert torch.allclose(xa.grad, xb.grad, rtol=1e-8, atol=1e-12)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pa.grad is not None, k
        assert torch.allclose(pa.grad, pb.grad, rtol=1e-8, atol=1e-12), k
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(ba) == int(bb) == 1, k               # every norm tracked exactly once
        else:
            assert torch.allclose(ba, bb, rtol=1e-8, atol=1e-12), k
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())


def test_cpu_eval_and_switch_never_join(monkeypatch):
    def boom(*a):
        raise AssertionError("join attempted")
    monkeypatch.setattr(roi_head._JoinFn, "apply", boom)
    t = backbones.ResNetTrunk(18).to(memory_format=torch.channels_last)
    x = torch.randn(1, 3, 70, 102).contiguous(memory_format=torch.channels_last)
    assert t.train()(x).shape == (1, 256, 5, 7)             # CPU tensors: the kernels do not take them
    monkeypatch.setattr(_plumbing, "usable", lambda t: True)
    assert t.eval()(x).shape == (1, 256, 5, 7)
    with torch.no_grad():
        t.train()(x)
    monkeypatch.setenv("WSSDL_TRUNK_UNFUSED_JOIN", "1")
    t.train()(x)
