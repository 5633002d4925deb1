"""CPU only: when a bottleneck's conv1 norm moves into the 3x3 patch gather (networks/roi_head.py:
_BlockNHWC._tapnorm_fused / _conv12_pm, TapConv3x3Fn's norm form).  It is a GPU route: the predicate's conditions are
checked with a stand-in for the input, and on CPU tensors the head is the same with and without
WSSDL_HEAD_UNFUSED_TAPNORM and never calls TapConv3x3Fn."""
import copy
import types

import torch

from wssdl_bus_amd.networks import _plumbing, roi_head


def test_predicate(monkeypatch):
    monkeypatch.setattr(_plumbing, "lib", lambda: object())
    monkeypatch.delenv("WSSDL_HEAD_UNFUSED_TAPNORM", raising=False)
    gpu, cpu = types.SimpleNamespace(is_cuda=True), types.SimpleNamespace(is_cuda=False)
    fused = roi_head._BlockNHWC._tapnorm_fused
    bott = roi_head.BottleneckNHWC(64, 16, 2, "both_preact", "BN")
    body = [bott.conv1, bott.conv2]
    assert fused(body, gpu) and not fused(body, cpu)
    monkeypatch.setenv("WSSDL_HEAD_UNFUSED_TAPNORM", "1")
    assert not fused(body, gpu)
    monkeypatch.delenv("WSSDL_HEAD_UNFUSED_TAPNORM")
    bott.conv1.bn.eval()                                            # an inference-mode norm has no batch statistics
    assert not fused(body, gpu)
    bott.conv1.bn.train()
    basic = roi_head.BasicBlockNHWC(64, 64, 2, "both_preact", "BN")
    assert not fused([basic.conv1], gpu)                            # the basic block: a 3x3 conv1, one body member
    plain = roi_head.BottleneckNHWC(64, 16, 2, "both_preact", None)
    assert not fused([plain.conv1, plain.conv2], gpu)               # no norm to move
    monkeypatch.setattr(_plumbing, "lib", lambda: None)
    assert not fused(body, gpu)
    assert "WSSDL_HEAD_UNFUSED_TAPNORM" in _plumbing.SWITCHES


def test_cpu_head_ignores_the_switch(monkeypatch):
    calls = []
    real = _plumbing.TapConv3x3Fn.apply
    monkeypatch.setattr(_plumbing.TapConv3x3Fn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    torch.manual_seed(4)
    a = roi_head.ResNetHeadNHWC(50)
    b = copy.deepcopy(a)
    x = torch.relu(torch.randn((5, 7, 7, 1024)))
    outs = []
    for head, on in ((a, False), (b, True)):
        if on:
            monkeypatch.setenv("WSSDL_HEAD_UNFUSED_TAPNORM", "1")
        else:
            monkeypatch.delenv("WSSDL_HEAD_UNFUSED_TAPNORM", raising=False)
        xx = x.clone().requires_grad_(True)
        y = head(xx)
        y.square().sum().backward()
        outs.append((y, xx.grad, [p.grad for p in head.parameters()], [t.clone() for t in head.buffers()]))
    (ya, ga, pa, ba), (yb, gb, pb, bb) = outs
    assert torch.equal(ya, yb) and torch.equal(ga, gb)
    assert all(torch.equal(p, q) for p, q in zip(pa + ba, pb + bb))
    assert not calls
