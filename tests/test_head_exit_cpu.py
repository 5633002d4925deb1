"""CPU only: the head's exit inside the last join (networks/roi_head.py: _Exit / _join_pm, rownorm._JoinFn's exit form,
rownorm._SlotMeanFn) is a GPU route.  On CPU tensors, and without the plumbing library, the head keeps torch's
mean(dim=(1, 2)) whatever WSSDL_HEAD_UNFUSED_EXIT says -- same output, gradients and buffers -- and calls neither
_JoinFn nor _SlotMeanFn; the predicate's conditions are checked with a stand-in for the input."""
import copy
import types

import torch

from wssdl_bus_amd.networks import _plumbing, roi_head


def test_predicate(monkeypatch):
    monkeypatch.delenv("WSSDL_HEAD_UNFUSED_EXIT", raising=False)
    monkeypatch.delenv("WSSDL_HEAD_UNFUSED_JOIN", raising=False)
    monkeypatch.setattr(_plumbing, "usable", lambda x: True)
    x = types.SimpleNamespace(shape=(16 * 37, 2048))
    assert _plumbing.exit_usable(x)
    monkeypatch.setenv("WSSDL_HEAD_UNFUSED_EXIT", "1")
    assert not _plumbing.exit_usable(x)
    monkeypatch.delenv("WSSDL_HEAD_UNFUSED_EXIT")
    monkeypatch.setenv("WSSDL_HEAD_UNFUSED_JOIN", "1")             # no join, no exit form of it
    assert not _plumbing.exit_usable(x)
    monkeypatch.delenv("WSSDL_HEAD_UNFUSED_JOIN")
    assert not _plumbing.exit_usable(types.SimpleNamespace(shape=(2 ** 31, 2048)))
    monkeypatch.setattr(_plumbing, "usable", lambda x: False)      # CPU tensors, no library
    assert not _plumbing.exit_usable(x)
    assert "WSSDL_HEAD_UNFUSED_EXIT" in _plumbing.SWITCHES


def test_cpu_head_ignores_the_switch(monkeypatch):
    calls = []
    for fn in (roi_head._JoinFn, roi_head._SlotMeanFn):
        real = fn.apply
        monkeypatch.setattr(fn, "apply", lambda *a, _r=real: (calls.append(1), _r(*a))[1])
    torch.manual_seed(4)
    a = roi_head.ResNetHeadNHWC(50)
    b = copy.deepcopy(a)
    x = torch.relu(torch.randn((5, 7, 7, 1024)))
    outs = []
    for head, on in ((a, False), (b, True)):
        if on:
            monkeypatch.setenv("WSSDL_HEAD_UNFUSED_EXIT", "1")
        else:
            monkeypatch.delenv("WSSDL_HEAD_UNFUSED_EXIT", raising=False)
        xx = x.clone().requires_grad_(True)
        y = head(xx)
        y.square().sum().backward()
        outs.append((y, xx.grad, [p.grad for p in head.parameters()], [t.clone() for t in head.buffers()]))
    (ya, ga, pa, ba), (yb, gb, pb, bb) = outs
    assert ya.shape == (5, 2048)
    assert torch.equal(ya, yb) and torch.equal(ga, gb)
    assert all(torch.equal(p, q) for p, q in zip(pa + ba, pb + bb))
    assert not calls


def test_cpu_head_output_is_torch_mean(monkeypatch):
    """inference mode (no batch statistics, so a second pass changes nothing): the head's output is torch's mean of
    the final norm's output over the positions, with and without the switch"""
    torch.manual_seed(5)
    head = roi_head.ResNetHeadNHWC(18).eval()
    x = torch.relu(torch.randn((3, 7, 7, 256)))
    with torch.no_grad():
        want = roi_head._norm_relu(head.norm, head.group3(x)).mean(dim=(1, 2))
        for on in (False, True):
            if on:
                monkeypatch.setenv("WSSDL_HEAD_UNFUSED_EXIT", "1")
            else:
                monkeypatch.delenv("WSSDL_HEAD_UNFUSED_EXIT", raising=False)
            assert torch.equal(head(x), want)
