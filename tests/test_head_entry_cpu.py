"""CPU only: block 1's entry Function (networks/roi_head.py: _EntryNormFn) is a GPU route.  Without the plumbing
library, and on CPU tensors, the head keeps its stock route whatever WSSDL_HEAD_UNFUSED_ENTRY says: same output,
same gradients, and the Function never runs.  Also the position -> slot table the entry kernels read."""
import copy

import torch

from wssdl_bus_amd.networks import _plumbing, roi_head


def _run(head, x, mask):
    xx = x.clone().requires_grad_(True)
    roi_head.set_roi_mask(mask)
    try:
        y = head(xx)
    finally:
        roi_head.set_roi_mask(None)
    y.square().sum().backward()
    return y, xx.grad, [p.grad for p in head.parameters()], [b.clone() for b in head.buffers()]


def test_head_without_plumbing_library_ignores_the_entry_route(monkeypatch):
    monkeypatch.setattr(_plumbing, "lib", lambda: None)
    calls = []
    real = roi_head._EntryNormFn.apply
    monkeypatch.setattr(roi_head._EntryNormFn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    torch.manual_seed(3)
    a = roi_head.ResNetHeadNHWC(50)
    b = copy.deepcopy(a)
    x = torch.relu(torch.randn((6, 7, 7, 1024)))
    mask = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.float32)
    for m in (None, mask):
        monkeypatch.delenv("WSSDL_HEAD_UNFUSED_ENTRY", raising=False)
        ya, ga, pa, ba = _run(a, x, m)
        monkeypatch.setenv("WSSDL_HEAD_UNFUSED_ENTRY", "1")
        yb, gb, pb, bb = _run(b, x, m)
        assert torch.equal(ya, yb) and torch.equal(ga, gb)
        assert all(torch.equal(p, q) for p, q in zip(pa, pb))
        assert all(torch.equal(p, q) for p, q in zip(ba, bb))
        for p in list(a.parameters()) + list(b.parameters()):
            p.grad = None
    assert not calls
    assert not _plumbing.entry_usable(x.reshape(-1, 1024))


def test_subsample_slots_inverts_subsample_index():
    plan = _plumbing.tap_plan(7, 7, 2)
    idx = plan.subsample_index(7, 2, torch.device("cpu"))
    inv = plan.subsample_slots(7, 7, 2, torch.device("cpu"))
    assert inv.dtype == torch.int32 and inv.shape == (49,)
    assert int((inv >= 0).sum()) == len(plan.slots) == 16
    for slot, p in enumerate(idx.tolist()):
        assert int(inv[p]) == slot
