"""-m gpu: the residual joins of the per-RoI head's position-major section (csrc/plumbing/rowbn.hip:
wsplumb_rowbn_join_*, networks/roi_head.py: _JoinFn / _join_pm).  The join kernels against the sequence they
replace -- rowbn_forward / rowbn_backward on each branch and torch's adds -- and the head against its unfused
route (WSSDL_HEAD_UNFUSED_JOIN=1).  Everything is compared with torch.equal: the joins keep the arithmetic and
the order of every sum, so no output may differ in any bit."""
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


def _mask(torch, kind, R, g):
    """None, a random live-row mask, or one whose dead RoIs cover whole row slabs of the partial kernels."""
    if kind == "none":
        return None
    m = (torch.rand((R,), device="cuda", generator=g) > 0.3).float()
    if kind == "dead_slabs":
        m[R // 5:R // 5 + min(R // 2, 700)] = 0.0            # a dead run longer than a slab (slabs are <= ~450 rows)
        m[-3:] = 0.0
    m[0] = 1.0
    return m


def _bn(torch, C, g):
    w = torch.rand((C,), device="cuda", generator=g) + 0.5
    b = torch.rand((C,), device="cuda", generator=g) * 0.4 - 0.2
    return w, b, 1e-3


# R: not a multiple of the slab height, the block size or the two-row step; 2053 rows * 16 positions spans every
# partial block count up to the cap at C = 2048.
@pytest.mark.parametrize("mask_kind", ["none", "random", "dead_slabs"])
@pytest.mark.parametrize("C", [512, 2048])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("R", [37, 2053])
def test_join_kernels_equal_separate_layers(torch_cuda, mask_kind, C, dual, res, R):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing as P
    g = torch.Generator(device="cuda").manual_seed(R * 7 + C + 2 * dual + res)
    per = 16
    M = R * per
    mask = _mask(torch, mask_kind, R, g)
    x3 = torch.randn((M, C), device="cuda", generator=g)
    other = torch.randn((M, C), device="cuda", generator=g) * 1.5 + 0.3
    bn3, bns, bnn = _bn(torch, C, g), _bn(torch, C, g), _bn(torch, C, g)
    dy = torch.randn((M, C), device="cuda", generator=g)
    dres = torch.randn((M, C), device="cuda", generator=g) if res else None

    # today's sequence
    t3, st3, _ = P.rowbn_forward(x3, bn3[0], bn3[1], bn3[2], False, mask, pos_major=mask is not None)
    if dual:
        ts, sts, _ = P.rowbn_forward(other, bns[0], bns[1], bns[2], False, mask, pos_major=mask is not None)
    else:
        ts, sts = other, None
    out = t3 + ts
    y, stn, cnt = P.rowbn_forward(out, bnn[0], bnn[1], bnn[2], True, mask, pos_major=mask is not None)
    dxn, dwn, dbn = P.rowbn_backward(out, dy, bnn[0], stn, True, mask, pos_major=mask is not None)
    gg = dxn + dres if res else dxn
    dx3, dw3, db3 = P.rowbn_backward(x3, gg, bn3[0], st3, False, mask, pos_major=mask is not None)
    if dual:
        dxs, dws, dbs = P.rowbn_backward(other, gg, bns[0], sts, False, mask, pos_major=mask is not None)

    # the joins
    jout, jy, jst3, jsts, jstn, jcnt = P.rowbn_join_forward(x3, bn3, other, bns if dual else None, bnn, mask)
    jg, jdx3, jdxs, jdwbn, jdwb3, jdwbs = P.rowbn_join_backward(
        jout, dy, dres, x3, other if dual else None, bnn[0], jstn, bn3[0], jst3, bns[0] if dual else None,
        jsts if dual else None, mask)
    torch.cuda.synchronize()

    def same(name, a, b):
        assert torch.equal(a, b), "%s differs: max |d| = %g" % (name, float((a - b).abs().max()))

    same("out", jout, out)
    same("next stats", jstn, stn)
    same("bn3 stats", jst3, st3)
    same("y", jy, y)
    if mask is not None:
        same("count", jcnt, cnt)
        dead = (mask == 0).repeat(per)
        assert not bool(jy[dead].any()) and not bool(jdx3[dead].any())
    same("g", jg, gg)
    same("dx3", jdx3, dx3)
    same("dweight_n", jdwbn[0], dwn)
    same("dbias_n", jdwbn[1], dbn)
    same("dweight3", jdwb3[0], dw3)
    same("dbias3", jdwb3[1], db3)
    if dual:
        same("shortcut stats", jsts, sts)
        same("dxs", jdxs, dxs)
        same("dweight_s", jdwbs[0], dws)
        same("dbias_s", jdwbs[1], dbs)


def _run_head(torch, head, x, mask, unfused, monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    if unfused:
        monkeypatch.setenv("WSSDL_HEAD_UNFUSED_JOIN", "1")
    else:
        monkeypatch.delenv("WSSDL_HEAD_UNFUSED_JOIN", raising=False)
    xx = x.clone().requires_grad_(True)
    roi_head.set_roi_mask(mask)
    try:
        y = head(xx)
    finally:
        roi_head.set_roi_mask(None)
    return xx, y


@pytest.mark.parametrize("depth", [18, 50])
@pytest.mark.parametrize("mode", ["train", "masked"])
def test_head_fused_joins_equal_unfused_route(torch_cuda, depth, mode, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing, roi_head
    R = 2051                                                  # >= TAPS_MIN_ROIS: the position-major route
    assert R >= _plumbing.TAPS_MIN_ROIS
    monkeypatch.delenv("WSSDL_HEAD_DENSE_3X3", raising=False)
    torch.manual_seed(depth)
    a = roi_head.ResNetHeadNHWC(depth).cuda()
    e = a.group3[0].expansion
    with torch.no_grad():
        for m in a.modules():
            if isinstance(m, roi_head.RowBatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    b = copy.deepcopy(a)
    g = torch.Generator(device="cuda").manual_seed(R)
    x = torch.relu(torch.randn((R, 7, 7, 256 * e), device="cuda", generator=g))
    assert a._tap_plans(x) is not None
    mask = None
    if mode == "masked":
        mask = (torch.rand((R,), device="cuda", generator=g) > 0.25).float()
        mask[100:900] = 0.0
        x = x * mask.view(-1, 1, 1, 1)

    calls = []
    real = roi_head._JoinFn.apply
    monkeypatch.setattr(roi_head._JoinFn, "apply", lambda *args: (calls.append(1), real(*args))[1])
    xa, ya = _run_head(torch, a, x, mask, False, monkeypatch)
    assert len(calls) == len(a.group3), "the fused route did not run a join per block"
    xb, yb = _run_head(torch, b, x, mask, True, monkeypatch)
    assert len(calls) == len(a.group3), "WSSDL_HEAD_UNFUSED_JOIN=1 still ran the join kernels"
    assert torch.equal(ya, yb)
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
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())


def test_head_joins_without_autograd_in_training_mode(torch_cuda, monkeypatch):
    """Training mode under torch.no_grad(): the head still takes the join kernels (its eligibility has no autograd
    term, unlike the trunk's), while block 1's entry Function, which exists for its backward, is not taken.  Output
    and every buffer equal the unfused route's bit for bit."""
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing, roi_head
    R = 37
    monkeypatch.setattr(_plumbing, "TAPS_MIN_ROIS", 1)        # the position-major route at any R
    for s in ("WSSDL_HEAD_DENSE_3X3", "WSSDL_HEAD_UNFUSED_ENTRY"):
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
    before = {k: v.clone() for k, v in a.named_buffers()}
    assert a.training and b.training
    g = torch.Generator(device="cuda").manual_seed(R)
    x = torch.relu(torch.randn((R, 7, 7, 1024), device="cuda", generator=g))
    assert a._tap_plans(x) is not None

    calls = {"join": [], "entry": []}
    for key, fn in (("join", roi_head._JoinFn), ("entry", roi_head._EntryNormFn)):
        real = fn.apply
        monkeypatch.setattr(fn, "apply", lambda *args, _r=real, _l=calls[key]: (_l.append(1), _r(*args))[1])
    with torch.no_grad():
        _, ya = _run_head(torch, a, x, None, False, monkeypatch)
        assert (len(calls["join"]), len(calls["entry"])) == (3, 0), calls
        _, yb = _run_head(torch, b, x, None, True, monkeypatch)
    assert (len(calls["join"]), len(calls["entry"])) == (3, 0), calls
    assert not ya.requires_grad and torch.equal(ya, yb)
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(ba, bb), k
    assert all(not torch.equal(v, before[k]) for k, v in a.named_buffers()), "a norm did not track its statistics"
