"""-m gpu: the trunk's residual joins (networks/backbones.py: _join / _walk on roi_head._JoinFn, the unmasked
instantiations of the join kernels of csrc/plumbing/rowbn.hip).  ResNetTrunk on the join route against the same
trunk with WSSDL_TRUNK_UNFUSED_JOIN=1 (the separate layers and torch's adds): the join kernels keep the arithmetic
and the order of every sum, so output, gradients and buffers are compared with torch.equal.

Input 2 x 3 x 70 x 102: odd map sizes (group0 17 x 25, group1 9 x 13, group2 5 x 7), so no M is a multiple of the
row slabs or the two-row step, group2 has 70 rows; depth 18 covers C = 64 / 128 / 256 (several rows per workgroup
pass), depth 50 C = 256 / 512 / 1024 (C/4 = 256: one row per pass), the dual form (group0's first block), the
both_preact boundaries (no residual gradient) and the final-norm join.

The trunk's convolutions are MIOpen's, and at these shapes its default solvers do not reproduce their own results
from one call to the next (two runs of the SAME route differed in about 80 of 83 tensors at 6e-7 relative), so no
bit-level comparison of two runs would mean anything; the `deterministic_convs` fixture asks for the deterministic
solvers, under which the separate-layer route reproduces itself bit for bit and the joins must equal it.

Both sides are routes of backbones.py and share its wiring (which tensor a shortcut takes, the norm a join applies as
`nxt`, the hand-over of `pre`, the buffers updated); the reference this bitwise comparison stands on is
test_gpu_network_reference.py, which holds the join route to the f64 statement of the trunk in
tests/network_reference.py."""
import copy

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    if _plumbing.lib() is None:
        pytest.skip("plumbing library not built")
    return torch


@pytest.fixture
def deterministic_convs(torch_cuda):
    cudnn = torch_cuda.backends.cudnn
    old = cudnn.deterministic
    cudnn.deterministic = True
    try:
        yield
    finally:
        cudnn.deterministic = old


def _trunk(torch, depth):
    from wssdl_bus_amd.networks import backbones
    torch.manual_seed(depth)
    t = backbones.ResNetTrunk(depth).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in t.modules():
            if isinstance(m, backbones.BatchNormAct2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
            elif isinstance(m, torch.nn.Conv2d):
                m.weight.mul_(20.0)                     # activations of order 1 through the depth
    return t.train()


def _input(torch):
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((2, 3, 70, 102), device="cuda", generator=g)
    return x.contiguous(memory_format=torch.channels_last)


def _count_joins(monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    calls = []
    real = roi_head._JoinFn.apply
    monkeypatch.setattr(roi_head._JoinFn, "apply", lambda *args: (calls.append(args), real(*args))[1])
    return calls


def _step(torch, trunk, x, unfused, monkeypatch):
    if unfused:
        monkeypatch.setenv("WSSDL_TRUNK_UNFUSED_JOIN", "1")
    else:
        monkeypatch.delenv("WSSDL_TRUNK_UNFUSED_JOIN", raising=False)
    xx = x.clone().requires_grad_(True)
    out = trunk(xx)
    out.square().mean().backward()
    return xx, out


@pytest.mark.parametrize("depth", [18, 50])
def test_trunk_joins_equal_unfused_route(torch_cuda, deterministic_convs, depth, monkeypatch):
    torch = torch_cuda
    a = _trunk(torch, depth)
    b = copy.deepcopy(a)
    c = copy.deepcopy(a)
    x = _input(torch)
    calls = _count_joins(monkeypatch)
    n_blocks = len(a.group0) + len(a.group1) + len(a.group2)
    xa, ya = _step(torch, a, x, False, monkeypatch)
    assert len(calls) == n_blocks == {18: 6, 50: 13}[depth], "the join route did not run a join per block"
    duals = sum(1 for c in calls if c[4] is not None)
    assert duals == {18: 2, 50: 3}[depth]               # the blocks with a projection shortcut
    xb, yb = _step(torch, b, x, True, monkeypatch)
    assert len(calls) == n_blocks, "WSSDL_TRUNK_UNFUSED_JOIN=1 still ran the join kernels"
    assert torch.isfinite(ya).all() and float(ya.abs().max()) > 0
    xc, yc = _step(torch, c, x, True, monkeypatch)      # the reference reproduces itself: the comparison means something
    assert torch.equal(yb, yc) and torch.equal(xb.grad, xc.grad), "the separate-layer route is not reproducible"
    assert torch.equal(ya, yb)
    assert ya.stride() == yb.stride()
    assert torch.equal(xa.grad, xb.grad)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pa.grad is not None and pb.grad is not None, k
        assert torch.equal(pa.grad, pb.grad), k
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(ba, bb), k
        if k.endswith("num_batches_tracked"):
            assert int(ba) == 1, k
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())


@pytest.mark.parametrize("mode", ["eval", "no_grad"])
def test_eval_and_no_grad_never_reach_the_joins(torch_cuda, mode, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    monkeypatch.delenv("WSSDL_TRUNK_UNFUSED_JOIN", raising=False)

    def boom(*a, **k):
        raise AssertionError("rowbn_join_forward called in %s mode" % mode)

    monkeypatch.setattr(_plumbing, "rowbn_join_forward", boom)
    t = _trunk(torch, 18)
    x = _input(torch)
    if mode == "eval":
        t.eval()
        y = t(x.clone().requires_grad_(True))
    else:
        with torch.no_grad():
            y = t(x)
    assert y.shape == (2, 256, 5, 7) and torch.isfinite(y).all()
