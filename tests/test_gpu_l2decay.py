"""-m gpu: the L2 weight decay as one device op (csrc/plumbing/l2decay.hip, networks/_plumbing.py: l2_decay)
against what it replaces in fast_rcnn/train_bus.py: l2_weight_decay, torch's per-parameter chain
stack([(p * p).sum() ...]).sum() * k with k = 0.5 * WEIGHT_DECAY.

* Value: against the f64 numpy sum times k32, |got - ref| <= 2^-23 * ref, where k32 = f32(k) is the constant both
  routes multiply by (torch casts the Python scalar to the tensor's f32).  The argument: w * w is exact in f64; the
  f64 accumulation error over up to 2.6e7 terms is below 3e-9 relative (here a few hundred adds deep: ~1e-14); two
  f32 roundings follow -- the sum's and the product's -- each at most 2^-24 / (1 + 2^-24) relative.
* Gradients: torch.equal to the chain's, for an upstream gradient of 1 and of 0.37, each with its parameter's
  strides.  The kernel issues the chain's roundings: c = gout * k32, t = w * c, t + t.
* A list the op does not take (a non-dense view) runs the chain; another parameter list rebuilds the chunk table,
  the same list does not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None
    return torch


def _params(torch):
    """numel 1, 3, one chunk, one chunk + 1, a channels_last conv weight (dense, permuted), a [512, 4608] weight
    (576 chunks), and a contiguous slice that starts one float into its storage (not float4-aligned: the scalar
    form of both kernels)."""
    g = torch.Generator(device="cuda").manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda") * 0.05
    ps = [rn(1), rn(3), rn(4096), rn(4097),
          rn(64, 3, 7, 7).contiguous(memory_format=torch.channels_last), rn(512, 4608),
          rn(4100)[1:4098].detach()]
    assert not ps[4].is_contiguous() and ps[6].data_ptr() % 16 == 4
    return [p.requires_grad_() for p in ps]


def _chain(torch, params, k):
    return torch.stack([(p * p).sum() for p in params]).sum() * k


K = 0.5 * 0.0005


def test_value_against_f64_sum(torch_cuda):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    params = _params(torch)
    assert _plumbing.l2decay_usable(params)
    got = _plumbing.l2_decay(params, K)
    assert got.shape == () and got.dtype == torch.float32
    k32 = float(np.float32(K))
    ref = sum(float((p.detach().cpu().numpy().astype(np.float64) ** 2).sum()) for p in params) * k32
    err = abs(float(got.item()) - ref)
    print("l2 decay value: got %.9g ref %.9g rel err %.3g (bound %.3g)" % (got.item(), ref, err / ref, 2.0 ** -23))
    assert err <= 2.0 ** -23 * ref


@pytest.mark.parametrize("gout", [1.0, 0.37])
def test_gradients_equal_the_torch_chain(torch_cuda, gout):
    torch = torch_cuda
    from wssdl_bus_amd.networks import _plumbing
    params = _params(torch)
    g = torch.tensor(gout, dtype=torch.float32, device="cuda")
    want = torch.autograd.grad(_chain(torch, params, K), params, grad_outputs=g)
    got = torch.autograd.grad(_plumbing.l2_decay(params, K), params, grad_outputs=g)
    for p, a, b in zip(params, got, want):
        assert a.shape == p.shape and a.stride() == p.stride()
        assert torch.equal(a, b), (tuple(p.shape), float((a - b).abs().max()))


def test_backward_accumulates_into_grad_like_the_chain(torch_cuda):
    """.backward() through the training step's function: .grad equals the chain's, twice in a row (accumulated)."""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.fast_rcnn.config import cfg
    params = _params(torch)
    k = 0.5 * cfg.TRAIN.WEIGHT_DECAY
    for _ in range(2):
        loss = T.l2_weight_decay(params)
        assert type(loss.grad_fn).__name__ == "_L2DecayFnBackward"
        loss.backward()
    got = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    for _ in range(2):
        _chain(torch, params, k).backward()
    for p, a in zip(params, got):
        assert torch.equal(a, p.grad)


def test_fallback_switch_and_table_rebuild(torch_cuda, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.networks import _plumbing
    params = _params(torch)
    k = 0.5 * cfg.TRAIN.WEIGHT_DECAY
    # a non-dense view sends the whole call to torch's chain
    strided = torch.randn(64, 8, device="cuda")[:, ::2].requires_grad_()
    mixed = params + [strided]
    assert not _plumbing.l2decay_usable(mixed) and not _plumbing.l2decay_usable([])
    assert not _plumbing.l2decay_usable(params[:2] + [params[2].double()])
    loss = T.l2_weight_decay(mixed)
    assert type(loss.grad_fn).__name__ == "MulBackward0"
    assert torch.equal(loss, _chain(torch, mixed, k))
    # so does the switch
    monkeypatch.setenv("WSSDL_TORCH_L2_DECAY", "1")
    assert type(T.l2_weight_decay(params).grad_fn).__name__ == "MulBackward0"
    monkeypatch.delenv("WSSDL_TORCH_L2_DECAY")
    # the table is built once per parameter list; in-place updates keep it, another list rebuilds it
    T.l2_weight_decay(params)
    n = _plumbing.L2_TABLE_BUILDS[0]
    with torch.no_grad():
        for p in params:
            p.mul_(0.5)
    a = T.l2_weight_decay(params)
    a.backward()
    assert _plumbing.L2_TABLE_BUILDS[0] == n
    b = T.l2_weight_decay(params[:-1])
    assert _plumbing.L2_TABLE_BUILDS[0] == n + 1
    ref_b = sum(float((p.detach().cpu().numpy().astype(np.float64) ** 2).sum()) for p in params[:-1]) \
        * float(np.float32(k))
    assert abs(float(b.item()) - ref_b) <= 2.0 ** -23 * ref_b
    c = T.l2_weight_decay(params)
    assert _plumbing.L2_TABLE_BUILDS[0] == n + 2 and torch.equal(a, c)
