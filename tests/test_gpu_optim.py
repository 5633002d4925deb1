"""-m gpu: the reference optimisers as one HIP launch (csrc/plumbing/optim.hip, fast_rcnn/optim.py) against the f64
statement and the counted elementwise bounds of tests/optim_reference.py.

* HIP against f64: every element of every parameter and state tensor inside its bound, for each optimiser, at t = 1,
  2 and 1000, from a state that is not zero (m of mixed signs, vhat on both sides of v).  The parameter set is that of
  test_gpu_l2decay.py (numel 1, 3, one chunk, one chunk + 1, a channels_last weight, a 576-chunk matrix, a slice 4
  bytes off alignment: the scalar form) plus a parameter without a gradient, a channels_last parameter with a
  contiguous gradient (copied into the parameter's layout) and one whose gradient is all zeros; the 4097-element
  parameter's gradient is itself 4 bytes off alignment.
* Nesterov has no sqrt and no division: torch.equal with the torch-op form run on the CPU.
* HIP against the WSSDL_TORCH_OPTIM=1 route on the GPU: within the sum of the two routes' bounds.
* A parameter without a gradient is bit-identical before and after, state included.
* The chunk table is built once per parameter list.
* One real train step with opt='adam': the f64 reference applied to the gradients the step produced gives the new
  parameters; and opt='sgd' under the one-rank RCCL context equals the plain step."""
import os

import numpy as np
import pytest

import optim_reference as R

pytestmark = pytest.mark.gpu

KINDS = ("adam", "amsgrad", "sgd")
LR = 5e-4
NONE_GRAD, CL_PARAM_CONTIG_GRAD, ZERO_GRAD = 7, 8, 9


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None
    return torch


def _params(torch, device, seed=11):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: (torch.randn(*s, generator=g) * 0.05).to(device)
    ps = [rn(1), rn(3), rn(4096), rn(4097),
          rn(64, 3, 7, 7).contiguous(memory_format=torch.channels_last), rn(512, 4608),
          rn(4100)[1:4098].detach(), rn(33),
          rn(8, 4, 3, 3).contiguous(memory_format=torch.channels_last), rn(1000)]
    assert not ps[4].is_contiguous() and not ps[8].is_contiguous()
    assert device == "cpu" or ps[6].data_ptr() % 16 == 4
    return [p.requires_grad_() for p in ps]


def _set_grads(torch, params, seed):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        r = (torch.randn(p.shape, generator=g) * 0.01).to(p.device)
        if i == NONE_GRAD:
            p.grad = None
        elif i == ZERO_GRAD:
            p.grad = torch.zeros_like(p)
        elif i == CL_PARAM_CONTIG_GRAD:
            p.grad = r.contiguous()
            assert p.grad.stride() != p.stride()
        elif i == 3:
            buf = torch.zeros(p.numel() + 4, device=p.device)
            buf[1:1 + p.numel()] = r
            p.grad = buf[1:1 + p.numel()]
            assert p.device.type == "cpu" or p.grad.data_ptr() % 16 == 4
        elif i == 4:
            p.grad = r.contiguous(memory_format=torch.channels_last)
        else:
            p.grad = r


def _inject_state(torch, opt, seed=1):
    """through load_state_dict: m (accum) of mixed signs, v >= 0, vhat = 1.5 v or 0.5 v (both sides of the max)"""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for i, p in enumerate(opt.params):
        r = [torch.randn(p.shape, generator=g) for _ in range(3)]
        v = r[1] * r[1] * 1e-3
        full = dict(m=r[0] * 0.02, accum=r[0] * 0.02, v=v, vhat=v * (1.0 + 0.5 * torch.sign(r[2])))
        state[i] = {s: full[s] for s in opt.views}
    opt.load_state_dict(dict(kind=opt.kind, step=0, lr=LR, state=state))
    if opt.kind == "amsgrad":
        vh, v = opt.views["vhat"][5], opt.views["v"][5]
        assert bool((vh > v).any()) and bool((vh < v).any())
    first = opt.views["accum" if opt.kind == "sgd" else "m"][5]
    assert bool((first < 0).any()) and bool((first > 0).any()) and opt.t == 0


def _make(torch, kind, device="cuda"):
    from wssdl_bus_amd.fast_rcnn import optim as O
    params = _params(torch, device)
    opt = O.ReferenceOptimizer(params, kind, LR, eps=0.1, momentum=0.9)
    _inject_state(torch, opt)
    return O, params, opt


STEPS = ((1, 21), (2, 22), (1000, 23))          # (t, gradient seed)


def _run(torch, opt, params, check=None):
    """the three steps; `check(t, before)` after each"""
    for t, seed in STEPS:
        opt.t = t - 1                            # t = 1000 is set through the step count
        _set_grads(torch, params, seed)
        before = R.snapshot(opt) if check else None
        opt.step()
        if check:
            check(t, before)
        opt.zero_grad()


@pytest.mark.parametrize("kind", KINDS)
def test_hip_against_f64_reference(torch_cuda, kind):
    torch = torch_cuda
    O, params, opt = _make(torch, kind)
    assert O.hip_usable(params)
    worst = []

    def check(t, before):
        assert before[NONE_GRAD]["g"] is None and not before[ZERO_GRAD]["g"].any()
        worst.append(R.check_step(opt, before, t, LR, 0.9, what="hip"))
        print("%s t = %d: worst error / bound %.3f" % (kind, t, worst[-1]))
    _run(torch, opt, params, check)
    assert len(worst) == 3 and max(worst) <= 1.0 and opt.t == 1000


def test_nesterov_equals_the_torch_form_on_the_cpu(torch_cuda):
    torch = torch_cuda
    O, params, opt = _make(torch, "sgd")
    _, cparams, copt = _make(torch, "sgd", "cpu")
    for p, q in zip(params, cparams):
        assert torch.equal(p.detach().cpu(), q.detach())
    _run(torch, opt, params)
    _run(torch, copt, cparams)
    for i, (p, q) in enumerate(zip(params, cparams)):
        assert torch.equal(p.detach().cpu(), q.detach()), i
        assert torch.equal(opt.views["accum"][i].cpu(), copt.views["accum"][i]), i
    assert not torch.equal(cparams[0].detach(), _params(torch, "cpu")[0].detach())
    print("nesterov: HIP == torch-op form on the CPU, bit for bit, %d parameters, 3 steps" % len(params))


@pytest.mark.parametrize("kind", KINDS)
def test_hip_against_the_torch_route_on_the_gpu(torch_cuda, kind, monkeypatch):
    torch = torch_cuda
    O, params, opt = _make(torch, kind)
    _, tparams, topt = _make(torch, kind)
    n = O.TABLE_BUILDS[0]
    worst = []
    for t, seed in STEPS:
        # both from the same f32 state, so that the comparison stays per step
        with torch.no_grad():
            for p, q in zip(tparams, params):
                p.copy_(q)
        topt.load_state_dict(opt.state_dict())
        opt.t = topt.t = t - 1
        _set_grads(torch, params, seed)
        _set_grads(torch, tparams, seed)
        before = R.snapshot(opt)
        opt.step()
        monkeypatch.setenv("WSSDL_TORCH_OPTIM", "1")
        assert not O.hip_usable(tparams)
        topt.step()
        monkeypatch.delenv("WSSDL_TORCH_OPTIM")
        # each route is inside its bound of the same f64 value, so the two differ by at most the sum of the bounds
        for i, b in enumerate(before):
            got = dict(p=(params[i], tparams[i]), **{s: (opt.views[s][i], topt.views[s][i]) for s in opt.views})
            if b["g"] is None:
                assert all(torch.equal(x, y) for x, y in got.values())
                continue
            ref = R.step(kind, b["p"], b["g"], {s: b[s] for s in opt.views}, LR, t, 0.1, 0.9)
            for k, (x, y) in got.items():
                d = np.abs(R.to_numpy(x).astype(np.float64) - R.to_numpy(y).astype(np.float64))
                worst.append(float((d / (2 * ref[k][1])).max()))
                assert worst[-1] <= 1.0, (kind, t, i, k, worst[-1])
    assert O.TABLE_BUILDS[0] == n + 1            # the torch route builds no table
    print("%s HIP vs torch ops on the GPU: worst difference / (sum of the two bounds) %.3f" % (kind, max(worst)))


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_without_gradient_is_bit_identical(torch_cuda, kind):
    torch = torch_cuda
    O, params, opt = _make(torch, kind)
    _set_grads(torch, params, 5)
    p0 = params[NONE_GRAD].detach().clone()
    s0 = {s: v[NONE_GRAD].clone() for s, v in opt.views.items()}
    first = params[0].detach().clone()
    opt.step()
    assert torch.equal(params[NONE_GRAD].detach(), p0) and not torch.equal(params[0].detach(), first)
    for s, v in opt.views.items():
        assert torch.equal(v[NONE_GRAD], s0[s]) and bool(s0[s].abs().max() > 0)
    # the padding between the parameters' state segments stays zero
    for s, buf in opt.buffers.items():
        used = torch.zeros_like(buf, dtype=torch.bool)
        for p, off in zip(params, opt.offsets):
            used[off:off + p.numel()] = True
        assert not bool(buf[~used].any())


def test_chunk_table_is_built_once_per_parameter_list(torch_cuda):
    torch = torch_cuda
    O, params, opt = _make(torch, "adam")
    n = O.TABLE_BUILDS[0]
    for seed in (1, 2, 3):
        _set_grads(torch, params, seed)              # new gradient tensors every step
        opt.step()
        opt.zero_grad()
    assert O.TABLE_BUILDS[0] == n + 1
    rows = opt._table[1].chunks.cpu().tolist()
    assert len(rows) == sum(-(-p.numel() // O.CHUNK) for p in params) and rows[4] == [3, O.CHUNK, 1, opt.offsets[3] + O.CHUNK]
    other = O.ReferenceOptimizer(params[:-1], "adam", LR)
    _set_grads(torch, params, 4)
    other.step()
    assert O.TABLE_BUILDS[0] == n + 2
    opt.step()
    assert O.TABLE_BUILDS[0] == n + 2                # the first optimiser still holds its own
    with torch.no_grad():
        params[1].data = params[1].data.clone()      # a re-allocated parameter rebuilds it
    opt.step()
    assert O.TABLE_BUILDS[0] == n + 3
    torch.cuda.synchronize()


def test_train_step_joint_with_reference_adam(torch_cuda):
    """One combined step on the smallest network and input of the solver tests (test_gpu_edges.py), opt='adam': the
    f64 reference applied to the gradients the step produced reproduces the new parameters inside the bounds."""
    torch = torch_cuda
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn import optim as O
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper
    from wssdl_bus_amd.networks.factory_bus import get_network
    old = cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 1, 1
    cfg.SAMPLING_RNG = "reference"
    np.random.seed(3)
    torch.manual_seed(3)
    try:
        net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
        blobs = synthetic.make_batch(1, 1, 320, 480, seed=3)
        solver = SolverWrapper(net, opt="adam")
        opt = solver.optimizer
        assert isinstance(opt, O.ReferenceOptimizer) and opt.kind == "adam" and O.hip_usable(opt.params)
        before, step = [], opt.step

        def spy():                                   # the gradients as _apply hands them to the optimiser
            before.extend(R.snapshot(opt))
            step()
        opt.step = spy
        losses = solver.train_step_joint(blobs)
        for k in ("loss", "mil_cross_entropy", "rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box"):
            assert torch.isfinite(losses[k]).all(), k
        assert solver.global_step == 1 and opt.t == 1 and len(before) == len(opt.params)
        assert all(p.grad is None for p in opt.params)
        with_grad = [i for i, b in enumerate(before) if b["g"] is not None]
        assert len(with_grad) > len(before) // 2
        moved = sum(1 for i in with_grad if not np.array_equal(R.to_numpy(opt.params[i]), before[i]["p"]))
        assert moved > len(with_grad) // 2
        worst = R.check_step(opt, before, 1, solver.lr, what="train step")
        print("train_step_joint, opt='adam': %d parameters, %d with a gradient, %d moved, worst error / bound %.3f"
              % (len(before), len(with_grad), moved, worst))
    finally:
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG = old


def _worker_sgd_force_dist(port, q):
    try:
        import test_gpu_distributed as D
        np_, torch, cfg, get_network = D._setup(0, 1, port, None, force=False)
        import copy
        from wssdl_bus_amd import synthetic
        from wssdl_bus_amd.distributed import DistContext
        from wssdl_bus_amd.fast_rcnn import optim as O
        from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper
        net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
        net.train()
        state0 = copy.deepcopy(net.state_dict())
        blobs = synthetic.make_batch(1, 1, 320, 480, seed=21)
        outs = []
        for kind in ("plain", "plain", "plain", "plain", "dist"):
            D._load(net, state0)
            ctx = None
            if kind == "dist":
                os.environ["WSSDL_FORCE_DIST"] = "1"
                ctx = DistContext(bucket_bytes=4 << 20)
                assert ctx.enabled and ctx.backend == "nccl" and ctx.world_size == 1
            solver = SolverWrapper(net, dist_ctx=ctx, opt="sgd")
            assert isinstance(solver.optimizer, O.ReferenceOptimizer) and O.hip_usable(solver.params)
            cfg.DEVICE_RNG_SEED = 3
            np_.random.seed(7)
            solver.train_step_joint(blobs)
            torch.cuda.synchronize()
            outs.append(D._flat(torch, D._params(net)).clone())
            if kind == "dist":
                assert len(solver.overlap.buckets) >= 2
                solver.overlap.remove()
                ctx.shutdown()
        plain, b = outs[:-1], outs[-1]
        moved = float((plain[0] - D._flat(torch, [state0[k] for k, _ in net.named_parameters()])).abs().max())
        repeat = max(float((x - y).abs().max()) for i, x in enumerate(plain) for y in plain[i + 1:])
        dist_d = min(float((x - b).abs().max()) for x in plain)
        q.put(dict(ok=True, repeat=repeat, dist=dist_d, moved=moved))
    except Exception as e:                                   # surface the child's failure in the parent
        import traceback
        q.put(dict(ok=False, err=traceback.format_exc() + repr(e)))


@pytest.mark.timeout(600)
def test_sgd_under_one_rank_rccl_equals_the_plain_step():
    """opt='sgd' with the bucketed, backward-overlapped all-reduce of one RCCL rank: the same parameters as without it
    -- the yardstick of test_gpu_distributed.py: bit for bit when the backward is deterministic, else no further from
    the plain step than twice what four plain repeats differ among themselves (MIOpen's weight gradients use atomics;
    a lost or unscaled bucket shows at the scale of `moved`, orders above)."""
    import torch.multiprocessing as mp
    import test_gpu_distributed as D
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_sgd_force_dist, args=(D._free_port(), q))
    p.start()
    res = q.get(timeout=540)
    p.join(timeout=60)
    assert res["ok"], res.get("err")
    print("sgd under one-rank RCCL: %r" % (res,))
    assert res["moved"] > 0
    if res["repeat"] == 0.0:
        assert res["dist"] == 0.0, res
    else:
        assert res["dist"] <= max(2 * res["repeat"], 1e-3 * res["moved"]), res
