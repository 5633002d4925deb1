"""-m gpu: the group-norm kernels (csrc/plumbing/groupnorm.hip through networks/_plumbing.py) against the plain f64
reference of tests/groupnorm_reference.py, computed in torch float64 on the device, each output inside its elementwise
bound (counted roundings, see that module; test_groupnorm_cpu.py shows on the CPU that a model of the kernels stays
inside them and that seeded defects do not).  Shapes are the smallest that reach each path (groupnorm_reference.TABLE).
The backward is judged on its own arithmetic: it takes the kernel's f32 mean / rstd, and its ReLU gate (bit-identical
to y_kernel > 0: the kernels recompute fma(x, scale, shift) > 0) as data, while the forward test checks that gate
against f64 wherever |y64| exceeds its bound.

Then the two networks with norm_type='GN' -- the fused route H against the same module on the stock-PyTorch stand-in in
f32 (S) and f64 (D) under the criterion of tests/network_reference.py, ||H - D|| <= K max(||S - D||, 2^-24 ||D||) per
tensor -- the routes they take, and one full training step."""
import copy
import functools

import pytest
import torch

import groupnorm_reference as GR
import network_reference as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = {}            # worst |error| / bound per kernel output over the module (printed at the end: pytest -s)
NET_WORST = {}      # worst err / floor per network case

# Twice the worst err / floor measured on an MI355X over the network cases below (1.43: trunk, depth 18, a norm's
# weight gradient; six seeds of every case, profiles/groupnorm_netref_ratios.log), rounded up to a power of two.  The
# criterion admits at most 16 (test_gpu_network_reference.py).
K = 4.0


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None, "plumbing library not built"
    yield _plumbing
    for k in sorted(LOG):
        print("gn-worst %s %.4g" % (k, LOG[k]))
    for k in sorted(NET_WORST):
        print("gn-netref-worst %s %.3f %s" % ((k,) + NET_WORST[k]))


@functools.lru_cache(maxsize=2)
def _case(S, Pn, C):
    return GR.make_case(31, S, Pn, C, DEV)


def _mask_kinds(S, Pn, C):
    return ["none"] + (GR.MASK_KINDS if GR.is_small(S, Pn, C) and S > 1 else [])


KERNEL_CASES = [(S, Pn, C, pm, kind) for (S, Pn, C) in GR.TABLE for pm in (False, True)
                for kind in _mask_kinds(S, Pn, C)]


@pytest.mark.parametrize("S,Pn,C,pm,kind", KERNEL_CASES,
                         ids=["%dx%dx%d-%s-%s" % (S, Pn, C, "pm" if pm else "sm", kind) for S, Pn, C, pm, kind in KERNEL_CASES])
def test_kernels_against_f64(P, S, Pn, C, pm, kind):
    c = _case(S, Pn, C)
    x, dy, w, b = c["x"], c["dy"], c["w"], c["b"]
    assert P.groupnorm_usable(x, Pn, GR.G)
    geo = GR.geometry(S, Pn, C)
    small, n, rows = P.groupnorm_plan(S, Pn, C)
    assert (small, n) == (geo[0] == "small", geo[1]) and (small or rows == geo[2]), (geo, small, n, rows)
    mask = None if kind == "none" else GR.make_mask(kind, S, 3, DEV)
    for relu in (False, True):
        case = "%dx%dx%d relu=%d pm=%d mask=%s" % (S, Pn, C, relu, pm, kind)
        y, mean, rstd = P.groupnorm_forward(x, Pn, w, b, GR.EPS, GR.G, relu, mask, pm)
        r, f, by = GR.forward_ratios(x, w, b, GR.EPS, GR.G, Pn, relu, dict(y=y, mean=mean, rstd=rstd), mask, pm)
        GR.check_ratios(case, r, LOG)
        GR.check_gate(case, y, f, by)
        live = f["live"]
        del f, by
        gate = (y > 0) if relu else None
        dx, dg, db = P.groupnorm_backward(x, dy, Pn, w, b, mean, rstd, relu, mask, pm)
        rb, _ = GR.backward_ratios(x, dy, w, mean, rstd, GR.G, Pn, gate, dict(dx=dx, dgamma=dg, dbeta=db), mask, pm)
        GR.check_ratios(case, rb, LOG)
        if mask is not None:
            dead = ~live
            assert not bool(GR.to_groups(y, S, Pn, GR.G, pm)[dead].any()), "%s: y is not zero on dead samples" % case
            assert not bool(GR.to_groups(dx, S, Pn, GR.G, pm)[dead].any()), "%s: dx is not zero on dead samples" % case
            assert not bool(mean[dead].any()) and not bool(rstd[dead].any()), "%s: dead statistics not 0" % case
        if kind == "all_dead":
            assert not bool(dg.any()) and not bool(db.any()), "%s: dgamma / dbeta not 0" % case
        if Pn * C == GR.G:                  # one value per group: var = 0 exactly
            want = float(torch.tensor(GR._eps32(GR.EPS) ** -0.5).float())
            assert torch.equal(rstd, torch.full_like(rstd, want)), "%s: rstd is not eps^-1/2" % case
        # two runs: the same bits
        y2, mean2, rstd2 = P.groupnorm_forward(x, Pn, w, b, GR.EPS, GR.G, relu, mask, pm)
        dx2, dg2, db2 = P.groupnorm_backward(x, dy, Pn, w, b, mean, rstd, relu, mask, pm)
        for name, a, a2 in (("y", y, y2), ("mean", mean, mean2), ("rstd", rstd, rstd2), ("dx", dx, dx2),
                            ("dgamma", dg, dg2), ("dbeta", db, db2)):
            assert torch.equal(a, a2), "%s: %s differs between two runs" % (case, name)


def test_unsupported_shapes_are_declined(P):
    x = torch.zeros((6, 64), device=DEV)
    assert P.groupnorm_usable(x, 3, 8)
    assert not P.groupnorm_usable(x, 3, 4) and not P.groupnorm_usable(x, 4, 8)          # G != 8; rows do not divide
    assert not P.groupnorm_usable(torch.zeros((6, 60), device=DEV), 3, 8)               # C no multiple of 8
    assert not P.groupnorm_usable(torch.zeros((6, 4096), device=DEV), 3, 8)             # C past the kernels' limit
    assert not P.groupnorm_usable(x.double(), 3, 8) and not P.groupnorm_usable(x.cpu(), 3, 8)
    assert not P.groupnorm_usable(torch.zeros((6, 128), device=DEV)[:, :64], 3, 8)      # not contiguous


# ---------------------------------------------------------------- the networks
@pytest.fixture()
def routes(monkeypatch):
    """The head takes the position-major route at every R; no A/B switch is set; fused calls are counted."""
    from wssdl_bus_amd.networks import _plumbing
    monkeypatch.setattr(_plumbing, "TAPS_MIN_ROIS", 1)
    for s in _plumbing.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    calls = {}
    for name in ("groupnorm_forward", "groupnorm_backward", "rowbn_forward", "rowbn_stats", "rowbn_apply",
                 "rowbn_forward_entry", "rowbn_join_forward", "tap_gather_norm", "tap_gather", "slot_mean"):
        real = getattr(_plumbing, name)
        calls[name] = []
        monkeypatch.setattr(_plumbing, name, lambda *a, _r=real, _l=calls[name], **k: (_l.append(1), _r(*a, **k))[1])
    return calls


def _prepare(module):
    """non-trivial weights (network_reference.prepare's, for modules without buffers)"""
    from wssdl_bus_amd.networks import rownorm
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, rownorm.RowGroupNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
            elif "weight" in m._parameters:
                m.weight.mul_(20.0)
    return module.train()


def _step(module, x, dy, mask=None):
    from wssdl_bus_amd.networks import roi_head
    module.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    roi_head.set_roi_mask(mask)
    try:
        y = module(xx)
    finally:
        roi_head.set_roi_mask(None)
    (y * dy).sum().backward()
    return {k: v.detach().clone() for k, v in N.module_outputs(module, y, xx).items()}


def _three(module, x, dy, mask, monkeypatch, routes, share_gates=False):
    """(H, S, D) of one training step and the fused group-norm calls of H and of S.  The three must evaluate one
    piecewise-linear function, or err / floor measures a ReLU argument that f32 rounding put on either side of zero
    and not the route (see SEED).  Two ways to that:
      share_gates=False  H and S are asserted to take the same gates at every norm (inputs chosen so that they do);
      share_gates=True   S and D take H's gates as data, y = pre * gate_H -- what the kernel cases do with the
                         backward's gate -- where the three runs see the same rows in the same order (the trunk).  A gate
                         of H that differs from D's own is admitted only where |pre_D| <= K * max |pre_S - pre_D| of that
                         norm: within K times what the f32 stand-in itself is off by there."""
    from wssdl_bus_amd.networks import rownorm
    real = rownorm.RowGroupNorm.forward
    gates_h, gates_s, pre_s, flipped = [], [], [], []

    def record_h(self, x, samples, relu=False, pos_major=False):
        y = real(self, x, samples, relu=relu, pos_major=pos_major)
        if relu:
            gates_h.append(y.detach() > 0)
        return y

    def run_s(self, x, samples, relu=False, pos_major=False):
        if not relu:
            return real(self, x, samples, relu=False, pos_major=pos_major)
        if not share_gates:
            y = real(self, x, samples, relu=True, pos_major=pos_major)
            gates_s.append(y.detach() > 0)
            return y
        pre = real(self, x, samples, relu=False, pos_major=pos_major)
        pre_s.append(pre.detach())
        return pre * gates_h[len(pre_s) - 1].to(pre.dtype)

    seen_d = [0]

    def run_d(self, x, samples, relu=False, pos_major=False):
        if not (relu and share_gates):
            return real(self, x, samples, relu=relu, pos_major=pos_major)
        pre = real(self, x, samples, relu=False, pos_major=pos_major)
        i = seen_d[0]
        seen_d[0] += 1
        gate = gates_h[i]
        flip = gate != (pre.detach() > 0)
        if bool(flip.any()):
            off = float((pre_s[i].double() - pre.detach()).abs().max())
            flipped.append((i, int(flip.sum()), float(pre.detach()[flip].abs().max()), off))
        return pre * gate.to(pre.dtype)

    monkeypatch.setattr(rownorm.RowGroupNorm, "forward", record_h)
    H = _step(module, x, dy, mask)
    n_h = (len(routes["groupnorm_forward"]), len(routes["groupnorm_backward"]))
    others = {k: len(v) for k, v in routes.items() if k.startswith("rowbn") or k == "tap_gather_norm"}
    assert not any(others.values()), "a group-norm network took a batch-norm route: %s" % others
    monkeypatch.setenv("WSSDL_DISABLE_FUSED_GN", "1")
    monkeypatch.setattr(rownorm.RowGroupNorm, "forward", run_s)
    S = _step(module, x, dy, mask)
    monkeypatch.delenv("WSSDL_DISABLE_FUSED_GN")
    n_s = (len(routes["groupnorm_forward"]) - n_h[0], len(routes["groupnorm_backward"]) - n_h[1])
    if not share_gates:
        flips = sum(int((a != b).sum()) for a, b in zip(gates_h, gates_s))
        assert len(gates_h) == len(gates_s) and flips == 0, \
            "%d ReLU gates differ between the fused route and the stand-in: an input of this seed lies within f32 " \
            "rounding of zero, the comparison says nothing (SEED)" % flips
    monkeypatch.setattr(rownorm.RowGroupNorm, "forward", run_d)
    ref = copy.deepcopy(module).double()
    D = _step(ref, x.double(), dy.double(), mask.double() if mask is not None else None)
    monkeypatch.setattr(rownorm.RowGroupNorm, "forward", real)
    if share_gates:
        assert len(pre_s) == len(gates_h) == seen_d[0]
        for i, n, worst, off in flipped:
            print("gn-gate norm call %d: %d gates of the fused route differ from f64, largest |pre64| %.3g, the f32 "
                  "stand-in is off by %.3g there" % (i, n, worst, off))
            assert worst <= K * off, "norm call %d: a gate of the fused route differs from f64 at |pre64| = %g" % (i, worst)
    return H, S, D, n_h, n_s


def _judge(case, H, S, D):
    N.check_nonzero(D)
    rat = N.ratios(H, S, D)
    assert len(rat) == len(D)
    worst = max(rat, key=rat.get)
    print("gn-netref %s %.3f %s" % (case, rat[worst], worst))
    NET_WORST[case] = (rat[worst], worst)
    over = {k: round(v, 2) for k, v in rat.items() if not v <= K}
    assert not over, (case, over)


def _n_sites(module):
    from wssdl_bus_amd.networks import rownorm
    return sum(isinstance(m, rownorm.RowGroupNorm) for m in module.modules())


# The inputs' seed offset.  Group norm's fused route and its stand-in round differently (batch norm's are bit-identical),
# so a ReLU argument within ~1e-7 of zero can come out on either side; one such element moves every gradient behind it
# by ~1e-4 of its norm in whichever evaluation met it, and err / floor then measures that element, not the route (the
# same finding as for the eval cases of test_gpu_network_reference.py).  The head's GEMMs give the
# same bits on every run, so its cases fix inputs: _three asserts that no gate differs, and of six seeds scanned on an
# MI355X (profiles/groupnorm_netref_ratios.log: the depth-50 head at R = 37 meets such an element under about every
# second seed) seed 1 holds at every case but one, which takes seed 0.  The trunk's convolutions do not repeat bit for
# bit from run to run, so no seed can be fixed for it: its cases hand the fused route's gates to S and D as data
# (_three, share_gates).
SEED = 1
CASE_SEEDS = {"head-d50-r37-dense": 0}


def _seed(case):
    return 1000 * CASE_SEEDS.get(case, SEED)


HEAD_CASES = [(d, R, route) for d in (18, 50) for R, route in ((37, "default"), (1, "default"), (37, "dense"),
                                                               (37, "masked"))]


@pytest.mark.parametrize("depth,R,route", HEAD_CASES, ids=["d%d-r%d-%s" % c for c in HEAD_CASES])
def test_head_training_step(P, depth, R, route, routes, monkeypatch):
    from wssdl_bus_amd.networks import roi_head
    case = "head-d%d-r%d-%s" % (depth, R, route)
    torch.manual_seed(depth + R + _seed(case))
    head = _prepare(roi_head.ResNetHeadNHWC(depth, "GN")).cuda()
    c = {18: 256, 50: 1024}[depth]
    g = torch.Generator(device=DEV).manual_seed(R + _seed(case))
    x = torch.relu(torch.randn((R, 7, 7, c), device=DEV, generator=g))
    dy = torch.randn((R, 2 * c), device=DEV, generator=g)
    mask = None
    if route == "masked":
        mask = torch.ones(R, device=DEV)
        mask[0] = mask[R - 1] = 0.0
        x = torch.where(mask.view(R, 1, 1, 1) > 0, x, 1e3 * torch.randn(x.shape, device=DEV, generator=g))
    if route == "dense":
        monkeypatch.setenv("WSSDL_HEAD_DENSE_3X3", "1")
    H, S, D, n_h, n_s = _three(head, x.contiguous(), dy, mask, monkeypatch, routes)
    sites = _n_sites(head)
    assert n_h == (sites, sites), "fused group-norm calls %s for %d norm sites" % (n_h, sites)
    assert n_s == (0, 0), "WSSDL_DISABLE_FUSED_GN=1 still made fused calls: %s" % (n_s,)
    pm = bool(routes["tap_gather"])
    assert pm == (route != "dense"), "route %s: position-major tap convolutions %s" % (route, pm)
    assert bool(routes["slot_mean"]) == pm                       # _SlotMeanFn still ends the position-major head
    if mask is not None:
        for out in (H, S, D):
            assert not bool(out["dx"][mask == 0].any()) and not bool(out["y"][mask == 0].any())
    _judge(case, H, S, D)


@pytest.mark.parametrize("depth", [18, 50])
def test_trunk_training_step(P, depth, routes, monkeypatch):
    from wssdl_bus_amd.networks import backbones
    torch.manual_seed(depth + _seed("trunk-d%d" % depth))
    trunk = _prepare(backbones.ResNetTrunk(depth, "GN")).cuda().to(memory_format=torch.channels_last)
    g = torch.Generator(device=DEV).manual_seed(depth + _seed("trunk-d%d" % depth))
    x = torch.randn((2, 3, 70, 102), device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        shape = trunk(x).shape
    routes["groupnorm_forward"].clear()
    dy = torch.randn(shape, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    H, S, D, n_h, n_s = _three(trunk, x, dy, None, monkeypatch, routes, share_gates=True)
    sites = _n_sites(trunk)
    assert n_h == (sites, sites) and n_s == (0, 0), (n_h, n_s, sites)
    _judge("trunk-d%d" % depth, H, S, D)


def test_inference_runs_the_forward_kernel(P, routes):
    from wssdl_bus_amd.networks import rownorm
    gn = rownorm.RowGroupNorm(64, 8).cuda().eval()
    x = torch.randn((3 * 49, 64), device=DEV)
    with torch.no_grad():
        y = gn(x, 3, relu=True)
    assert len(routes["groupnorm_forward"]) == 1 and not routes["groupnorm_backward"]
    want = rownorm._group_norm_rows(x.double(), 3, gn.weight.double(), gn.bias.double(), gn.eps, 8, True, None, False)
    assert float((y.double() - want).abs().max()) < 1e-5


def test_full_train_step(P):
    """One combined step (2 supervised + 2 weak images, the smallest synthetic batch of test_gpu_configs.py) of a
    depth-18 'GN' network through the solver: finite losses, a non-zero gradient on every gamma / beta, and a second
    step after the optimiser's update."""
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper
    from wssdl_bus_amd.networks import rownorm
    from wssdl_bus_amd.networks.factory_bus import get_network
    old = (cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG)
    try:
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
        cfg.SAMPLING_RNG = "device"
        torch.manual_seed(13)
        net = get_network("Resnet_train", 18, norm_type="GN").cuda().to(memory_format=torch.channels_last)
        net.train()
        solver = SolverWrapper(net)
        blobs = synthetic.make_batch(2, 2, 320, 480, seed=13)
        losses = solver.joint_backward(blobs)
        for k, v in losses.items():
            assert bool(torch.isfinite(torch.as_tensor(v)).all()), (k, v)
        for name, m in net.named_modules():
            if isinstance(m, rownorm.RowGroupNorm):
                for p in (m.weight, m.bias):
                    assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
        solver._apply()
        losses2 = solver.train_step_joint(blobs)
        assert bool(torch.isfinite(torch.as_tensor(losses2["loss"])).all())
        assert float(losses2["loss"]) != float(losses["loss"])
        solver.check_flags()
    finally:
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG = old
