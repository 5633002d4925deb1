"""-m gpu: every fused route through networks/roi_head.py (ResNetHeadNHWC) and networks/backbones.py (ResNetTrunk)
against the independent f64 statement of the two networks in tests/network_reference.py, on output, input gradient,
every parameter gradient and every buffer.  test_network_reference_cpu.py proves that reference against the one
route that uses no kernel and shows that the criterion sees every seeded wiring defect; this module closes the
triangle.  The route-against-route suites (test_gpu_trunk_join.py, test_gpu_head_taps.py, test_gpu_head_join.py,
test_gpu_head_entry.py, test_gpu_padded.py) stand on it: a mistake in the wiring their two sides share shows here.

Criterion (network_reference): err(H) = ||H - D|| <= K * max(||S - D||, 2^-24 ||D||, 2^-24 ||D_sib||) for every
tensor, H the route, D / S the reference in f64 / f32 on the device.  K is one constant for the module: twice the
worst measured err / floor over all cases and tensors, rounded up to a power of two ("Networks against
an f64 reference"; profiles/netref_ratios.log).  Every case prints its worst ratio per output class
(`netref <case> <class> <ratio> <tensor>`) before it asserts, and the module ends with `netref-worst <class>
<ratio>` lines (pytest -s).

Exact checks: the trunk's num_batches_tracked is 1 after one step; in eval mode every buffer is bit-identical to its
value before the call; dx is exactly zero on dead RoIs; and the default route ran the fused calls it is supposed to
(joins / entry / tap convolutions: 3 / 1 / 3 at depth 50, 2 / 0 / 4 at depth 18, one join per trunk block), the
all-switches-off route none of them.

Shapes: R = 37 (odd: M = 1813 rows at 7 x 7, 592 at 4 x 4, neither a multiple of a row slab), R = 1 (M = 49 and
16), a masked batch whose first and last rows are dead, a masked batch with one live RoI; the trunk at 2 x 3 x 70 x
102 (maps 17 x 25, 9 x 13, 5 x 7), where conv0's total padding is odd."""
import copy

import pytest

import network_reference as N

pytestmark = pytest.mark.gpu

# Twice the worst err / floor measured on an MI355X over all cases below (7.24: trunk, depth 50, a norm's bias
# gradient), rounded up to a power of two.  16 is also the largest value the criterion admits: two f32 evaluations of
# one graph do not differ by more, and every seeded defect of test_network_reference_cpu.py gives 1e4 and more.
K = 16.0

_SWITCHES = ("WSSDL_HEAD_DENSE_3X3", "WSSDL_HEAD_UNFUSED_JOIN", "WSSDL_HEAD_UNFUSED_ENTRY")
_WORST = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None
    return torch


@pytest.fixture(autouse=True)
def taps_at_any_r(monkeypatch):
    """The head takes the class-packed route from _plumbing.TAPS_MIN_ROIS RoIs on; here at every R."""
    from wssdl_bus_amd.networks import _plumbing
    monkeypatch.setattr(_plumbing, "TAPS_MIN_ROIS", 1)
    monkeypatch.delenv("WSSDL_TRUNK_UNFUSED_JOIN", raising=False)
    for s in _SWITCHES:
        monkeypatch.delenv(s, raising=False)


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print()
    for c in N.CLASSES:
        if c in _WORST:
            print("netref-worst %s %.3f (%s %s)" % ((c,) + _WORST[c]))


def _judge(case, H, S, D):
    """Every floating-point tensor of D inside K * floor; prints the case's worst ratio per class first."""
    N.check_nonzero(D)
    rat = N.ratios(H, S, D)
    assert len(rat) == sum(v.dtype.is_floating_point for v in D.values())
    print()
    for c, (r, name) in sorted(N.worst_by_class(rat, D.keys()).items()):
        print("netref %s %s %.3f %s" % (case, c, r, name))
        if r > _WORST.get(c, (-1.0,))[0]:
            _WORST[c] = (r, case, name)
    over = {k: round(v, 2) for k, v in rat.items() if not v <= K}
    assert not over, (case, over)


def _counters(monkeypatch):
    """Calls of the fused Functions: {'join': [...], 'entry': [...], 'taps': [...]}."""
    from wssdl_bus_amd.networks import _plumbing, roi_head
    calls = {"join": [], "entry": [], "taps": []}
    for key, fn in (("join", roi_head._JoinFn), ("entry", roi_head._EntryNormFn), ("taps", _plumbing.TapConv3x3Fn)):
        real = fn.apply
        monkeypatch.setattr(fn, "apply", lambda *a, _r=real, _l=calls[key]: (_l.append(len(a)), _r(*a))[1])
    return calls


def _step(module, x, dy, mask=None, grad=True):
    import torch
    from wssdl_bus_amd.networks import roi_head
    xx = x.clone().requires_grad_(grad)
    roi_head.set_roi_mask(mask)
    try:
        with torch.set_grad_enabled(grad):
            y = module(xx)
    finally:
        roi_head.set_roi_mask(None)
    if not grad:
        return {"y": y}
    (y * dy).sum().backward()
    return N.module_outputs(module, y, xx)


def _head(torch, depth, seed):
    from wssdl_bus_amd.networks import roi_head
    torch.manual_seed(seed)
    return N.prepare(roi_head.ResNetHeadNHWC(depth)).cuda()


def _head_inputs(torch, depth, R, live, seed):
    """relu(randn) on the live RoIs, 1e3 * randn (finite garbage) on the dead ones; randn upstream on all."""
    c = {18: 256, 50: 1024}[depth]
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.relu(torch.randn((R, 7, 7, c), device="cuda", generator=g))
    dy = torch.randn((R, 2 * c), device="cuda", generator=g)
    mask = idx = None
    if live is not None:
        idx = torch.tensor(live, device="cuda")
        mask = torch.zeros(R, device="cuda")
        mask[idx] = 1.0
        x = torch.where(mask.view(R, 1, 1, 1) > 0, x, 1e3 * torch.randn(x.shape, device="cuda", generator=g))
        assert float(dy[mask == 0].abs().min()) > 0
    return x.contiguous(), dy, mask, idx


HEAD_CASES = [
    # id, depth, R, live RoIs, route, (joins, entry, tap convolutions)
    ("d50-r37", 50, 37, None, "default", (3, 1, 3)),
    ("d50-r37-unfused", 50, 37, None, "unfused", (0, 0, 0)),
    ("d50-r37-masked", 50, 37, list(range(1, 29)), "default", (3, 1, 3)),
    ("d50-r1", 50, 1, None, "default", (3, 1, 3)),
    ("d18-r37", 18, 37, None, "default", (2, 0, 4)),
    ("d18-r5-one-live", 18, 5, [3], "default", (2, 0, 4)),
]


@pytest.mark.parametrize("case,depth,R,live,route,fused", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_training_step(torch_cuda, case, depth, R, live, route, fused, monkeypatch):
    torch = torch_cuda
    if route == "unfused":
        for s in _SWITCHES:
            monkeypatch.setenv(s, "1")
    head = _head(torch, depth, depth + R)
    state = copy.deepcopy(head.state_dict())
    x, dy, mask, idx = _head_inputs(torch, depth, R, live, R)
    if live is not None:
        assert mask[0] == 0 and mask[R - 1] == 0 and int(mask.sum()) == len(live)
    calls = _counters(monkeypatch)
    H = _step(head, x, dy, mask)
    assert (len(calls["join"]), len(calls["entry"]), len(calls["taps"])) == fused, \
        "route %s ran joins / entry / tap convolutions %s" % (route, {k: len(v) for k, v in calls.items()})
    if live is not None:
        assert not bool(H["dx"][mask == 0].any()), "a dead RoI received a gradient"
        H["y"], H["dx"] = H["y"][idx], H["dx"][idx]
    D = N.head(state, x.double(), dy.double(), depth, live=idx)
    S = N.head(state, x, dy, depth, live=idx)
    _judge(case, H, S, D)


def _calibrated_eval_head(torch, depth, seed):
    """A head for inference whose running buffers are random AROUND the statistics of its own activations.  With
    the buffers of N.prepare (variance in [0.5, 2] whatever the layer sees) the x 20 weights make the eval-mode
    activations grow to 5e6 through the depth, and so do the gradients: one ReLU whose argument changes sign under
    f32 rounding then moves every gradient behind it by 1e-4 of its norm, in S as in any route (measured on the CPU
    route: ||S - D|| / ||D|| of dx 5e-5, of the route 4e-4, of later weight gradients 5e-7 against 3e-4), and err /
    floor measures which of the two met such an element, not the route.  So the buffers are first set to the batch
    statistics of a calibration input (one training-mode forward with momentum 1 on the CPU route), then randomised:
    variance x [0.8, 1.25], mean moved by up to 0.1 standard deviations.  Activations stay of order 1, as in
    training mode, and the reference takes the resulting state like any other."""
    from wssdl_bus_amd.networks import roi_head
    torch.manual_seed(seed)
    head = N.prepare(roi_head.ResNetHeadNHWC(depth))
    norms = [m for m in head.modules() if isinstance(m, roi_head.RowBatchNorm)]
    for m in norms:
        m.momentum = 1.0
    with torch.no_grad():
        head(torch.relu(torch.randn((37, 7, 7, {18: 256, 50: 1024}[depth]))))
        for m in norms:
            m.momentum = 0.01
            m.running_var.mul_(torch.empty_like(m.running_var).uniform_(0.8, 1.25))
            m.running_mean.add_(m.running_var.sqrt() * torch.empty_like(m.running_mean).uniform_(-0.1, 0.1))
    return head.cuda().eval()


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "autograd"])
@pytest.mark.parametrize("buffers", ["randomised", "calibrated"])
def test_head_eval(torch_cuda, buffers, grad, monkeypatch):
    """Inference: under no_grad the rowbn_apply kernel, with autograd torch's addcmul; both against the reference's
    eval form (running buffers in, buffers untouched).  With the buffers of N.prepare y and dx are judged; with
    the calibrated ones (_calibrated_eval_head) every parameter gradient too."""
    torch = torch_cuda
    head = _calibrated_eval_head(torch, 50, 50) if buffers == "calibrated" else _head(torch, 50, 50).eval()
    state = copy.deepcopy(head.state_dict())
    x, dy, _, _ = _head_inputs(torch, 50, 37, None, 37)
    H = _step(head, x, dy, grad=grad)
    for k, v in head.state_dict().items():
        assert torch.equal(v, state[k]), k
    D = N.head(state, x.double(), dy.double(), 50, training=False)
    S = N.head(state, x, dy, 50, training=False)
    for k, v in state.items():
        if "running" in k:
            assert torch.equal(S["b." + k], v), k
    keep = None if grad and buffers == "calibrated" else ("y", "dx") if grad else ("y",)
    if keep is not None:
        H, S, D = ({k: t[k] for k in keep} for t in (H, S, D))
    if buffers == "calibrated":
        assert float(D["y"].abs().max()) < 1e2               # the calibration kept the activations of order 1
    _judge("d50-r37-eval-%s-%s" % (buffers, "autograd" if grad else "no_grad"), H, S, D)


@pytest.mark.parametrize("depth", [18, 50])
def test_trunk_training_step(torch_cuda, depth, monkeypatch):
    torch = torch_cuda
    from wssdl_bus_amd.networks import backbones
    torch.manual_seed(depth)
    trunk = N.prepare(backbones.ResNetTrunk(depth)).cuda().to(memory_format=torch.channels_last)
    state = copy.deepcopy(trunk.state_dict())
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((2, 3, 70, 102), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    dy = torch.randn((2, trunk.out_channels, 5, 7), device="cuda", generator=g)
    calls = _counters(monkeypatch)
    H = _step(trunk, x, dy)
    n_blocks = len(trunk.group0) + len(trunk.group1) + len(trunk.group2)
    assert len(calls["join"]) == n_blocks == {18: 6, 50: 13}[depth], "the join route did not run a join per block"
    tracked = [k for k in H if k.endswith("num_batches_tracked")]
    assert tracked and all(int(H[k]) == 1 for k in tracked)
    D = N.trunk(state, x.double(), dy.double(), depth)
    S = N.trunk(state, x, dy, depth)
    for k in tracked:
        assert int(D[k]) == 1, k
    _judge("trunk%d" % depth, H, S, D)
