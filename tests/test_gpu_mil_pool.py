"""-m gpu: the MIL term under every pair of the five bag functions (csrc/mil.hip through wssdl_mil_pool_forward /
_backward, wssdl_mil_select, and mil/core.py's wrappers) against the f64 statement of tests/mil_pool_reference.py:
rows and counts exactly the reference's, every value and gradient element inside its counted bound, exact zeros where
the reference has them, identical bits on a second run, for the pairs of the three older functions the bits of the
older exports, and the pair a SolverWrapper was given arriving at every place the MIL term is computed.

The accuracy of the device's expf / log1pf is measured first, as test_gpu_loss_reference.py does, over the grids and
over every argument these cases hand them; it fixes the allowance of the bounds."""
import numpy as np
import pytest
import torch

import loss_reference as R
import mil_pool_reference as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = {}
LIB = {}
_SOME = [(3, 4), (4, 3), (4, 4), (3, 3), (4, 0), (2, 4)]
COMBOS = ([("mixed_k3", s) for s in P.ALL_PAIRS] + [("mixed_k5", s) for s in _SOME]
          + [(n, s) for n in ("bags65_k3", "bags65_k5") for s in [(3, 4), (4, 3)]]
          + [(n, s) for n in ("underflow_k3", "underflow_k5") for s in [(4, 4), (3, 4), (4, 3)]])
_REFS = {}


def _id(combo):
    return "%s-%s-%s" % (combo[0], P.NAMES[combo[1][0]], P.NAMES[combo[1][1]])


def _ref(name, sel):
    """the f64 reference of one case, computed once on the CPU and kept on the device unchanged"""
    key = (name, tuple(sel))
    if key not in _REFS:
        ref = P.reference(P.make_case(name, sel, "cpu"))
        _REFS[key] = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ref.items()}
    return _REFS[key]


def _probe(L, x, which):
    from wssdl_bus_amd import _lib
    y = torch.empty_like(x)
    _lib.check(L.wssdl_loss_libm_probe(_lib.ptr(x), x.numel(), which, _lib.ptr(y), _lib.stream()), "wssdl_loss_libm_probe")
    return y


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    lib = _lib.lib()
    ex, lg = R.lib_grids(DEV)
    R.ALLOW.update(exp=0, log1p=0)                              # provisional: only the cases' arguments are taken here
    args, z1 = [ex], [lg]
    for name, sel in COMBOS:
        ref = _ref(name, sel)
        args.append(ref["args"])
        z1.append(ref["z1"])
    _REFS.clear()                                               # their bounds were made with the provisional allowance
    a, z1 = torch.cat(args).contiguous(), torch.cat(z1).contiguous()
    R.ALLOW.clear()
    we = R.lib_accuracy(_probe(lib, a, 0), torch.exp(a.double()))
    wl = R.lib_accuracy(_probe(lib, z1, 1), torch.log1p(z1.double()))
    print("pool-lib-ulp expf %.3f over %d arguments, log1pf %.3f over %d" % (we[0], a.numel(), wl[0], z1.numel()))
    LIB["set"] = False
    try:
        print("pool-lib-allowance %s" % R.set_allowance(we[0], wl[0]))
        LIB["set"] = True
    except AssertionError as e:
        LIB["error"] = str(e)
        R.ALLOW.update(exp=R.MAX_ALLOWANCE, log1p=R.MAX_ALLOWANCE)
    yield lib
    for k in sorted(LOG):
        print("pool-worst %s %.4g" % (k, LOG[k]))


def test_library_accuracy(L):
    assert LIB["set"], LIB.get("error")


# ---------------------------------------------------------------- the exports

def _stride(c):
    return int(c["col"].stride(0)) if c["logits"].shape[0] > 1 else 1


def _pool(L, c):
    """wssdl_mil_pool_forward / _backward on outputs pre-filled with NaN / -7 -> dict"""
    from wssdl_bus_amd import _lib
    sel = c["sel"]
    logits, col = c["logits"], c["col"]
    Rn, K, nb = logits.shape[0], c["K"], c["n_bags"]
    rows = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    bag_logits = torch.full((nb, K), float("nan"), dtype=torch.float32, device=DEV)
    bag_loss = torch.full((nb,), float("nan"), dtype=torch.float32, device=DEV)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    grad = torch.full_like(logits, float("nan"))
    cw = np.ascontiguousarray(c["cw"].cpu().numpy(), np.float32)
    gl = c["gl"].reshape(1).contiguous()
    _lib.check(L.wssdl_mil_pool_forward(
        _lib.ptr(logits), Rn, K, _lib.ptr(col), _stride(c), float(c["offset"]), _lib.ptr(c["bag_labels"]), nb, sel[0],
        sel[1], _lib.host_ptr(cw), float(c["scale"]), _lib.ptr(loss), _lib.ptr(rows), _lib.ptr(counts),
        _lib.ptr(bag_logits), _lib.ptr(bag_loss), _lib.stream()), "wssdl_mil_pool_forward")
    _lib.check(L.wssdl_mil_pool_backward(
        _lib.ptr(logits), Rn, K, _lib.ptr(col), _stride(c), float(c["offset"]), _lib.ptr(c["bag_labels"]), nb, sel[0],
        sel[1], _lib.ptr(rows), _lib.ptr(counts), _lib.ptr(bag_logits), _lib.host_ptr(cw), float(c["scale"]),
        _lib.ptr(gl), _lib.ptr(grad), _lib.stream()), "wssdl_mil_pool_backward")
    torch.cuda.synchronize()
    return dict(rows=rows, counts=counts, bag_logits=bag_logits, bag_loss=bag_loss, loss=loss[0], grad=grad)


def _old(L, c):
    """wssdl_mil_loss_forward / _backward, the exports the three older functions have always gone through"""
    from wssdl_bus_amd import _lib
    logits, col = c["logits"], c["col"]
    Rn, K, nb = logits.shape[0], c["K"], c["n_bags"]
    rows = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    bag_loss = torch.full((nb,), float("nan"), dtype=torch.float32, device=DEV)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    grad = torch.full_like(logits, float("nan"))
    cw = np.ascontiguousarray(c["cw"].cpu().numpy(), np.float32)
    gl = c["gl"].reshape(1).contiguous()
    _lib.check(L.wssdl_mil_loss_forward(
        _lib.ptr(logits), Rn, K, _lib.ptr(col), _stride(c), float(c["offset"]), _lib.ptr(c["bag_labels"]), nb,
        c["sel"][0], c["sel"][1], _lib.host_ptr(cw), float(c["scale"]), _lib.ptr(loss), _lib.ptr(rows),
        _lib.ptr(bag_loss), _lib.stream()), "wssdl_mil_loss_forward")
    _lib.check(L.wssdl_mil_loss_backward(
        _lib.ptr(logits), Rn, K, _lib.ptr(col), _stride(c), float(c["offset"]), _lib.ptr(c["bag_labels"]), nb,
        _lib.ptr(rows), _lib.host_ptr(cw), float(c["scale"]), _lib.ptr(gl), _lib.ptr(grad), _lib.stream()),
        "wssdl_mil_loss_backward")
    torch.cuda.synchronize()
    return dict(rows=rows, bag_loss=bag_loss, loss=loss[0], grad=grad)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_pool_exports_inside_every_bound(L, combo):
    name, sel = combo
    c = P.make_case(name, sel, DEV)
    ref = _ref(name, sel)
    got = _pool(L, c)
    assert torch.equal(got["rows"].long(), ref["rows"]), "%s: rows differ at bags %s" % (
        _id(combo), (got["rows"].long() != ref["rows"]).nonzero().reshape(-1).tolist()[:8])
    assert torch.equal(got["counts"].long(), ref["counts"]), "%s: counts differ" % _id(combo)
    R.check_ratios(_id(combo), P.ratios(ref, got["loss"], got["bag_loss"], got["grad"], got["bag_logits"]), LOG)
    assert not bool((got["grad"][ref["zero"]] != 0).any()), "%s: gradient where it must be exactly 0" % _id(combo)
    empty = ref["rows"] < 0
    assert not bool(got["bag_logits"][empty].any()) and not bool(got["bag_loss"][empty].any())
    if name.startswith("mixed"):
        assert c["sizes"] == [1, 0, 257, 300] and bool(empty[1]) and int(empty.sum()) == 1


def test_cases_hold_what_they_are_for(L):
    """ties at r, r + 1, r + 256 under the selecting functions; a disc-max key from class 1 and one from class K-1; a
    nearly cancelling mean; p_1 -> 1 and -> 0"""
    for K, name in ((3, "mixed_k3"), (5, "mixed_k5")):
        for sel in (0, 1, 2, 3):
            c = P.make_case(name, (sel, sel), "cpu")
            rows, _, members = P.select(c)
            winners = []
            for b in (2, 3):
                k = P.keys(c["logits"][members[b]], sel)
                r = int(rows[b] - members[b][0])
                assert (k == k.max()).nonzero().squeeze(1).tolist() == [r, r + 1, r + 256]
                winners.append(int(c["logits"][rows[b], 1:].argmax()) + 1)
            if sel == 3:
                assert winners == [1, K - 1]
        c = P.make_case(name, (4, 4), "cpu")
        _, _, members = P.select(c)
        x = c["logits"][members[2], 1].double()
        assert float(x.abs().max()) > 500 and abs(float(x.sum())) < 1.0 and float(x.abs().min()) < 0.01
    c = P.make_case("underflow_k3", (4, 4), "cpu")
    ref = P.reference(c)
    assert ref["bag_logits"][:, 1].abs().min() > 79 and bool((ref["bag_logits"][:, 1] > 0).any()) \
        and bool((ref["bag_logits"][:, 1] < 0).any())


@pytest.mark.parametrize("combo", [("mixed_k3", (4, 3)), ("mixed_k3", (3, 4)), ("mixed_k5", (4, 4)),
                                   ("bags65_k3", (4, 3))], ids=_id)
def test_two_runs_give_identical_bits(L, combo):
    c = P.make_case(combo[0], combo[1], DEV)
    a, b = _pool(L, c), _pool(L, c)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), "%s: %s differs between two runs" % (_id(combo), k)


@pytest.mark.parametrize("name", ["mixed_k3", "mixed_k5", "bags65_k3"])
def test_older_functions_keep_their_bits(L, name):
    """pairs of mal-max, ben-max, mass-max: the new exports against the older ones, bit for bit"""
    for sel in P.OLD_PAIRS:
        c = P.make_case(name, sel, DEV)
        new, old = _pool(L, c), _old(L, c)
        for k in old:
            assert torch.equal(_bits(new[k]), _bits(old[k])), "%s %s: %s differs from the older export's" % (name, sel, k)


def test_older_exports_and_the_two_new_selectors(L):
    """wssdl_mil_select takes 3 and 4 (a mean-ben bag reports its first row, -1 when empty); the older loss pair takes
    disc-max with the new pair's bits and rejects mean-ben"""
    from wssdl_bus_amd import _lib
    c = P.make_case("mixed_k5", (3, 4), DEV)
    ref = _ref("mixed_k5", (3, 4))
    nb = c["n_bags"]
    rows = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.wssdl_mil_select(_lib.ptr(c["logits"]), c["logits"].shape[0], c["K"], _lib.ptr(c["col"]), _stride(c),
                                  float(c["offset"]), _lib.ptr(c["bag_labels"]), nb, 3, 4, _lib.ptr(rows),
                                  _lib.ptr(counts), _lib.stream()), "wssdl_mil_select")
    assert torch.equal(rows.long(), ref["rows"]) and torch.equal(counts.long(), ref["counts"])
    assert rows.tolist()[:3] == [P.FRONT, -1, P.FRONT + 1]                          # bags 0 and 2 pool: their first rows
    c = P.make_case("mixed_k3", (3, 3), DEV)
    new, old = _pool(L, c), _old(L, c)
    for k in old:
        assert torch.equal(_bits(new[k]), _bits(old[k])), k
    cw = np.ascontiguousarray(c["cw"].cpu().numpy(), np.float32)
    out = torch.full((nb + 2,), -7.0, device=DEV)
    irows = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    for sel in ((4, 0), (0, 4), (5, 0), (0, -1)):
        rc = L.wssdl_mil_loss_forward(_lib.ptr(c["logits"]), c["logits"].shape[0], 3, _lib.ptr(c["col"]), 1, 0.0,
                                      _lib.ptr(c["bag_labels"]), nb, sel[0], sel[1], _lib.host_ptr(cw), 1.0,
                                      _lib.ptr(out), _lib.ptr(irows), _lib.ptr(out[1:]), _lib.stream())
        assert rc == _lib.ERR_INVALID_ARGUMENT, sel
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((irows == -7).all())                 # nothing was launched


# ---------------------------------------------------------------- mil/core.py

def _funcs(sel):
    from wssdl_bus_amd.mil import core as M
    return [M.MIL_FUNCS[P.NAMES[sel[0]]], M.MIL_FUNCS[P.NAMES[sel[1]]]]


@pytest.mark.parametrize("combo", [("mixed_k3", (3, 4)), ("mixed_k5", (4, 3)), ("mixed_k5", (4, 4)), ("mixed_k3", (3, 3)),
                                   ("underflow_k5", (4, 4))], ids=_id)
def test_python_layer_fused(L, combo):
    """mil_loss_device under autograd and mil_bag_losses_device"""
    from wssdl_bus_amd.mil import core as M
    name, sel = combo
    c = P.make_case(name, sel, DEV)
    ref = _ref(name, sel)
    x = c["logits"].clone().requires_grad_(True)
    loss = M.mil_loss_device(x, c["col"], c["offset"], c["bag_labels"], c["n_bags"], _funcs(sel), c["cw"].cpu().numpy(),
                             c["scale"])
    (loss * c["gl"]).backward()
    bag = M.mil_bag_losses_device(c["logits"], c["col"], c["offset"], c["bag_labels"], c["n_bags"], _funcs(sel),
                                  c["cw"].cpu().numpy())
    R.check_ratios("python " + _id(combo), {"py_" + k: v for k, v in P.ratios(ref, loss.detach(), bag, x.grad).items()}, LOG)
    assert not bool((x.grad[ref["zero"]] != 0).any())


@pytest.mark.parametrize("combo", [("mixed_k3", (3, 4)), ("mixed_k5", (4, 3)), ("mixed_k5", (4, 4)), ("mixed_k3", (3, 3))],
                         ids=_id)
def test_get_bag_logit_device_values_and_gradient(L, combo):
    from wssdl_bus_amd.mil import core as M
    name, sel = combo
    c = P.make_case(name, sel, DEV)
    ref = _ref(name, sel)
    nb, K = c["n_bags"], c["K"]
    x = c["logits"].clone().requires_grad_(True)
    bag_logits, scale, valid = M.get_bag_logit_device(x, c["col"], c["offset"], c["bag_labels"], nb, _funcs(sel),
                                                     return_valid=True)
    assert torch.equal(valid, ref["rows"] >= 0)
    R.check_ratios("bag_logit " + _id(combo), P.ratios(ref, bag_logits=bag_logits.detach()), LOG)
    want_scale = torch.softmax(ref["bag_logits"], 1).gather(1, c["bag_labels"].long().unsqueeze(1)).squeeze(1)
    assert R.ratio(scale.detach(), want_scale, 16 * R.U) <= 1.0        # a probability: 16 roundings of at most 1
    G = torch.randn((nb, K), generator=torch.Generator().manual_seed(5)).to(DEV)
    (bag_logits * G).sum().backward()
    # the scatter: a selected row takes its bag's G (a copy: exact), every row of a pooled bag G[b, 1] / count in
    # column 1 (one division in f32 or better: u |g|), all else exactly 0
    _, counts, members = P.select(P.make_case(name, sel, "cpu"))
    want = torch.zeros_like(ref["grad"])
    bound = torch.zeros_like(want)
    zero = torch.ones_like(want, dtype=torch.bool)
    for b in range(nb):
        if int(ref["rows"][b]) < 0:
            continue
        if bool(ref["pooled"][b]):
            m = members[b].to(DEV)
            want[m, 1] = float(G[b, 1].double()) / float(counts[b])
            bound[m, 1] = R.SLACK * R.U * abs(float(G[b, 1])) / float(counts[b])
            zero[m, 1] = False
        else:
            want[ref["rows"][b]] = G[b].double()
            zero[ref["rows"][b]] = False
    R.check_ratios("bag_logit grad " + _id(combo), {"bag_logit_grad": R.ratio(x.grad, want, bound)}, LOG)
    assert not bool((x.grad[zero] != 0).any())


@pytest.mark.parametrize("sel", [(3, 4), (4, 3), (4, 4), (3, 3), (2, 4)], ids=lambda s: "%s-%s" % (P.NAMES[s[0]], P.NAMES[s[1]]))
def test_unfused_route_agrees(L, sel):
    """train_bus.mil_loss with cfg.FUSED_LOSS on and off: each inside its own bound of the f64 statement, and the two
    within the sum of the two bounds of each other"""
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.fast_rcnn.config import cfg
    step = 4100
    pct = float(cfg.TRAIN.WS_MAL_PCT)

    def case(device):
        c = P.make_case("mixed_k3", sel, device)
        c["cw"] = torch.tensor([0.0, pct, 1.0 - pct], dtype=torch.float64).float().to(device)
        c["scale"] = float(T._mil_scale(step))
        c["gl"] = torch.tensor(1.0, device=device)
        return c
    c = case(DEV)
    ref = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in P.reference(case("cpu")).items()}
    tol_loss, tol_g = P.host_tolerance(c, ref)
    old = cfg.get("FUSED_LOSS", True)
    out = {}
    try:
        for fused in (True, False):
            cfg.FUSED_LOSS = fused
            x = c["logits"].clone().requires_grad_(True)
            loss = T.mil_loss(x, c["col"], c["bag_labels"], c["n_bags"], step, _funcs(sel))
            loss.backward()
            out[fused] = (loss.detach(), x.grad)
    finally:
        cfg.FUSED_LOSS = old
    r = {"fused_loss": R.ratio(out[True][0], ref["loss"], ref["b_loss"]),
         "fused_grad": R.ratio(out[True][1], ref["grad"], ref["b_grad"]),
         "unfused_loss": R.ratio(out[False][0], ref["loss"], tol_loss),
         "unfused_grad": R.ratio(out[False][1], ref["grad"], tol_g),
         "routes_loss": R.ratio(out[False][0], out[True][0].double(), ref["b_loss"] + tol_loss),
         "routes_grad": R.ratio(out[False][1], out[True][1].double(), ref["b_grad"] + tol_g)}
    R.check_ratios("routes %s" % (sel,), r, LOG)
    for fused in (True, False):
        assert not bool((out[fused][1][ref["zero"]] != 0).any())


# ---------------------------------------------------------------- wiring

@pytest.fixture()
def cfg_guard():
    from wssdl_bus_amd.fast_rcnn.config import cfg
    old = (cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG)
    yield cfg
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG = old


def _net(name, seed):
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(seed)
    return get_network(name, 18).cuda().to(memory_format=torch.channels_last)


def _record(monkeypatch):
    """recording wrappers on train_bus.mil_loss and train_bus._mil_per_image -> the list they append (site, funcs) to"""
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    seen = []
    real_loss, real_per_image = T.mil_loss, T._mil_per_image

    def mil_loss(cls, inds, label, n_bags, step, funcs, counts_host=None):
        seen.append(("mil_loss", list(funcs)))
        return real_loss(cls, inds, label, n_bags, step, funcs, counts_host)

    def per_image(cls, col, label, n, step, funcs):
        seen.append(("per_image", list(funcs)))
        return real_per_image(cls, col, label, n, step, funcs)

    monkeypatch.setattr(T, "mil_loss", mil_loss)
    monkeypatch.setattr(T, "_mil_per_image", per_image)
    return seen


def test_solver_hands_the_pair_to_the_joint_step_and_validate(L, cfg_guard, monkeypatch):
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.mil import core as M
    cfg = cfg_guard
    cfg.SAMPLING_RNG = "device"
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
    net = _net("Resnet_train", 47)
    net.train()
    blobs = synthetic.make_batch(2, 2, 320, 480, seed=47)
    val = [synthetic.make_batch(1, 0, 320, 480, seed=48)]
    seen = _record(monkeypatch)
    pair = [M.get_disc_max_logit, M.get_mean_ben_logit]
    solver = T.SolverWrapper(net, mil_funcs=("disc_max", "mean_ben"))
    losses = solver.train_step_joint(blobs)
    assert bool(torch.isfinite(losses["loss"])) and bool(torch.isfinite(losses["mil_cross_entropy"]))
    out = solver.validate(val)
    assert np.isfinite(out["per_image"]).all()
    assert seen == [("mil_loss", pair), ("per_image", pair)]
    del seen[:]
    plain = T.SolverWrapper(net)
    plain.train_step_joint(blobs)
    plain.validate(val)
    assert seen == [("mil_loss", [M.get_mal_max_logit] * 2), ("per_image", [M.get_mal_max_logit] * 2)]
    solver.check_flags()


def test_solver_hands_the_pair_to_the_weak_half_and_validate(L, cfg_guard, monkeypatch):
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.mil import core as M
    cfg = cfg_guard
    cfg.SAMPLING_RNG = "device"
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
    net = _net("Resnet_train_alter", 49)
    net.train()
    blobs_s = synthetic.make_batch(2, 0, 320, 480, seed=49)
    blobs_ws = synthetic.make_batch(0, 2, 320, 480, seed=50)
    val = [synthetic.make_batch(1, 0, 320, 480, seed=51)]
    seen = _record(monkeypatch)
    pair = [M.get_disc_max_logit, M.get_mean_ben_logit]
    solver = T.SolverWrapper(net, mil_funcs=pair)
    # the weak half alone: the MIL term is the only loss, so what reaches cls_score's weights came through its backward
    mil = solver.weak_backward(blobs_ws)
    assert bool(torch.isfinite(mil))
    w = [p for n, p in net.named_parameters() if n.startswith("cls_score") and p.dim() == 2]
    assert len(w) == 1 and w[0].grad is not None and bool(torch.isfinite(w[0].grad).all()) and bool(w[0].grad.any())
    solver.optimizer.zero_grad(set_to_none=True)
    losses = solver.train_step_alter(blobs_s, blobs_ws)
    assert bool(torch.isfinite(losses["loss"])) and bool(torch.isfinite(losses["mil_cross_entropy"]))
    solver.validate(val)
    assert seen == [("mil_loss", pair), ("mil_loss", pair), ("per_image", pair)]
    del seen[:]
    plain = T.SolverWrapper(net)
    plain.train_step_alter(blobs_s, blobs_ws)
    plain.validate(val)
    default = [M.get_mass_max_logit, M.get_mal_max_logit]
    assert seen == [("mil_loss", default), ("per_image", default)]
    solver.check_flags()
