"""-m gpu: the fused losses (csrc/loss.hip through fast_rcnn/loss_op.py; csrc/mil.hip through its exports, the way
mil/core.py calls them) against the plain f64 references of tests/loss_reference.py, computed in torch float64 on the
device: every value and every gradient element inside its bound (counted roundings, see that module), every
exact-zero set exactly zero, the selected MIL rows exactly the reference's.  test_loss_reference_cpu.py shows on the
CPU that a model of the kernels stays inside these bounds and that seeded defects do not.

The tolerances of test_gpu_loss.py, tools/loss_fuzz.py and tools/mil_fuzz.py (1e-5 of the largest element) stand on
this module.  The accuracy of the device's expf / log1pf is measured first, through wssdl_loss_libm_probe (the
functions as the loss kernels get them), and fixes the allowance of the bounds; the module's fixture does the
measuring, so any single test can run alone."""

import numpy as np
import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = {}            # worst |error| / bound per output over the module (printed at the end: pytest -s)
LIB = {}


def _probe(L, x, which):
    from wssdl_bus_amd import _lib
    y = torch.empty_like(x)
    _lib.check(L.wssdl_loss_libm_probe(_lib.ptr(x), x.numel(), which, _lib.ptr(y), _lib.stream()), "wssdl_loss_libm_probe")
    return y


@pytest.fixture(scope="module")
def L():
    """the library, with the allowance of the bounds measured on this device: expf over the grid and over every
    argument the cases hand it (both subtractions of the backward included), log1pf over the grid and the cases' z1"""
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    lib = _lib.lib()
    ex, lg = R.lib_grids(DEV)
    R.ALLOW.update(exp=0, log1p=0)                              # provisional: only the cases' arguments are taken here
    args, z1 = [ex], [lg]
    for name in R.MT_CASES:
        ref = R.mt_reference(R.make_mt_case(name, DEV))
        args.append(ref["args"])
        z1.append(ref["z1"])
    for name in R.MIL_CASES:
        ref = R.mil_reference(R.make_mil_case(name, DEV))
        args.append(ref["args"])
        z1.append(ref["z1"])
    z1 = torch.cat(z1)
    a = torch.cat(args).contiguous()
    R.ALLOW.clear()
    we = R.lib_accuracy(_probe(lib, a, 0), torch.exp(a.double()))
    wl = R.lib_accuracy(_probe(lib, z1, 1), torch.log1p(z1.double()))
    LIB.update(exp=we, log1p=wl)
    print("loss-lib-ulp expf %.3f over %d arguments (subnormal results: %.3f, flushed to zero %d)" % (we[0], a.numel(), we[1], we[2]))
    print("loss-lib-ulp log1pf %.3f over %d arguments (subnormal results: %.3f, flushed to zero %d)" % (wl[0], z1.numel(), wl[1], wl[2]))
    LIB["set"] = False
    try:
        print("loss-lib-allowance %s" % R.set_allowance(we[0], wl[0]))
        LIB["set"] = True
    except AssertionError as e:                                  # reported by test_library_accuracy; bounds at the cap
        LIB["error"] = str(e)
        R.ALLOW.update(exp=R.MAX_ALLOWANCE, log1p=R.MAX_ALLOWANCE)
    yield lib
    for k in sorted(LOG):
        print("loss-worst %s %.4g" % (k, LOG[k]))


def test_library_accuracy(L):
    """expf and log1pf of the device within MAX_ALLOWANCE - 1 ulp of f64 on normal results; a subnormal result is
    within the same allowance of its own grid (2^-149) or flushed to zero"""
    assert LIB["set"], LIB.get("error")
    for name in ("exp", "log1p"):
        worst, worst_sub, _ = LIB[name]
        assert worst_sub <= R.ALLOW[name], "%sf: a subnormal result is %.3g units of 2^-149 off" % (name, worst_sub)


def _run_mt(c):
    from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss
    leaves = [c[k].clone().requires_grad_(True) for k in ("rpn_cls", "rpn_box", "cls", "box")]
    rpn_data = (c["rpn_labels"], c["rpn_tg"], c["rpn_inw"], c["rpn_outw"])
    roi_data = (torch.zeros((c["n_rows"], 5), device=DEV), c["labels"], c["tg"], c["inw"], c["outw"])
    terms = multi_task_loss(*leaves, rpn_data, roi_data, c["dims"][4])
    (terms * c["gl"]).sum().backward()
    return terms.detach(), dict(zip(("rpn_cls", "rpn_box", "cls", "box"), (x.grad for x in leaves)))


@pytest.mark.parametrize("name", list(R.MT_CASES))
def test_multi_task_loss_inside_every_bound(L, name):
    c = R.make_mt_case(name, DEV)
    ref = R.mt_reference(c)
    assert (ref["sub"] > 0) == (name == "underflow"), "%s holds %d subnormal exp results" % (name, ref["sub"])
    terms, grads = _run_mt(c)
    zeros = R.mt_zero_violations(ref, grads)
    R.check_ratios(name, R.mt_ratios(ref, terms, grads), LOG)
    assert not any(zeros.values()), "%s: elements that must be exactly 0 are not: %s" % (name, zeros)
    if c["n_rows"] == 0:
        assert bool(torch.isnan(terms[2])) and bool(torch.isfinite(terms[[0, 1, 3]]).all())
        assert not bool(grads["cls"].any()) and not bool(grads["box"].any())


def _mil_forward_backward(L, c):
    """wssdl_mil_loss_forward / _backward as mil/core.py's _MilLoss calls them -> rows, bag_loss, loss, grad"""
    from wssdl_bus_amd import _lib
    logits, col = c["logits"].contiguous(), c["col"]
    Rn, K, nb = logits.shape[0], c["K"], c["n_bags"]
    stride = col.stride(0) if Rn > 1 else 1
    rows = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    bag_loss = torch.full((nb,), float("nan"), dtype=torch.float32, device=DEV)
    loss = torch.empty((1,), dtype=torch.float32, device=DEV)
    grad = torch.full_like(logits, float("nan"))
    cw = np.ascontiguousarray(c["cw"].cpu().numpy(), np.float32)
    gl = c["gl"].reshape(1).contiguous()
    _lib.check(L.wssdl_mil_loss_forward(
        _lib.ptr(logits), Rn, K, _lib.ptr(col), int(stride), float(c["offset"]), _lib.ptr(c["bag_labels"]), nb,
        c["sel"][0], c["sel"][1], _lib.host_ptr(cw), float(c["scale"]), _lib.ptr(loss), _lib.ptr(rows),
        _lib.ptr(bag_loss), _lib.stream()), "wssdl_mil_loss_forward")
    _lib.check(L.wssdl_mil_loss_backward(
        _lib.ptr(logits), Rn, K, _lib.ptr(col), int(stride), float(c["offset"]), _lib.ptr(c["bag_labels"]), nb,
        _lib.ptr(rows), _lib.host_ptr(cw), float(c["scale"]), _lib.ptr(gl), _lib.ptr(grad), _lib.stream()),
        "wssdl_mil_loss_backward")
    torch.cuda.synchronize()
    return rows, bag_loss, loss[0], grad


@pytest.mark.parametrize("name", list(R.MIL_CASES))
def test_mil_loss_inside_every_bound(L, name):
    c = R.make_mil_case(name, DEV)
    ref = R.mil_reference(c)
    assert (ref["sub"] > 0) == (name == "underflow"), "%s holds %d subnormal exp results" % (name, ref["sub"])
    rows, bag_loss, loss, grad = _mil_forward_backward(L, c)
    assert torch.equal(rows.long(), ref["rows"]), "%s: selected rows differ at bags %s" % (
        name, (rows.long() != ref["rows"]).nonzero().reshape(-1).tolist()[:8])
    R.check_ratios("mil " + name, R.mil_ratios(ref, loss, bag_loss, grad), LOG)
    assert not bool((grad[ref["zero"]] != 0).any()), "%s: gradient outside the selected rows" % name


@pytest.mark.parametrize("name", ["five_alt", "bags65"])         # one per selector pair: alternating, combined
def test_mil_loss_device_under_autograd(L, name):
    from wssdl_bus_amd.mil import core as M
    c = R.make_mil_case(name, DEV)
    ref = R.mil_reference(c)
    funcs = {0: M.get_mal_max_logit, 1: M.get_ben_max_logit, 2: M.get_mass_max_logit}
    x = c["logits"].clone().requires_grad_(True)
    loss = M.mil_loss_device(x, c["col"], c["offset"], c["bag_labels"], c["n_bags"],
                             [funcs[c["sel"][0]], funcs[c["sel"][1]]], c["cw"].cpu().numpy(), c["scale"])
    (loss * c["gl"]).backward()
    r = R.mil_ratios(ref, loss.detach(), ref["bag_loss"], x.grad)
    del r["mil_bag_loss"]                                          # not visible through the autograd op
    R.check_ratios("mil autograd " + name, {"auto_" + k: v for k, v in r.items()}, LOG)
    assert not bool((x.grad[ref["zero"]] != 0).any())
