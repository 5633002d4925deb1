"""CPU only: batch renormalisation (cfg.TRAIN.USE_BRN) on the stock-PyTorch route of the 'BN' modules
(networks/rownorm.py: stock_rows / renorm_step; RowBatchNorm and backbones.BatchNormAct2d built with renorm=True)
against the f64 statement of tests/renorm_reference.py, and the switch itself.

The modules run in float64 with eps and momentum set to the f32 values the fused entry points would receive, so the only differences from the reference are f64 roundings; every output is nevertheless held to the
reference's f32-counted bounds (the same ones the GPU tests use), and each seeded defect of renorm_reference.DEFECTS
must break at least one of those bounds on the same inputs:

    u   warm state (W = 0.875) and step 2 of a fresh layer           r, d, y
    w   warm state                                                    dweight
    a   warm state                                                    dx
    n   any step (n / (n - 1) = 1.0039 at 259 rows, times m = 0.01)   running_var
    e   any step (eps = 1e-3 times m = 0.01)                          running_var

(On step 1 of a fresh layer r = 1 and d = 0 whichever state they are formed from: defect u is invisible there, which
is why the fresh sequence is judged at step 2.)
"""
import copy

import pytest
import torch

import renorm_reference as N
import rowbn_reference as R
from wssdl_bus_amd.fast_rcnn.config import cfg
from wssdl_bus_amd.networks import backbones, roi_head, rownorm

EPS, MOM, RHO = R._eps32(1e-3), N._f32(0.01), 0.99
M_ROIS, PER, C = 37, 7, 16                      # 259 rows
LAYOUTS = {"plain": (False, False), "roi_major": (True, False), "pos_major": (True, True)}


@pytest.fixture
def use_brn():
    old = cfg.TRAIN.USE_BRN
    cfg.TRAIN.USE_BRN = True
    yield
    cfg.TRAIN.USE_BRN = old


def _module(case, state=None):
    bn = rownorm.RowBatchNorm(C, eps=EPS, momentum=MOM, renorm=True).double()
    bn.renorm_momentum = RHO
    with torch.no_grad():
        bn.weight.copy_(case["w"])
        bn.bias.copy_(case["b"])
        bn.running_mean.copy_(case["rm"])
        bn.running_var.copy_(case["rv"])
        if state is not None:
            for k in ("mean", "stddev", "weight"):
                getattr(bn, "renorm_" + k).copy_(state[k])
    return bn.train()


def _state_of(bn):
    return {k: getattr(bn, "renorm_" + k).detach().clone() for k in ("mean", "stddev", "weight")}


def _step(bn, c, relu, mask, pos_major, log, case):
    """one training step of the module on batch c against the reference from the module's own state before it"""
    state, rm0, rv0 = _state_of(bn), bn.running_mean.clone(), bn.running_var.clone()
    x = c["x"].double().requires_grad_(True)
    rownorm.set_roi_mask(mask.double() if mask is not None else None)
    try:
        y = bn(x, relu=relu, pos_major=pos_major)
    finally:
        rownorm.set_roi_mask(None)
    bn.zero_grad()
    y.backward(c["dy"].double())
    f = N.forward(c["x"], c["w"], c["b"], EPS, relu, state, rm0, rv0, MOM, RHO, mask, PER, pos_major)
    b = N.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], f["r"], f["d"], (f["pre"] > 0) if relu else None,
                   mask, PER, pos_major)
    bs, (bm, bv) = N.bound_state(f), N.bound_running(f)
    ratios = {"y": R.ratio(y.detach(), f["y"], N.bound_y(c["x"], f)),
              "running_mean": R.ratio(bn.running_mean, f["rm"], bm), "running_var": R.ratio(bn.running_var, f["rv"], bv)}
    for k in ("mean", "stddev", "weight"):
        ratios["renorm_" + k] = R.ratio(getattr(bn, "renorm_" + k), f["state"][k], bs[k])
    ratios.update(N.backward_ratios(c["x"], b, dict(dx=x.grad, dweight=bn.weight.grad, dbias=bn.bias.grad)))
    R.check_ratios(case, ratios, log)
    return f, b


def _mask(layout, seed):
    return R.make_mask("random", M_ROIS, seed) if LAYOUTS[layout][0] else None


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_stock_route_three_steps(layout, relu):
    steps = N.make_steps(11, M_ROIS * PER, C)
    bn = _module(steps[0])
    for i, c in enumerate(steps):
        _step(bn, c, relu, _mask(layout, i), LAYOUTS[layout][1], None, "%s relu=%d step %d" % (layout, relu, i + 1))
    assert float(bn.renorm_weight[0]) == pytest.approx(1.0 - RHO ** 3, rel=1e-12)
    assert torch.equal(bn.renorm_weight, bn.renorm_weight[0].expand(C))


@pytest.mark.parametrize("weight", [0.0, 0.01, 0.875, 1.0])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_stock_route_warm_state(layout, weight):
    c = N.make_steps(5, M_ROIS * PER, C)[1]
    bn = _module(c, N.warm_state(C, weight, 3))
    f, _ = _step(bn, c, True, _mask(layout, 2), LAYOUTS[layout][1], None, "%s W=%g" % (layout, weight))
    assert float((f["r"] - 1).abs().max()) > 0.2 and float(f["d"].abs().max()) > 0.2      # far from 1 and 0


def test_all_dead_rows_follow_the_arithmetic():
    """n clamped to 1, mu = v = 0: y = 0 everywhere, the state moves towards (0, sqrt(eps), 1)"""
    c = N.make_steps(5, M_ROIS * PER, C)[0]
    bn = _module(c, N.warm_state(C, 0.875, 4))
    mask = torch.zeros((M_ROIS,))
    f, _ = _step(bn, c, True, mask, True, None, "all dead")
    assert float(f["y"].abs().max()) == 0.0 and f["count"] == 1.0


def test_first_step_of_a_fresh_layer_is_plain_batch_norm():
    c = N.make_steps(3, M_ROIS * PER, C)[0]
    bn = _module(c)
    plain = rownorm.RowBatchNorm(C, eps=EPS, momentum=MOM).double().train()
    with torch.no_grad():
        plain.weight.copy_(c["w"])
        plain.bias.copy_(c["b"])
    outs = []
    for m in (bn, plain):
        x = c["x"].double().requires_grad_(True)
        y = m(x, relu=True)
        y.backward(c["dy"].double())
        outs.append((y, x.grad, m.weight.grad, m.bias.grad))
    for a, b in zip(*outs):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-13)


def _defect_ratios(c, state, defects, relu=True):
    rm0, rv0 = c["rm"], c["rv"]
    f = N.forward(c["x"], c["w"], c["b"], EPS, relu, state, rm0, rv0, MOM, RHO)
    g = N.forward(c["x"], c["w"], c["b"], EPS, relu, state, rm0, rv0, MOM, RHO, defects=defects)
    gate = (f["pre"] > 0) if relu else None
    b = N.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], f["r"], f["d"], gate)
    h = N.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], f["r"], f["d"], gate, defects=defects)
    out = N.forward_ratios(c["x"], f, g, g["state"], g["rm"], g["rv"])
    out.update(N.backward_ratios(c["x"], b, h))
    return out


@pytest.mark.parametrize("defect,where", [("u", ("r", "d", "y")), ("w", ("dweight",)), ("a", ("dx",)),
                                          ("n", ("running_var",)), ("e", ("running_var",))])
def test_seeded_defects_break_their_bounds_on_the_warm_inputs(defect, where):
    c = N.make_steps(5, M_ROIS * PER, C)[1]
    ratios = _defect_ratios(c, N.warm_state(C, 0.875, 3), defect)
    print("renorm-defect %s (%s): %s" % (defect, N.DEFECTS[defect], {k: "%.3g" % v for k, v in ratios.items()}))
    for name in where:
        assert ratios[name] > 1.0, "defect %s stays inside the bound of %s (%.3g)" % (defect, name, ratios[name])
    clean = _defect_ratios(c, N.warm_state(C, 0.875, 3), "")
    assert max(clean.values()) == 0.0


def test_defect_u_shows_at_step_two_of_a_fresh_layer_not_at_step_one():
    steps = N.make_steps(11, M_ROIS * PER, C)
    assert max(_defect_ratios(steps[0], N.fresh_state(C), "u", relu=False)[k] for k in ("r", "d", "y")) < 1.0
    f = N.forward(steps[0]["x"], steps[0]["w"], steps[0]["b"], EPS, False, N.fresh_state(C), steps[0]["rm"],
                  steps[0]["rv"], MOM, RHO)
    state2 = {k: v.float() for k, v in f["state"].items()}
    ratios = _defect_ratios(steps[1], state2, "u", relu=False)
    assert min(ratios[k] for k in ("r", "d", "y")) > 1.0, ratios


def test_nchw_module_matches_the_reference(use_brn):
    """backbones.BatchNormAct2d in renorm mode on its stock route: an [N, C, H, W] tensor is its [N*H*W, C] rows"""
    steps = N.make_steps(23, 2 * 5 * 7, C)
    bn = rownorm.make_norm("BN", C, rows=False).double().train()
    assert isinstance(bn, backbones.BatchNormAct2d) and bn.renorm
    bn.eps, bn.momentum, bn.renorm_momentum = EPS, MOM, RHO
    with torch.no_grad():
        bn.weight.copy_(steps[0]["w"])
        bn.bias.copy_(steps[0]["b"])
    for i, c in enumerate(steps):
        state, rm0, rv0 = _state_of(bn), bn.running_mean.clone(), bn.running_var.clone()
        x = c["x"].double().view(2, 5, 7, C).permute(0, 3, 1, 2).requires_grad_(True)
        y = bn(x, relu=True)
        bn.zero_grad()
        y.backward(c["dy"].double().view(2, 5, 7, C).permute(0, 3, 1, 2))
        f = N.forward(c["x"], c["w"], c["b"], EPS, True, state, rm0, rv0, MOM, RHO)
        b = N.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], f["r"], f["d"], f["pre"] > 0)
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
        bm, bv = N.bound_running(f)
        ratios = {"y": R.ratio(rows(y.detach()), f["y"], N.bound_y(c["x"], f)),
                  "running_mean": R.ratio(bn.running_mean, f["rm"], bm), "running_var": R.ratio(bn.running_var, f["rv"], bv)}
        ratios.update(N.backward_ratios(c["x"], b, dict(dx=rows(x.grad), dweight=bn.weight.grad, dbias=bn.bias.grad)))
        R.check_ratios("nchw step %d" % (i + 1), ratios)
        assert int(bn.num_batches_tracked) == i + 1


def test_eval_mode_ignores_the_renorm_state():
    c = N.make_steps(3, M_ROIS * PER, C)[0]
    a, b = _module(c, N.warm_state(C, 0.875, 1)).eval(), _module(c, N.warm_state(C, 0.01, 2)).eval()
    plain = rownorm.RowBatchNorm(C, eps=EPS, momentum=MOM).double().eval()
    plain.load_state_dict({k: v for k, v in a.state_dict().items() if not k.startswith("renorm_")})
    x = c["x"].double()
    before = copy.deepcopy(a.state_dict())
    assert torch.equal(a(x, relu=True), b(x, relu=True)) and torch.equal(a(x, relu=True), plain(x, relu=True))
    assert all(torch.equal(v, before[k]) for k, v in a.state_dict().items())


def test_switch_off_keeps_todays_state_dict_keys():
    assert cfg.TRAIN.USE_BRN is False
    for net in (backbones.ResNetTrunk(18), roi_head.ResNetHeadNHWC(18), backbones.ResNetHead(18)):
        keys = list(net.state_dict().keys())
        assert not any("renorm" in k for k in keys)
        norms = [m for m in net.modules() if rownorm.is_bn(m) and hasattr(m, "running_mean")]
        assert norms and not any(m.renorm for m in norms)
        assert all(k.rsplit(".", 1)[-1] in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
                   for k in keys)


def test_make_norm_honours_the_switch(use_brn):
    for rows, cls in ((True, rownorm.RowBatchNorm), (False, backbones.BatchNormAct2d)):
        bn = rownorm.make_norm("BN", 32, rows=rows)
        assert isinstance(bn, cls) and bn.renorm and bn.renorm_momentum == 0.99
        for k in ("renorm_mean", "renorm_stddev", "renorm_weight"):
            assert k in bn.state_dict() and bn.state_dict()[k].shape == (32,) and not bn.state_dict()[k].any()
        assert rownorm.is_bn(bn)
    assert isinstance(rownorm.make_norm("GN", 32, rows=True), rownorm.RowGroupNorm)
    assert rownorm.make_norm(None, 32, rows=True) is None
    trunk = backbones.ResNetTrunk(18)
    n_bn = sum(isinstance(m, backbones.BatchNormAct2d) for m in trunk.modules())
    cfg.TRAIN.USE_BRN = False
    plain_keys = list(backbones.ResNetTrunk(18).state_dict().keys())
    assert len(trunk.state_dict()) == len(plain_keys) + 3 * n_bn
    cfg.TRAIN.USE_BRN = True
    assert not any("renorm" in k for k in backbones.VGGTrunk().state_dict())        # no norms: untouched by the switch


def test_networks_train_on_the_stock_route(use_brn):
    """ResNet-18 trunk and head with the switch on, CPU: two steps run, every renorm layer stepped exactly twice"""
    torch.manual_seed(0)
    trunk = backbones.ResNetTrunk(18).to(memory_format=torch.channels_last).train()
    head = roi_head.ResNetHeadNHWC(18).train()
    for _ in range(2):
        t = trunk(torch.randn(2, 3, 64, 96).contiguous(memory_format=torch.channels_last))
        h = head(torch.randn(5, 7, 7, 256))
        (t.square().mean() + h.square().mean()).backward()
    want = 1.0 - 0.99 ** 2
    for net in (trunk, head):
        for m in net.modules():
            if rownorm.is_bn(m) and hasattr(m, "running_mean"):
                assert m.renorm and torch.allclose(m.renorm_weight, torch.full_like(m.renorm_weight, want), rtol=1e-5)
                assert torch.isfinite(m.running_var).all() and m.weight.grad is not None
