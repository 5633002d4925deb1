"""Group normalisation (norm_type='GN') without a GPU: the stock-PyTorch stand-ins of rownorm.RowGroupNorm and
backbones.GroupNormAct2d against the f64 reference of tests/groupnorm_reference.py and against the reference project's
own formula; the kernel model of that module inside every counted bound on the whole TABLE, and each seeded defect
outside one by a wide margin; the networks built with 'GN' (sites, group count, no bias, no buffers, decay list), the
'BN' networks' state_dict names unchanged, and the error for any other norm_type."""
import os
import re

import pytest
import torch

import groupnorm_reference as GR
from wssdl_bus_amd.fast_rcnn.config import cfg
from wssdl_bus_amd.networks import backbones, roi_head, rownorm
from wssdl_bus_amd.networks.backbones import RESNET_DEFS
from wssdl_bus_amd.networks.factory_bus import get_network

F64_TOL = 1e-10        # two f64 evaluations of the same formula: relative to the tensor's largest magnitude


def _close(got, want, what):
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got.detach().double() - want.double()).abs().max())
    assert err <= F64_TOL * scale, "%s: max |d| = %g against magnitude %g" % (what, err, scale)


# ---------------------------------------------------------------- the stand-in against the f64 reference
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pos_major", [False, True])
@pytest.mark.parametrize("groups", [1, 4, 8, 32])
def test_row_standin_matches_reference(groups, pos_major, masked):
    S, P, C = 5, 6, 64
    c = GR.make_case(3, S, P, C, "cpu")
    mask = GR.make_mask("random", S, 5, "cpu") if masked else None
    gn = rownorm.RowGroupNorm(C, groups).double()
    with torch.no_grad():
        gn.weight.copy_(c["w"])
        gn.bias.copy_(c["b"])
    x = c["x"].double().requires_grad_(True)
    rownorm.set_roi_mask(mask.double() if masked else None)
    try:
        y = gn(x, S, relu=True, pos_major=pos_major)
        y.backward(c["dy"].double())
    finally:
        rownorm.set_roi_mask(None)
    f = GR.forward(c["x"], c["w"], c["b"], gn.eps, groups, P, True, mask, pos_major)
    _close(y, f["y"], "y")
    b = GR.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], groups, P, f["pre"] > 0, mask, pos_major)
    _close(x.grad, b["dx"], "dx")
    _close(gn.weight.grad, b["dgamma"], "dgamma")
    _close(gn.bias.grad, b["dbeta"], "dbeta")
    if masked:
        dead = GR.to_groups(y.detach(), S, P, groups, pos_major)[mask == 0]
        assert not bool(dead.any()), "y is not zero on dead samples"


@pytest.mark.parametrize("channels_last", [False, True])
def test_trunk_standin_matches_reference(channels_last):
    N, H, W, C, groups = 2, 5, 7, 64, 8
    c = GR.make_case(4, N, H * W, C, "cpu")
    gn = backbones.GroupNormAct2d(C, groups).double()
    with torch.no_grad():
        gn.weight.copy_(c["w"])
        gn.bias.copy_(c["b"])
    x = c["x"].double().view(N, H, W, C).permute(0, 3, 1, 2)
    x = (x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()).requires_grad_(True)
    y = gn(x, relu=True)
    y.backward(c["dy"].double().view(N, H, W, C).permute(0, 3, 1, 2))
    f = GR.forward(c["x"], c["w"], c["b"], gn.eps, groups, H * W, True)
    b = GR.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], groups, H * W, f["pre"] > 0)
    _close(y.permute(0, 2, 3, 1).reshape(-1, C), f["y"], "y")
    _close(x.grad.permute(0, 2, 3, 1).reshape(-1, C), b["dx"], "dx")
    _close(gn.weight.grad, b["dgamma"], "dgamma")
    _close(gn.bias.grad, b["dbeta"], "dbeta")


def test_trunk_module_is_the_reference_formula_interleaved_groups():
    """network.py:528-546 written out: reshape [N, H, W, C] to [N, H, W, C // G, G], moments over axes 1, 2, 3, eps
    1e-5, reshape back, gamma and beta per channel.  The per-channel means span orders of magnitude, so a module that
    grouped contiguous channels would be off by far more than any rounding."""
    N, H, W, C, groups = 2, 4, 6, 64, 8
    g = torch.Generator().manual_seed(11)
    off = 10.0 ** (torch.arange(C, dtype=torch.float64) % 5 - 2)               # 0.01 ... 100
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64) + off
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    out = x.reshape(N, H, W, C // groups, groups)
    mean = out.mean(dim=(1, 2, 3), keepdim=True)
    var = ((out - mean) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    want = ((out - mean) / torch.sqrt(var + 1e-5)).reshape(N, H, W, C) * gamma + beta
    gn = backbones.GroupNormAct2d(C, groups).double()
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
    got = gn(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    _close(got, want, "y")
    other = torch.nn.functional.group_norm(x.permute(0, 3, 1, 2), groups, gamma, beta, 1e-5).permute(0, 2, 3, 1)
    gap = float((other - want).abs().max())
    print("interleaved against contiguous groups: max |d| = %g" % gap)
    assert gap > 0.1, "the input does not tell interleaved from contiguous groups"
    assert gn.eps == 1e-5 and not list(gn.buffers())


# ---------------------------------------------------------------- the kernel model and the bounds
def _model_ratios(S, P, C, relu, pos_major, mask, defect=None, seed=7):
    c = GR.make_case(seed, S, P, C, "cpu")
    x, dy, w, b = c["x"], c["dy"], c["w"], c["b"]
    y, mean, rstd = GR.model_forward(x, w, b, GR.EPS, GR.G, P, relu, mask, pos_major, defect)
    r, f, by = GR.forward_ratios(x, w, b, GR.EPS, GR.G, P, relu, dict(y=y, mean=mean, rstd=rstd), mask, pos_major)
    if defect is None:
        GR.check_gate("model", y, f, by)
    # the backward is judged on its own arithmetic: the sound model's f32 mean / rstd and its gate, as data
    _, ref_mean, ref_rstd = GR.model_forward(x, w, b, GR.EPS, GR.G, P, relu, mask, pos_major)
    gate = (GR.model_forward(x, w, b, GR.EPS, GR.G, P, True, None, pos_major)[0] > 0) if relu else None
    mean_b, rstd_b = (mean, rstd) if defect is None else (ref_mean, ref_rstd)
    if defect == "dead_dgamma":           # the dead samples' rows hold data: give the defect their statistics too
        _, mean_b, rstd_b = GR.model_forward(x, w, b, GR.EPS, GR.G, P, relu, None, pos_major)
    dx, dg, db = GR.model_backward(x, dy, w, b, mean_b, rstd_b, GR.G, P, relu, mask, pos_major, defect)
    rb, _ = GR.backward_ratios(x, dy, w, ref_mean, ref_rstd, GR.G, P, gate, dict(dx=dx, dgamma=dg, dbeta=db), mask,
                               pos_major)
    r.update(rb)
    return r


@pytest.mark.parametrize("pos_major", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("S,P,C", GR.TABLE)
def test_kernel_model_inside_every_bound(S, P, C, relu, pos_major):
    case = "model %dx%dx%d relu=%d pm=%d" % (S, P, C, relu, pos_major)
    GR.check_ratios(case, _model_ratios(S, P, C, relu, pos_major, None))
    if GR.is_small(S, P, C) and S > 1 and relu:
        for kind in GR.MASK_KINDS:
            GR.check_ratios(case + " " + kind, _model_ratios(S, P, C, relu, pos_major, GR.make_mask(kind, S, 3, "cpu")))


@pytest.mark.parametrize("defect", sorted(GR.DEFECTS))
def test_every_seeded_defect_leaves_a_bound(defect):
    S, P, C = 6, 16, 64
    mask = GR.make_mask("random", S, 3, "cpu") if defect == "dead_dgamma" else None
    assert mask is None or 0 < int(mask.sum()) < S
    r = _model_ratios(S, P, C, True, True, mask, defect)
    worst = max(r, key=r.get)
    print("gn-defect %s (%s): worst ratio %.4g at %s; all: %s" % (
        defect, GR.DEFECTS[defect], r[worst], worst, " ".join("%s=%.3g" % kv for kv in sorted(r.items()))))
    assert r[worst] > 100.0, "%s stays inside every bound (worst ratio %.4g)" % (defect, r[worst])


def test_one_value_per_group_has_zero_variance():
    c = GR.make_case(7, 1, 1, 8, "cpu")
    _, _, rstd = GR.model_forward(c["x"], c["w"], c["b"], GR.EPS, GR.G, 1, False)
    f = GR.forward(c["x"], c["w"], c["b"], GR.EPS, GR.G, 1, False)
    assert not bool(f["var"].any())
    _close(f["y"], c["b"].double().view(1, 8), "y = beta")
    assert torch.equal(rstd, torch.full_like(rstd, float(torch.tensor(GR._eps32(GR.EPS) ** -0.5).float())))


def test_table_reaches_every_path():
    geo = {t: GR.geometry(*t) for t in GR.TABLE}
    small = [t for t, g in geo.items() if g[0] == "small"]
    large = [t for t, g in geo.items() if g[0] == "large"]
    assert any(S > GR.GN_SMALL_MAX_WG for S, _, _ in small)                     # the sample loop
    assert any(geo[t][2] > GR.GN_CACHE for t in small)                          # rows past the register budget
    assert any(P * C == GR.GN_SMALL_MAX_FLOATS for _, P, C in small)            # just below the switch
    assert any(GR.GN_SMALL_MAX_FLOATS < P * C <= GR.GN_SMALL_MAX_FLOATS + C for _, P, C in large)
    assert any(geo[t][2] % geo[t][3] for t in large)                            # chunk rows no multiple of the row step
    assert any(geo[t][1] == GR.GN_MAX_CHUNKS and -(-t[1] // (geo[t][3] * GR.GN_CHUNK_STEPS)) > GR.GN_MAX_CHUNKS
               for t in large)                                                  # the cap
    assert any(geo[t][4] == 2 for t in large)                                   # two column passes
    assert all(C % 8 == 0 and C <= GR.GN_MAX_C for _, _, C in GR.TABLE)


def test_geometry_constants_are_those_of_the_source():
    import wssdl_bus_amd
    src = os.path.join(os.path.dirname(wssdl_bus_amd.__file__), "csrc", "plumbing", "groupnorm.hip")
    text = open(src).read()
    for name in ("GN_SMALL_MAX_FLOATS", "GN_BLOCK_SMALL", "GN_BLOCK_LARGE", "GN_SMALL_MAX_WG", "GN_CACHE", "GN_CACHE_BWD",
                 "GN_CHUNK_STEPS", "GN_MAX_CHUNKS", "GN_MAX_C"):
        m = re.search(r"constexpr (?:int|long long) %s = (\d+);" % name, text)
        assert m, name
        assert int(m.group(1)) == getattr(GR, name), name


# ---------------------------------------------------------------- the networks
def _norm_sites(net, depth):
    """(name, module) of every site the reference normalises at, from RESNET_DEFS"""
    defs, block = RESNET_DEFS[depth]
    n_conv = len(block.chain)
    sites = [("trunk.conv0.bn", net.trunk.conv0.bn), ("trunk.norm", net.trunk.norm), ("rpn_conv.bn", net.rpn_conv.bn),
             ("head.norm", net.head.norm)]
    groups = [("trunk.group%d" % i, getattr(net.trunk, "group%d" % i), defs[i], i == 0) for i in range(3)]
    groups.append(("head.group3", net.head.group3, defs[3], False))
    for gname, group, count, first in groups:
        assert len(group) == count
        for i, blk in enumerate(group):
            name = "%s.%d" % (gname, i)
            if not (first and i == 0):
                sites.append((name + ".pre_bn", blk.pre_bn))
            else:
                assert blk.pre_bn is None
            for k in range(1, n_conv + 1):
                sites.append(("%s.conv%d.bn" % (name, k), getattr(blk, "conv%d" % k).bn))
            if blk.short is not None:
                sites.append((name + ".short.bn", blk.short.bn))
    return sites


@pytest.mark.parametrize("name", ["Resnet_train", "Resnet_train_alter"])
@pytest.mark.parametrize("depth", [18, 50])
def test_gn_network_sites(depth, name):
    net = get_network(name, depth, norm_type="GN")
    sites = _norm_sites(net, depth)
    for sname, m in sites:
        assert isinstance(m, rownorm.RowGroupNorm), sname
        assert m.groups == 8 and m.eps == 1e-5, sname
        assert bool((m.weight == 1).all()) and bool((m.bias == 0).all()), sname
    norms = [m for m in net.modules() if isinstance(m, rownorm.RowGroupNorm)]
    assert len(norms) == len(sites)                                       # and nowhere else
    assert not [m for m in net.modules() if isinstance(m, (torch.nn.BatchNorm2d, rownorm.RowBatchNorm))]
    for m in net.modules():
        if isinstance(m, backbones.Conv):
            assert (m.conv.bias is None) == (m.bn is not None)
        if isinstance(m, roi_head.ConvNHWC):
            assert (m.bias is None) == (m.bn is not None)
            assert m.bn is not None
    assert net.trunk.conv0.conv.bias is None and net.rpn_conv.conv.bias is None
    assert net.rpn_cls_score.conv.bias is not None and net.rpn_cls_score.bn is None
    assert not [k for k, _ in net.named_buffers()], "a group-norm network has no buffers"
    assert not [k for k in net.state_dict() if "running_" in k or "num_batches" in k]
    decayed = {id(p) for p in net.weight_decay_params()}
    for sname, m in sites:
        assert id(m.weight) not in decayed and id(m.bias) not in decayed, sname
    assert len(decayed) == sum(isinstance(m, (torch.nn.Conv2d, torch.nn.Linear, roi_head.ConvNHWC))
                               for m in net.modules())


def _bn_state_names(depth):
    """the state_dict of a 'BN' Resnet_train as it has always been, from RESNET_DEFS"""
    defs, block = RESNET_DEFS[depth]
    n_conv, e = len(block.chain), block.expansion
    bn2d = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    rowbn = ["weight", "bias", "running_mean", "running_var"]
    names = ["trunk.conv0.conv.weight", "rpn_conv.conv.weight", "rpn_cls_score.conv.weight", "rpn_cls_score.conv.bias",
             "rpn_bbox_pred.conv.weight", "rpn_bbox_pred.conv.bias", "cls_score.weight", "cls_score.bias",
             "bbox_pred.weight", "bbox_pred.bias"]
    names += ["%s.%s" % (m, k) for m in ("trunk.conv0.bn", "trunk.norm", "rpn_conv.bn") for k in bn2d]
    names += ["head.norm.%s" % k for k in rowbn]
    c_in = 64
    for gi, c_o in enumerate((64, 128, 256, 512)):
        head = gi == 3
        prefix, keys = ("head.group3", rowbn) if head else ("trunk.group%d" % gi, bn2d)
        for i in range(defs[gi]):
            blk = "%s.%d" % (prefix, i)
            if not (gi == 0 and i == 0):
                names += ["%s.pre_bn.%s" % (blk, k) for k in keys]
            convs = ["conv%d" % k for k in range(1, n_conv + 1)] + (["short"] if c_in != c_o * e else [])
            for cv in convs:
                names.append("%s.%s.weight" % (blk, cv) if head else "%s.%s.conv.weight" % (blk, cv))
                names += ["%s.%s.bn.%s" % (blk, cv, k) for k in keys]
            c_in = c_o * e
    return names


@pytest.mark.parametrize("depth", [18, 50])
def test_bn_network_state_dict_names_unchanged(depth):
    net = get_network("Resnet_train", depth, norm_type="BN")
    want = _bn_state_names(depth)
    assert len(want) == len(set(want))
    assert set(net.state_dict()) == set(want), sorted(set(net.state_dict()) ^ set(want))[:8]


def test_unknown_norm_type_is_an_error_and_none_builds_biases():
    with pytest.raises(ValueError):
        get_network("Resnet_train", 18, norm_type="XN")
    with pytest.raises(ValueError):
        backbones.ResNetHead(18, "gn")
    with pytest.raises(ValueError):
        rownorm.make_norm("LN", 64, rows=True)
    assert rownorm.make_norm(None, 64, rows=True) is None and rownorm.make_norm(None, 64, rows=False) is None
    net = get_network("Resnet_train", 18, norm_type=None)
    assert not [m for m in net.modules() if isinstance(m, (torch.nn.BatchNorm2d, rownorm.RowBatchNorm,
                                                           rownorm.RowGroupNorm))]
    for m in net.modules():
        if isinstance(m, backbones.Conv):
            assert m.bn is None and m.conv.bias is not None
        if isinstance(m, roi_head.ConvNHWC):
            assert m.bn is None and m.bias is not None
    assert isinstance(backbones.ResNetHead(18, "GN").norm, backbones.GroupNormAct2d)


def test_group_count_follows_the_config():
    assert cfg.TRAIN.GN_MIN_NUM_G == 8 and cfg.TRAIN.GN_MIN_CHS_PER_G == 4
    assert [rownorm.gn_groups(c) for c in (64, 256, 2048, 16, 4, 3)] == [8, 8, 8, 4, 1, 1]


@pytest.mark.parametrize("depth", [18, 50])
def test_head_forward_backward_cpu_train_equals_eval(depth):
    torch.manual_seed(5)
    head = roi_head.ResNetHeadNHWC(depth, "GN")
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, rownorm.RowGroupNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
            elif isinstance(m, roi_head.ConvNHWC):
                m.weight.mul_(20.0)
    x = torch.randn(3, 7, 7, head.group3[0].conv1.c_i, requires_grad=True)
    y = head.train()(x)
    y.backward(torch.randn_like(y))
    assert y.shape == (3, head.out_features) and bool(torch.isfinite(y).all()) and float(x.grad.abs().sum()) > 0
    for k, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    with torch.no_grad():
        assert torch.equal(head.eval()(x), y)
    # a sample is one RoI: the same RoI alone gives the same output
    with torch.no_grad():
        alone = head(x[1:2])
    assert torch.allclose(alone, y[1:2], rtol=1e-4, atol=1e-5)
