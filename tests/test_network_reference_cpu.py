"""The f64 network reference and the criterion of tests/network_reference.py, established without a GPU.

1. The tap-sum convolution against F.conv2d in f64 on explicitly padded NCHW input, in both weight layouts, at the
   geometries the networks run (and 5x6, a map that is not square), to 1e-12 relative.
2. The reference in f64 against the modules' CPU routes in f64 (the one route of roi_head.py / backbones.py that uses
   no kernel: stock convolutions, unfold, nn.BatchNorm2d, _RowBatchNormFn): every output, gradient and buffer to 1e-9
   of its scale.  This proves the weight-layout mapping and the reference's reading of the wiring;
   test_gpu_network_reference.py then holds every kernel route to the same reference, which closes the triangle.
   The scale of a tensor is ||D||, for a norm's bias gradient max(||D||, ||D_sib||) (network_reference: such a
   gradient can be zero in exact arithmetic, and 1e-9 of 1e-17 would compare rounding noise).
3. The masked head on the CPU route, garbage in the dead rows, against the reference on the compacted rows.
4. Every seeded defect (a)-(g), evaluated in f32 as a kernel route would be, must put at least one output tensor a
   factor 100 above 16 * floor -- 16 is the largest K the GPU test may use -- or the criterion could not see it.
   Head defects run at 3 RoIs of which 2 are live (n = 98 and 32 rows: the unbiasing n / (n - 1) that defect (e)
   drops is 3e-2 of the variance there, 3e-4 of the buffer after momentum 0.01); (d) runs on the trunk, whose
   conv0 is the only convolution with an odd total padding (7x7 at stride 2: 70 -> 35 and 102 -> 51, 5 each).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import network_reference as N


def _same_pad(size, k, s):
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


@pytest.mark.parametrize("h,w,s,k", [(7, 7, 2, 3), (4, 4, 1, 3), (7, 7, 2, 1), (70, 102, 2, 7), (35, 51, 2, 3),
                                     (5, 6, 1, 3)])
@pytest.mark.parametrize("layout", ["rows", "oihw"])
def test_tap_sum_convolution_equals_conv2d(h, w, s, k, layout):
    g = torch.Generator().manual_seed(h * 100 + k)
    c_i, c_o, n = 5, 7, 3
    x = torch.randn((n, h, w, c_i), dtype=torch.float64, generator=g)
    oihw = torch.randn((c_o, c_i, k, k), dtype=torch.float64, generator=g)
    pt, pb = _same_pad(h, k, s)
    pl, pr = _same_pad(w, k, s)
    if (h, s, k) == (70, 2, 7):
        assert (pt, pb) == (2, 3) and (pl, pr) == (2, 3)     # odd total padding: the odd unit goes after
    want = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), oihw, stride=s).permute(0, 2, 3, 1)
    weight = oihw if layout == "oihw" else oihw.permute(0, 2, 3, 1).reshape(c_o, k * k * c_i)
    net = N._Net({"w": weight}, x, True, None)
    got = net.conv(x, "w", k, s, layout).detach()
    assert got.shape == want.shape == (n, -(-h // s), -(-w // s), c_o)
    assert float((got - want).norm()) <= 1e-12 * float(want.norm())


def _scale(name, D):
    s = float(D[name].double().norm())
    if name.endswith(".bias") and N.is_norm_key(name, D.keys()):
        s = max(s, float(D[name[:-len("bias")] + "weight"].double().norm()))
    return s


def _assert_same(A, D, rel=1e-9):
    assert set(A) == set(D), sorted(set(A) ^ set(D))
    N.check_nonzero(D)
    for name, d in D.items():
        a = A[name]
        assert a.shape == d.shape and a.dtype == d.dtype, name
        if not d.dtype.is_floating_point:
            assert torch.equal(a, d), name
            continue
        err = float((a - d).norm())
        assert err <= rel * _scale(name, D), (name, err, _scale(name, D))


def _head(depth, seed):
    from wssdl_bus_amd.networks import roi_head
    torch.manual_seed(seed)
    return N.prepare(roi_head.ResNetHeadNHWC(depth))


def _trunk(depth, seed):
    from wssdl_bus_amd.networks import backbones
    torch.manual_seed(seed)
    return N.prepare(backbones.ResNetTrunk(depth))


def _module_step(module, x, dy, mask=None):
    from wssdl_bus_amd.networks import roi_head
    xx = x.clone().requires_grad_(True)
    roi_head.set_roi_mask(mask)
    try:
        y = module(xx)
    finally:
        roi_head.set_roi_mask(None)
    (y * dy).sum().backward()
    return N.module_outputs(module, y, xx)


@pytest.mark.parametrize("depth", [18, 50])
def test_head_reference_equals_cpu_route_f64(depth):
    m = _head(depth, depth).double()
    state = copy.deepcopy(m.state_dict())
    c = 256 * m.group3[0].expansion
    x = torch.relu(torch.randn((5, 7, 7, c), dtype=torch.float64))
    dy = torch.randn((5, m.out_features), dtype=torch.float64)
    D = N.head(state, x, dy, depth)
    A = _module_step(m, x, dy)
    _assert_same(A, D)
    # eval mode: the running buffers enter the output and are left alone
    m.eval()
    state = copy.deepcopy(m.state_dict())
    m.zero_grad()
    D = N.head(state, x, dy, depth, training=False)
    A = _module_step(m, x, dy)
    _assert_same(A, D)
    for k, v in state.items():
        if "running" in k:
            assert torch.equal(D["b." + k], v) and torch.equal(A["b." + k], v), k


def test_trunk_reference_equals_cpu_route_f64():
    m = _trunk(18, 18).double()
    state = copy.deepcopy(m.state_dict())
    x = torch.randn((2, 3, 70, 102), dtype=torch.float64)
    dy = torch.randn((2, 256, 5, 7), dtype=torch.float64)
    D = N.trunk(state, x, dy, 18)
    A = _module_step(m, x, dy)
    assert D["y"].shape == (2, 256, 5, 7)
    _assert_same(A, D)
    tracked = [k for k in D if k.endswith("num_batches_tracked")]
    assert len(tracked) == 21 and all(int(D[k]) == 1 for k in tracked)


@pytest.mark.parametrize("depth", [18, 50])
def test_masked_head_on_cpu_route_equals_reference_on_compacted_rows(depth):
    m = _head(depth, 100 + depth).double()
    state = copy.deepcopy(m.state_dict())
    c = 256 * m.group3[0].expansion
    R = 7
    live = torch.tensor([1, 2, 5])
    mask = torch.zeros(R, dtype=torch.float64)
    mask[live] = 1.0
    x = 1e3 * torch.randn((R, 7, 7, c), dtype=torch.float64)           # finite garbage in the dead rows
    x[live] = torch.relu(torch.randn((3, 7, 7, c), dtype=torch.float64))
    dy = torch.randn((R, m.out_features), dtype=torch.float64)          # nonzero on the dead rows too
    D = N.head(state, x, dy, depth, live=live)
    A = _module_step(m, x, dy, mask)
    assert not bool(A["dx"][mask == 0].any())
    A["y"], A["dx"] = A["y"][live], A["dx"][live]
    _assert_same(A, D)


# ---- the seeded defects ----
@pytest.fixture(scope="module")
def head_case():
    m = _head(18, 5)
    state = copy.deepcopy(m.state_dict())
    live = torch.tensor([0, 2])
    x = 1e3 * torch.randn((3, 7, 7, 256))
    x[live] = torch.relu(torch.randn((2, 7, 7, 256)))
    dy = torch.randn((3, 512))
    run = lambda dt, defect=None: N.head(state, x.to(dt), dy.to(dt), 18, defect=defect, live=live)
    return run, run(torch.float32), run(torch.float64)


@pytest.fixture(scope="module")
def trunk_case():
    m = _trunk(18, 6)
    state = copy.deepcopy(m.state_dict())
    x = torch.randn((2, 3, 70, 102))
    dy = torch.randn((2, 256, 5, 7))
    run = lambda dt, defect=None: N.trunk(state, x.to(dt), dy.to(dt), 18, defect=defect)
    return run, run(torch.float32), run(torch.float64)


def test_true_f32_evaluation_is_its_own_floor(head_case, trunk_case):
    for run, S, D in (head_case, trunk_case):
        N.check_nonzero(D)
        r = N.ratios(S, S, D)
        assert max(r.values()) <= 1.0 and len(r) == sum(v.dtype.is_floating_point for v in D.values())
        for k in ("y", "dx"):                                 # the f32 evaluation is an f32-accurate one
            assert float((S[k].double() - D[k]).norm()) <= 1e-5 * float(D[k].norm()), k


@pytest.mark.parametrize("defect", sorted(N.DEFECTS))
def test_criterion_sees_seeded_defect(defect, head_case, trunk_case, request):
    run, S, D = trunk_case if defect == "d" else head_case
    B = run(torch.float32, defect)
    r = N.ratios(B, S, D)
    worst = max(r, key=r.get)
    print("netref-defect (%s) %s: worst ratio %.3g (%s), %d of %d tensors over 16"
          % (defect, N.DEFECTS[defect], r[worst], worst, sum(v > 16 for v in r.values()), len(r)))
    assert r[worst] >= 100 * 16, (defect, worst, r[worst])


def test_padding_defect_cannot_show_in_the_head(head_case):
    """(d) cannot show in the head (7 -> 4 and 4 -> 4 have an even total padding): it is judged on the trunk alone."""
    run, S, D = head_case
    B = run(torch.float32, "d")
    for k in D:
        assert torch.equal(B[k], S[k]), k
