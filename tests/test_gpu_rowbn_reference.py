"""-m gpu: every entry point of the row batch norm (csrc/plumbing/rowbn.hip through networks/_plumbing.py) against
the plain f64 references of tests/rowbn_reference.py, computed in torch float64 on the device, each output inside
its elementwise bound (counted roundings, see that module; test_rowbn_reference_cpu.py shows on the CPU that a model
of the kernels stays inside them and that seeded defects do not).

The other suites compare these entry points with one another bit for bit; this one is what they all stand on.
Shapes are the smallest that reach each path of rowbn.hip (rowbn_reference.TABLE).  The backward is judged on its
own arithmetic: it takes the kernel's f32 mean / rstd, and its ReLU gate (bit-identical to y_kernel > 0, the kernels
recompute fma(x, scale, shift) > 0) as data, while the forward test checks that gate against f64 wherever |y64|
exceeds its bound -- so no element is left out of any comparison.  The joins are judged in stages: out against f64
of (x3, other); the next norm against f64 of the kernel's own out; g against f64 of (out, dy, dres, stats_n); the
input gradients against f64 of the kernel's own g.  Every forward call also updates running statistics, checked
against the once-rounded f64 formula exactly."""
import functools

import pytest
import torch

import rowbn_reference as R

pytestmark = pytest.mark.gpu

EPS = 1e-3
DEV = "cuda"
LOG = {}            # worst |error| / bound per output over the module (printed at the end: pytest -s)


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    from wssdl_bus_amd.networks import _plumbing
    assert _plumbing.lib() is not None, "plumbing library not built"
    yield _plumbing
    for k in sorted(LOG):
        print("rowbn-worst %s %.4g" % (k, LOG[k]))


@functools.lru_cache(maxsize=3)
def _case(seed, M, C):
    return R.make_case(seed, M, C, DEV)


@functools.lru_cache(maxsize=8)
def _mask(kind, n_rois):
    return R.make_mask(kind, n_rois, n_rois, DEV)


def _running(c, mom):
    return c["rm"].clone(), c["rv"].clone(), mom, torch.tensor([5], dtype=torch.int64, device=DEV)


def _check_running(case, c, run, stats, n):
    rm, rv = R.running(c["rm"], c["rv"], stats[0], stats[1], n, run[2])
    assert torch.equal(run[0], rm), "%s: running_mean differs from the formula, max |d| = %g" % (
        case, float((run[0] - rm).abs().max()))
    assert torch.equal(run[1], rv), "%s: running_var differs from the formula, max |d| = %g" % (
        case, float((run[1] - rv).abs().max()))
    assert int(run[3]) == 6, "%s: num_batches_tracked advanced by %d" % (case, int(run[3]) - 5)


def _layer(P, case, c, relu, mask, per, pm, mom):
    """one forward and backward of the layer, every output against its bound"""
    x, w, b, dy = c["x"], c["w"], c["b"], c["dy"]
    run = _running(c, mom)
    y, stats, count = P.rowbn_forward(x, w, b, EPS, relu, mask, pm, running=run)
    r, f, by = R.forward_ratios(x, w, b, EPS, relu, R.stats_dict(stats, y), mask, per, pm)
    R.check_ratios(case, r, LOG)
    R.check_gate(case, y, f, by)
    n, live = f["count"], f["live"]
    del f, by
    if mask is None:
        assert count is None, "%s: a count without a mask" % case
    else:
        assert float(count[0]) == n, "%s: count %g, live rows %g" % (case, float(count[0]), n)
        assert not bool(y[~live].any()), "%s: y is not zero on dead rows" % case
    _check_running(case, c, run, stats, n)
    gate = (y > 0) if relu else None
    dx, dw, db = P.rowbn_backward(x, dy, w, stats, relu, mask, pm)
    rb, _ = R.backward_ratios(x, dy, w, stats[0], stats[2], gate, dict(dx=dx, dweight=dw, dbias=db), mask, per, pm)
    R.check_ratios(case, rb, LOG)
    if mask is not None:
        assert not bool(dx[~live].any()), "%s: dx is not zero on dead rows" % case
    return y, stats, (dx, dw, db)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", R.TABLE)
def test_plain_forward_backward_apply(P, M, C, relu):
    c = _case(21, M, C)
    case = "plain %dx%d relu=%d" % (M, C, relu)
    y, stats, _ = _layer(P, case, c, relu, None, 1, False, 0.01 if relu else 1.0)
    if M == 1:
        assert not bool(stats[1].any()), "%s: one row, var is not 0" % case
    ya = P.rowbn_apply(c["x"], stats[3], stats[4], relu)
    ref = c["x"].double() * stats[3].double() + stats[4].double()
    bd = R.bound_apply(ref)
    R.check(case, "apply", ya, ref.clamp_min(0.0) if relu else ref, bd, LOG)
    assert torch.equal(ya, y), "%s: rowbn_apply with the layer's scale / shift differs from the layer's y" % case


@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("kind", R.MASK_KINDS)
@pytest.mark.parametrize("C", [256, 2048])
@pytest.mark.parametrize("n_rois,per", R.MASK_SPLITS)
def test_masked_both_layouts(P, n_rois, per, C, kind, pm):
    c = _case(22, n_rois * per, C)
    mask = _mask(kind, n_rois)
    case = "masked %dx%d C=%d %s pm=%d" % (n_rois, per, C, kind, pm)
    y, stats, (dx, dw, db) = _layer(P, case, c, True, mask, per, pm, 1.0 if pm else 0.01)
    if kind == "all_dead":
        assert not bool(stats[0].any()) and not bool(stats[1].any()), "%s: mean / var not 0" % case
        assert not bool(dw.any()) and not bool(db.any()), "%s: dweight / dbias not 0" % case
    if kind == "one_live" and per == 1:
        assert not bool(stats[1].any()), "%s: one live row, var is not 0" % case


@pytest.mark.parametrize("kind", ["none", "random"])
@pytest.mark.parametrize("C", [256, 1024])
@pytest.mark.parametrize("n_rois", [37, 301])
def test_entry_gradient(P, n_rois, C, kind):
    plan = P.tap_plan(7, 7, 2)
    per, ns = 49, len(plan.slots)
    c = _case(23, n_rois * per, C)
    dys = R.make_case(24, ns * n_rois, C, DEV)["dy"]
    possel = plan.subsample_slots(7, 7, 2, c["x"].device)
    mask = None if kind == "none" else _mask(kind, n_rois)
    case = "entry %dx49 C=%d mask=%s" % (n_rois, C, kind)
    assert int((possel >= 0).sum()) == ns, "%s: %d slots in possel, %d in the plan" % (case, int((possel >= 0).sum()), ns)
    x, w = c["x"], c["w"]
    y, stats, _ = P.rowbn_forward(x, w, c["b"], EPS, True, mask)
    dx, dw, db = P.rowbn_backward_entry(x, c["dy"], dys, possel, ns, w, stats, mask)
    rb = R.entry_ratios(x, c["dy"], dys, possel, n_rois, w, stats[0], stats[2], y > 0,
                        dict(dx=dx, dweight=dw, dbias=db), mask)
    R.check_ratios(case, rb, LOG)
    if mask is not None:
        assert not bool(dx[~R.row_live(mask, n_rois * per, per)].any()), "%s: dx is not zero on dead rows" % case


def _join(P, case, M, n_rois, C, dual, with_dres, kind, seed=25, nhw=None):
    c3, co, cn = _case(seed, M, C), R.make_case(seed + 1, M, C, DEV), R.make_case(seed + 2, M, C, DEV)
    x3, other = c3["x"], co["x"]
    if nhw is not None:             # the trunk's rows: a channels-last NCHW map viewed as [N*H*W, C]
        nchw = x3.view(*nhw, C).permute(0, 3, 1, 2)
        assert nchw.is_contiguous(memory_format=torch.channels_last), "%s: not a channels-last map" % case
        x3 = nchw.permute(0, 2, 3, 1).reshape(-1, C)
        assert x3.data_ptr() == c3["x"].data_ptr(), "%s: the row view copied" % case
    bn3, bnn = (c3["w"], c3["b"], EPS), (cn["w"], cn["b"], EPS)
    bns = (co["w"], co["b"], 1e-5) if dual else None
    mask = None if kind == "none" else _mask(kind, n_rois)
    live = R.row_live(mask, M, M // n_rois, True)
    runs = [_running(c3, 0.01), _running(co, 1.0) if dual else None, _running(cn, 1.0)]
    out, y, s3, ss, sn, count = P.rowbn_join_forward(x3, bn3, other, bns, bnn, mask, running=runs)
    r, fn, byn = R.join_forward_ratios(x3, bn3, other, bns, bnn, mask, out, y, R.stats_dict(s3),
                                       R.stats_dict(ss) if dual else None, R.stats_dict(sn))
    R.check_ratios(case, r, LOG)
    R.check_gate(case, y, fn, byn)
    n = fn["count"]
    if mask is None:
        assert count is None, "%s: a count without a mask" % case
    else:
        assert float(count[0]) == n, "%s: count %g, live rows %g" % (case, float(count[0]), n)
        assert torch.equal(out[~live], other[~live] if not dual else torch.zeros_like(out[~live])), \
            "%s: out on dead rows" % case
        assert not bool(y[~live].any()), "%s: y is not zero on dead rows" % case
    for cc, run, st in ((c3, runs[0], s3), (co, runs[1], ss), (cn, runs[2], sn)):
        if run is not None:
            _check_running(case, cc, run, st, n)
    del fn, byn

    dy, dres = cn["dy"], (cn["dres"] if with_dres else None)
    xs, ws = (other, co["w"]) if dual else (None, None)
    g, dx3, dxs, dwbn, dwb3, dwbs = P.rowbn_join_backward(out, dy, dres, x3, xs, cn["w"], sn, c3["w"], s3, ws,
                                                          ss if dual else None, mask)
    r = R.join_backward_ratios(out, dy, dres, x3, xs, cn["w"], sn, c3["w"], s3, ws, ss if dual else None, y > 0, mask,
                               g, dx3, dxs, dwbn, dwb3, dwbs)
    R.check_ratios(case, r, LOG)
    if mask is not None:
        assert torch.equal(g[~live], dres[~live] if with_dres else torch.zeros_like(g[~live])), \
            "%s: g on dead rows" % case
        assert not bool(dx3[~live].any()) and (dxs is None or not bool(dxs[~live].any())), \
            "%s: dx is not zero on dead rows" % case


# dead_run: position-major, the run is min(n_rois // 2, 300) consecutive rows.  Only 1031 x 16, C = 2048 (17 rows per
# slab, run of 300) has slabs that are dead throughout (the all-dead row pair's `continue` of the partial kernel); at
# 37 x 16, C = 512 the run is 18 rows of a 32-row slab.  The same holds for the masked position-major cases above:
# n_rois = 37 kills no slab, 1500 x 16 does (64 or 16 rows per slab, run of 300).
@pytest.mark.parametrize("kind", ["none", "random", "dead_run"])
@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("n_rois,per,C", [(37, 16, 512), (1031, 16, 2048)])
def test_joins_staged(P, n_rois, per, C, dual, with_dres, kind):
    case = "join %dx%d C=%d %s dres=%d mask=%s" % (n_rois, per, C, "dual" if dual else "identity", with_dres, kind)
    _join(P, case, n_rois * per, n_rois, C, dual, with_dres, kind)


@pytest.mark.parametrize("dual", [False, True])
def test_join_at_the_trunk_shape_class(P, dual):
    """unmasked rows of a 2 x 35 x 51 map, C = 256 (RS = 4, M no multiple of the slab)"""
    _join(P, "join trunk 2x35x51 C=256 %s" % ("dual" if dual else "identity"), 2 * 35 * 51, 1, 256, dual, not dual,
          "none", seed=28, nhw=(2, 35, 51))
