"""The f64 references and bounds of tests/rowbn_reference.py, established without a GPU.

* The references agree with torch.nn.functional.batch_norm plus autograd in float64 (1e-12 of each output's largest
  magnitude), unmasked and -- the masked layers being defined as the compacted blob's -- on the live rows of both
  mask layouts.
* The clean kernel model (model_forward / model_backward / model_apply / model_join_*: the kernels' sums, roundings
  and fmas restated in torch) stays inside every bound: the layer at every [M, C] of the table and at every mask
  kind, split and layout with C = 256 and C = 2048; the entry gradient at 37 x 49 rows (C = 256, 1024) and 301 x 49
  (C = 256); the joins, staged as on the GPU, in every form at 37 x 16, C = 512, at the trunk's 2 x 35 x 51 rows and
  at 1031 x 16, C = 2048.  REDUCED: 16400 x 1024 and 33000 x 2048 (plain), 1500 x 16 at C = 2048 (masked) and
  1031 x 16 at C = 2048 (joins) keep their M and their geometry (block count, rows per slab, row phases) but hold
  only the first float4 column group of the case; 301 x 49 at C = 1024 (entry) is left to the GPU.  Every other shape
  runs at full width.
* Each seeded defect breaks at least one bound, on the smallest shape that reaches its code path:
    (a) the tail row of each slab is left out of the sums            1 x 4 (the only row) and 1041 x 512 (one row)
    (b) n is taken as M instead of the live-row count                37 x 49 rows, C = 256, random mask
    (c) dead rows are included in the backward sums                  the same
    (d) a position-major mask is indexed roi-major                   the same, position-major
    (e) the second column pass reuses the first pass's scale / shift 1031 x 2048
    (f) scale is off by 64 ulp                                       7 x 256
    (g) the last non-empty block's partial is dropped when capped    16400 x 1024 (reduced as above)
"""
import pytest
import torch

import rowbn_reference as R

EPS = 1e-3
REDUCED = {(16400, 1024), (33000, 2048)}


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("layout", ["plain", "roi_major", "pos_major"])
def test_reference_equals_torch_batch_norm_in_float64(layout, relu):
    n_rois, per, C = 23, 9, 16
    M = n_rois * per
    c = R.make_case(3, M, C)
    mask = None if layout == "plain" else R.make_mask("random", n_rois, 3)
    pm = layout == "pos_major"
    f = R.forward(c["x"], c["w"], c["b"], EPS, relu, mask, per, pm)
    gate = (f["pre"] > 0) if relu else None
    bk = R.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], gate, mask, per, pm)

    live = R.row_live(mask, M, per, pm)
    rows = torch.arange(M) if live is None else live.nonzero().squeeze(1)
    xl = c["x"].double()[rows].requires_grad_(True)
    w, b = c["w"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    y = torch.nn.functional.batch_norm(xl, None, None, w, b, True, 0.0, R._eps32(EPS))
    if relu:
        y = torch.relu(y)
    y.backward(c["dy"].double()[rows])
    assert f["count"] == len(rows)
    want_y, want_dx = torch.zeros_like(f["y"]), torch.zeros_like(bk["dx"])
    want_y[rows], want_dx[rows] = y.detach(), xl.grad
    xd = xl.detach()
    for name, got, want in (("y", f["y"], want_y), ("dx", bk["dx"], want_dx), ("dweight", bk["dweight"], w.grad),
                            ("dbias", bk["dbias"], b.grad), ("mean", f["mean"], xd.mean(0)),
                            ("var", f["var"], xd.var(0, unbiased=False))):
        assert _rel(got, want) <= 1e-12, "%s %s relu=%s: %g" % (name, layout, relu, _rel(got, want))
    if live is not None:
        assert not bool(f["y"][~live].any()) and not bool(bk["dx"][~live].any())


def test_all_dead_reference():
    c = R.make_case(4, 32, 8)
    mask = torch.zeros((8,))
    f = R.forward(c["x"], c["w"], c["b"], EPS, True, mask, 4, False)
    assert f["count"] == 1.0 and not bool(f["mean"].any()) and not bool(f["var"].any()) and not bool(f["y"].any())
    bk = R.backward(c["x"], c["dy"], c["w"], f["mean"], f["rstd"], f["pre"] > 0, mask, 4, False)
    assert not bool(bk["dx"].any()) and not bool(bk["dweight"].any()) and not bool(bk["dbias"].any())


def test_entry_total_is_the_scatter_add():
    n_rois, per, C, ns = 5, 6, 8, 3
    g = torch.Generator().manual_seed(0)
    dy, dys = torch.randn((n_rois * per, C), generator=g), torch.randn((ns * n_rois, C), generator=g)
    possel = torch.tensor([-1, 2, -1, 0, 1, -1], dtype=torch.int32)
    t = R.entry_total(dy, dys, possel, n_rois)
    for roi in range(n_rois):
        for p in range(per):
            want = dy[roi * per + p].double()
            if possel[p] >= 0:
                want = want + dys[int(possel[p]) * n_rois + roi].double()
            assert torch.equal(t[roi * per + p], want)


def test_tail_rows_of_the_slab_walk():
    """_tail_rows against the loop it restates, row by row"""
    for M, C in [(1, 4), (259, 16), (7, 256), (1041, 512), (16400, 1024)]:
        L, RS, nb, rpb = R.geometry(M, C)
        want = torch.zeros((M,), dtype=torch.bool)
        seen = torch.zeros((M,), dtype=torch.int32)
        for blk in range(nb):
            r0, r1 = blk * rpb, min(blk * rpb + rpb, M)
            for lr in range(RS):
                r = r0 + lr
                while r + RS < r1:
                    seen[r] += 1
                    seen[r + RS] += 1
                    r += 2 * RS
                while r < r1:
                    seen[r] += 1
                    want[r] = True
                    r += RS
        assert bool((seen == 1).all()), (M, C)
        assert torch.equal(R._tail_rows(M, RS, rpb, "cpu"), want), (M, C)


def test_geometry_of_the_table():
    geo = {mc: R.geometry(*mc) for mc in R.TABLE}
    assert geo[(1, 4)][:3] == (1, 256, 1)
    assert geo[(259, 16)][:2] == (4, 64)
    assert geo[(7, 256)][:3] == (64, 4, 1)
    assert geo[(1041, 512)] == (128, 2, 33, 32) and (1041 - 32 * 32) % 2 == 1
    assert geo[(4099, 1024)][1:3] == (1, 257) and 4099 - 256 * geo[(4099, 1024)][3] == 3
    assert geo[(16400, 1024)] == (256, 1, 1024, 17) and (16400 - 1) // 17 < 1023
    assert geo[(33000, 2048)][2] == 1024 and 33000 * 512 > 65536 * 256


def _model_ratios(c, relu, mask=None, per=1, pm=False, geom_C=None, defects="", eps=EPS):
    """worst |error| / bound per output of the kernel model against the references, judged in stages as the GPU is"""
    m = R.model_forward(c["x"], c["w"], c["b"], eps, relu, mask, per, pm, geom_C, defects)
    r, f, by = R.forward_ratios(c["x"], c["w"], c["b"], eps, relu, m, mask, per, pm)
    bad, inside = R.gate_mismatches(m["y"], f, by)
    r["gate"] = float("inf") if bad else 0.0
    gate = (m["y"] > 0) if relu else None
    mb = R.model_backward(c["x"], c["dy"], c["w"], m, relu, mask, per, pm, geom_C, defects)
    rb, _ = R.backward_ratios(c["x"], c["dy"], c["w"], m["mean"], m["rstd"], gate, mb, mask, per, pm)
    r.update(rb)
    return r, m, inside


def _table_case(M, C, seed=11):
    if (M, C) in REDUCED:
        return R.make_case(seed, M, C, cols=4), C
    return R.make_case(seed, M, C), None


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", R.TABLE)
def test_clean_model_inside_every_bound_plain(M, C, relu):
    c, geom_C = _table_case(M, C)
    r, m, _ = _model_ratios(c, relu, geom_C=geom_C)
    ref = c["x"].double() * m["scale"].double() + m["shift"].double()
    r["apply"] = R.ratio(R.model_apply(c["x"], m["scale"], m["shift"], relu), ref.clamp_min(0.0) if relu else ref,
                         R.bound_apply(ref))
    R.check_ratios("model %dx%d relu=%d" % (M, C, relu), r)
    if M == 1:
        assert not bool(m["var"].any())                     # one row: var = 0 exactly


@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("kind", R.MASK_KINDS)
@pytest.mark.parametrize("C", [256, 2048])
@pytest.mark.parametrize("n_rois,per", R.MASK_SPLITS)
def test_clean_model_inside_every_bound_masked(n_rois, per, C, kind, pm):
    M = n_rois * per
    reduced = (n_rois, per, C) == (1500, 16, 2048)
    c = R.make_case(12, M, C, cols=4 if reduced else None)
    mask = R.make_mask(kind, n_rois, 12)
    r, m, _ = _model_ratios(c, True, mask, per, pm, geom_C=C if reduced else None)
    R.check_ratios("model %dx%d %s pm=%d" % (M, C, kind, pm), r)
    live = R.row_live(mask, M, per, pm)
    assert m["count"] == max(per * float(mask.sum()), 1.0)
    assert not bool(m["y"][~live].any())
    if kind == "all_dead":
        assert not bool(m["mean"].any()) and not bool(m["var"].any())
    if kind == "one_live" and per == 1:
        assert m["count"] == 1.0 and not bool(m["var"].any())


@pytest.mark.parametrize("kind", ["none", "random"])
@pytest.mark.parametrize("n_rois,C", [(37, 256), (37, 1024), (301, 256)])
def test_clean_model_inside_every_bound_entry(n_rois, C, kind):
    """the entry gradient: possel of the head's 7 x 7 map sampled at stride 2 (16 slots, as TapPlan.subsample_slots)"""
    per, ns = 49, 16
    possel = torch.full((per,), -1, dtype=torch.int32)
    for sl in range(ns):
        possel[(sl // 4) * 2 * 7 + (sl % 4) * 2] = (sl * 5) % ns          # some order of the slots
    assert sorted(possel[possel >= 0].tolist()) == list(range(ns))
    c = R.make_case(13, n_rois * per, C)
    dys = R.make_case(14, ns * n_rois, C)["dy"]
    mask = None if kind == "none" else R.make_mask(kind, n_rois, 13)
    m = R.model_forward(c["x"], c["w"], c["b"], EPS, True, mask, per, False)
    mb = R.model_backward(c["x"], c["dy"], c["w"], m, True, mask, per, False, entry=(dys, possel, n_rois))
    r = R.entry_ratios(c["x"], c["dy"], dys, possel, n_rois, c["w"], m["mean"], m["rstd"], m["y"] > 0, mb, mask)
    R.check_ratios("model entry %dx49 C=%d mask=%s" % (n_rois, C, kind), r)
    plain = R.model_backward(c["x"], c["dy"], c["w"], m, True, mask, per, False)
    assert not torch.equal(plain["dx"], mb["dx"])          # the shortcut's part reached the gradient


def _model_join(case, M, n_rois, C, dual, with_dres, kind, cols=None, seed=15):
    """the join models judged in the GPU test's stages"""
    geom_C = C if cols is not None else None
    c3, co, cn = (R.make_case(seed + k, M, C, cols=cols) for k in range(3))
    x3, other = c3["x"], co["x"]
    bn3, bnn = (c3["w"], c3["b"], EPS), (cn["w"], cn["b"], EPS)
    bns = (co["w"], co["b"], 1e-5) if dual else None
    mask = None if kind == "none" else R.make_mask(kind, n_rois, n_rois)
    out, y, m3, ms, mn = R.model_join_forward(x3, bn3, other, bns, bnn, mask, geom_C)
    r, fn, byn = R.join_forward_ratios(x3, bn3, other, bns, bnn, mask, out, y, m3, ms, mn)
    bad, _ = R.gate_mismatches(y, fn, byn)
    r["gate"] = float("inf") if bad else 0.0
    dres = cn["dres"] if with_dres else None
    xs, ws = (other, co["w"]) if dual else (None, None)
    g, bn, b3, bs = R.model_join_backward(out, cn["dy"], dres, x3, xs, cn["w"], mn, c3["w"], m3, ws, ms, mask, geom_C)
    pair = lambda b: None if b is None else (b["dweight"], b["dbias"])
    r.update(R.join_backward_ratios(out, cn["dy"], dres, x3, xs, cn["w"], mn, c3["w"], m3, ws, ms, y > 0, mask, g,
                                    b3["dx"], None if bs is None else bs["dx"], pair(bn), pair(b3), pair(bs)))
    R.check_ratios(case, r)
    if mask is not None:
        live = R.row_live(mask, M, M // n_rois, True)
        assert torch.equal(out[~live], torch.zeros_like(out[~live]) if dual else other[~live]), case
        assert torch.equal(g[~live], dres[~live] if with_dres else torch.zeros_like(g[~live])), case


@pytest.mark.parametrize("kind", ["none", "random", "dead_run"])
@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("dual", [False, True])
def test_clean_model_inside_every_bound_joins(dual, with_dres, kind):
    _model_join("model join 37x16 C=512 dual=%d dres=%d mask=%s" % (dual, with_dres, kind), 37 * 16, 37, 512, dual,
                with_dres, kind)


@pytest.mark.parametrize("dual", [False, True])
def test_clean_model_inside_every_bound_joins_other_shapes(dual):
    _model_join("model join trunk 2x35x51 C=256 dual=%d" % dual, 2 * 35 * 51, 1, 256, dual, not dual, "none", seed=18)
    _model_join("model join 1031x16 C=2048 (one column group) dual=%d" % dual, 1031 * 16, 1031, 2048, dual, True,
                "dead_run", cols=4)


def _masked(pm):
    n_rois, per = 37, 49
    return R.make_case(12, n_rois * per, 256), dict(mask=R.make_mask("random", n_rois, 12), per=per, pm=pm)


DEFECTS = [
    ("a", (1, 4), {}), ("a", (1041, 512), {}),
    ("b", None, dict(pm=False)), ("c", None, dict(pm=False)), ("d", None, dict(pm=True)),
    ("e", (1031, 2048), {}), ("f", (7, 256), {}), ("g", (16400, 1024), {}),
]


@pytest.mark.parametrize("defect,shape,kw", DEFECTS, ids=["%s-%s" % (d, "masked" if s is None else "%dx%d" % s)
                                                          for d, s, _ in DEFECTS])
def test_seeded_defect_breaks_a_bound(defect, shape, kw):
    if shape is None:
        c, kw = _masked(kw["pm"])
        geom_C = None
    else:
        c, geom_C = _table_case(*shape)
    clean, _, _ = _model_ratios(c, True, geom_C=geom_C, **kw)
    assert max(clean.values()) <= 1.0, clean
    bad, _, _ = _model_ratios(c, True, geom_C=geom_C, defects=defect, **kw)
    broken = {k: v for k, v in bad.items() if v > 1.0}
    print("defect (%s) breaks %s" % (defect, ", ".join("%s %.3g" % kv for kv in sorted(broken.items()))))
    assert broken, "defect (%s) stays inside every bound: %r" % (defect, bad)


def test_running_formula():
    """running() against the statement written out step by step for one column"""
    rm, rv = R.running(torch.tensor([0.25]), torch.tensor([1.5]), torch.tensor([2.0]), torch.tensor([3.0]), 4.0, 0.01)
    mom = float(torch.tensor(0.01, dtype=torch.float32).double())
    assert float(rm) == float(torch.tensor(0.25 + mom * (2.0 - 0.25)).float())
    assert float(rv) == float(torch.tensor(1.5 + mom * (3.0 * (4.0 / 3.0) - 1.5), dtype=torch.float64).float())
    _, rv1 = R.running(torch.tensor([0.25]), torch.tensor([1.5]), torch.tensor([2.0]), torch.tensor([0.0]), 1.0, 1.0)
    assert float(rv1) == 0.0                                # n = 1: the unbias factor is clamped to 1
