"""The f64 reference and bounds of tests/headconv_reference.py, established without a GPU.

* The reference (f64 conv2d on explicitly padded NCHW views, gradients by autograd) equals an explicit six-loop NumPy
  convolution and its adjoints on the case "one".
* The counts it takes from all-ones operands are those of the geometries: 100 of the 144 (position, tap) pairs of a
  4x4 output are valid (taps.hip's own figure), and (6, 5, 2) pads 0 before and 1 after along h.
* The clean model of the class-packed algorithm (model_conv: f32 on the CPU) stays inside every bound on every case.
* Each seeded defect misses a bound by a factor of at least 10, on "sharp" in every geometry where it can matter and
  on "flight" at 7x7.  The factor is a condition on the defects, not a tolerance on the kernels.
* Swapping `before` and `after` of the padding can matter only on (6, 5, 2): on the two symmetric geometries the
  swapped model's outputs are the clean model's bit for bit.  That is why the third geometry is there.
"""
import numpy as np
import pytest
import torch

import headconv_reference as R

LOG = {}
DEFECT_PAIRS = [("sharp", g) for g in R.CASES["sharp"][0]] + [("flight", (7, 7, 2))]


@pytest.fixture(scope="module", autouse=True)
def log():
    yield
    for k in sorted(LOG):
        print("headconv-worst %s %.4g" % (k, LOG[k]))


def test_case_table_and_inputs():
    assert R.PAIRS == [("sharp", (7, 7, 2)), ("sharp", (4, 4, 1)), ("sharp", (6, 5, 2)), ("one", (7, 7, 2)),
                       ("flight", (7, 7, 2)), ("flight", (4, 4, 1)), ("onerow", (4, 4, 1)), ("wide", (4, 4, 1))]
    dims = {name: v[1:] for name, v in R.CASES.items()}
    assert dims == dict(sharp=(37, 8, 12), one=(1, 8, 12), flight=(70, 128, 64), onerow=(5, 40, 8), wide=(3, 1028, 4))
    for name, geom in R.PAIRS:
        c = R.make_case(name, geom)
        zeros = float((c["x"] == 0).float().mean())
        assert 0.4 < zeros < 0.6 and bool((c["W"] < 0).any()) and bool((c["dy"] < 0).any()) and bool((c["b"] != 0).all())
        assert float(c["x"].min()) >= 0.0


def test_padding_rule_and_counts():
    assert R.same_pad(7, 2) == (4, 1, 1) and R.same_pad(4, 1) == (4, 1, 1) and R.same_pad(5, 2) == (3, 1, 1)
    assert R.same_pad(6, 2) == (3, 0, 1)                                   # the asymmetric axis
    assert R.same_pad(7, 2, 1) == (4, 0, 0)                                # the 1x1 at stride 2 reads rows 0, 2, 4, 6
    for geom, units, n_cls in (((4, 4, 1), 100, 9), ((7, 7, 2), 100, 9), ((6, 5, 2), 56, 6)):
        cnt = R.counts(*geom)
        pl = R.Classes(*geom)
        assert int(cnt["ntaps"].sum()) == units == int(cnt["pairs"].sum()) == int(cnt["npos"].sum())
        assert len(pl.classes) == n_cls and sorted(pl.slots) == [(y, x) for y in range(pl.oh) for x in range(pl.ow)]
        assert sum(len(t) * len(p) for t, p in pl.classes) == units
        for t in range(9):                      # the model's classes and the reference's counts agree, tap by tap
            assert int(cnt["ncls"][t]) == sum(1 for taps, _ in pl.classes if t in taps)
            assert int(cnt["npos"][t]) == sum(len(p) for taps, p in pl.classes if t in taps)
    cnt = R.counts(6, 5, 2)
    assert cnt["ntaps"].tolist() == [[6, 9, 6], [6, 9, 6], [4, 6, 4]]      # the padded row is the last one
    assert float(R.counts(4, 4, 1)["pairs"].min()) == 4 and float(R.counts(4, 4, 1)["pairs"].max()) == 9
    one = R.counts(7, 7, 2, 1)
    assert one["ntaps"].tolist() == [[1.0] * 4] * 4 and int(one["pairs"].sum()) == 16
    assert [int(v) for v in one["pairs"][0]] == [1, 0, 1, 0, 1, 0, 1] and not bool(one["pairs"][1].any())


def test_reference_equals_six_explicit_loops():
    c = R.make_case("one", (7, 7, 2))
    ref = R.case_reference("one", (7, 7, 2))
    h, w, s, C, co, oh, ow = (c[k] for k in ("h", "w", "s", "C", "co", "oh", "ow"))
    x, W, b, dy = (c[k].double().numpy() for k in ("x", "W", "b", "dy"))
    W = W.reshape(co, 3, 3, C)
    pt, pleft = 1, 1                                                        # 7 -> 4 at stride 2: total 2, 1 before
    y = np.zeros((1, oh, ow, co))
    dx, dW = np.zeros_like(x), np.zeros_like(W)
    for o in range(co):
        for oy in range(oh):
            for ox in range(ow):
                acc = b[o]
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = oy * s + ky - pt, ox * s + kx - pleft
                        if not (0 <= iy < h and 0 <= ix < w):
                            continue
                        for ch in range(C):
                            acc += x[0, iy, ix, ch] * W[o, ky, kx, ch]
                            dx[0, iy, ix, ch] += dy[0, oy, ox, o] * W[o, ky, kx, ch]
                            dW[o, ky, kx, ch] += dy[0, oy, ox, o] * x[0, iy, ix, ch]
                y[0, oy, ox, o] = acc
    for name, want in (("y", y), ("dx", dx), ("dW", dW.reshape(co, -1)), ("db", dy.sum((0, 1, 2)))):
        err = np.abs(ref[name].numpy() - want)
        assert (err <= 1e-13 * np.maximum(ref["m_" + name].numpy(), 1e-30)).all(), (name, float(err.max()))
    # the magnitudes are the sums of the terms' magnitudes
    assert abs(float(ref["m_db"][0]) - float(np.abs(dy[..., 0]).sum())) <= 1e-12


@pytest.mark.parametrize("pair", R.PAIRS, ids=R.pair_id)
@pytest.mark.parametrize("bias", [True, False])
def test_clean_model_inside_every_bound(pair, bias):
    c = R.make_case(*pair)
    ref = R.case_reference(pair[0], pair[1], bias)
    R.check_ratios("cpu-model %s bias=%d" % (R.pair_id(pair), bias), R.ratios(ref, R.model_conv(c, (), bias)), LOG)


def _defect_ratios(pair, defect):
    c = R.make_case(*pair)
    return R.ratios(R.case_reference(*pair), R.model_conv(c, (defect,)))


@pytest.mark.parametrize("pair", DEFECT_PAIRS, ids=R.pair_id)
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defect_misses_a_bound_tenfold(pair, defect):
    c = R.make_case(*pair)
    if defect == "swap_pad" and pair[1] in R.SYMMETRIC:
        clean, swapped = R.model_conv(c), R.model_conv(c, (defect,))
        for k in clean:                          # invisible where before = after: the reason for (6, 5, 2)
            assert torch.equal(clean[k], swapped[k]), (pair, k)
        return
    r = _defect_ratios(pair, defect)
    print("headconv-defect %s on %s: %s" % (defect, R.pair_id(pair), {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) >= 10.0, "%s goes unnoticed on %s: %s" % (defect, R.pair_id(pair), r)


def test_every_defect_is_seen_where_it_can_matter():
    assert ("sharp", (6, 5, 2)) in DEFECT_PAIRS and (6, 5, 2) not in R.SYMMETRIC
    assert set(R.DEFECTS) == {"drop_tap", "swap_kykx", "swap_slabs", "scatter_skip", "swap_pad", "w_kwkh"}


def test_one_dropped_tap_is_thousands_of_times_the_bound_on_sharp():
    """K <= 72: the outputs that the dropped tap reaches are far outside, each on its own"""
    for geom in R.CASES["sharp"][0]:
        r = _defect_ratios(("sharp", geom), "drop_tap")
        assert r["y"] >= 1e3 and r["dx"] >= 1e3 and r["dW"] >= 1e2, (geom, r)
