"""wssdl_decode_detections, host side: the NumPy statement of its arithmetic (tests/decode_reference.py) against an
f64 evaluation and a hand-computed row, the guard on the cases' exp arguments that makes the device test's bit
equality derivable, and the export's argument checks (every call returns before a launch).  No kernel runs here."""
import ctypes

import numpy as np
import pytest

import decode_reference as D

OK, INVALID = 0, 1


@pytest.fixture(scope="module")
def L():
    from wssdl_bus_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("name", list(D.BUILDERS))
def test_every_exp_argument_is_safe(name):
    """no exp(d) of any case lies within 4 f64 ulps of an f32 rounding boundary (a case that fails is reseeded)"""
    c = D.case(name)
    args = D.exp_arguments(c)
    assert args.size == 2 * c["K"] * int(D.live_rows(c["rois"], c["n_images"])[0].sum()) and args.size > 0
    assert np.abs(args).max() <= 4.0
    assert bool(D.exp_is_safe(args).all())


def test_exp_guard_rejects_a_boundary():
    """the guard is not vacuous: exp(0) = 1 is an f32 value (half an f32 ulp from the nearest midpoint: safe); the
    midpoint between 1 and 1 + 2^-23 and the f64 values up to 4 ulps on either side of it are rejected, the next ones
    accepted"""
    assert bool(D.exp_is_safe(np.float32(0.0)))
    mid = 1.0 + 2.0 ** -24
    ulp = float(np.spacing(mid))
    for k in range(-6, 7):
        assert bool(D.exp_value_is_safe(mid + k * ulp)) == (abs(k) > 4), k


def test_cases_cover_what_they_claim():
    c = D.case("mixed")
    live, img = D.live_rows(c["rois"], c["n_images"])
    assert c["rois"].shape[0] == 143 and c["K"] == 3 and c["n_images"] == 3
    assert [int((live & (img == i)).sum()) for i in range(3)] == [0, 1, 130]
    assert int((c["rois"][:, 0] == -1).sum()) >= 3 and int((c["rois"][:, 0] == 3).sum()) >= 3
    assert not live[0] and not live[-1]
    for bounds in (c["bounds"], None):
        raw = D.statement(c["rois"], c["deltas"], c["im_info"], 3, np.full((3, 2), 1e9, np.float32) if bounds is not None else None)
        got = D.statement(c["rois"], c["deltas"], c["im_info"], 3, bounds)
        lim = D.clip_bounds(c["im_info"], 3, bounds)[img]
        b = got.reshape(-1, 3, 4)[live]
        # clipped on all four sides, and not everything is clipped
        assert (b[:, :, 0] == 0).any() and (b[:, :, 1] == 0).any()
        assert (b[:, :, 2] == lim[live][:, None, 0]).any() and (b[:, :, 3] == lim[live][:, None, 1]).any()
        assert ((b[:, :, 0] > 0) & (b[:, :, 2] < lim[live][:, None, 0])).any()
        assert bool((got[~live] == 0).all()) and raw.shape == got.shape
    assert (c["rois"][live][:, 1:3] < 0).any()
    assert D.case("one_row")["rois"].shape == (1, 5) and D.case("one_row")["K"] == 2
    assert D.case("wide")["rois"].shape == (70, 5) and D.case("wide")["K"] == 21
    # the scores of test_gpu_val_detect's second test: no two equal scores above the threshold within an image
    s = c["scores"][live & (img == 2)][:, 1:].ravel()
    s = s[s > 0.05]
    assert s.size > 100 and np.unique(s).size == s.size


@pytest.mark.parametrize("name,given", D.RUNS)
def test_statement_within_the_counted_bound_of_f64(name, given):
    c = D.case(name)
    bounds = c["bounds"] if given else None
    got = D.statement(c["rois"], c["deltas"], c["im_info"], c["n_images"], bounds)
    want, bound = D.evaluate_f64(c["rois"], c["deltas"], c["im_info"], c["n_images"], bounds)
    assert got.dtype == np.float32 and got.shape == want.shape == c["deltas"].shape
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("decode-statement %s bounds=%s worst error / bound %.3f, largest bound %.3g" % (name, given, worst, bound.max()))
    assert bool((err <= bound).all())
    assert 0.0 < worst                                    # f32 and f64 do differ: the comparison is not of a thing with itself


def test_hand_computed_row():
    """scale 0.5, RoI (10, 20, 49, 59) -> b = (20, 40, 98, 118), w = h = 79, centre (59.5, 79.5); every value below
    is exact in f32, exp(0) = 1.
      class 0, d = (0.25, -0.5, 0, 0): pcx = 19.75 + 59.5 = 79.25, pcy = -39.5 + 79.5 = 40, pw = ph = 79
               -> (39.75, 0.5, 118.75, 79.5), clipped to (100, 70): (39.75, 0.5, 100, 70)
      class 1, d = (-1, 0, 0, 0):      pcx = -79 + 59.5 = -19.5, pcy = 79.5
               -> (-59, 40, 20, 119) -> (0, 40, 20, 70)"""
    rois = np.array([[0, 10, 20, 49, 59], [1, 10, 20, 49, 59], [-1, 10, 20, 49, 59]], np.float32)
    deltas = np.array([[0.25, -0.5, 0, 0, -1, 0, 0, 0]] * 3, np.float32)
    info = np.array([[100, 100, 0.5, 1]], np.float32)
    got = D.statement(rois, deltas, info, 1, np.array([[100, 70]], np.float32))
    assert got[0].tolist() == [39.75, 0.5, 100.0, 70.0, 0.0, 40.0, 20.0, 70.0]
    assert got[1].tolist() == [0.0] * 8 and got[2].tolist() == [0.0] * 8          # index N and -1: dead rows
    # without bounds: 100 / 0.5 - 1 = 199 on both axes, nothing clipped above
    got = D.statement(rois[:1], deltas[:1], info, 1)
    assert got[0].tolist() == [39.75, 0.5, 118.75, 79.5, 0.0, 40.0, 20.0, 119.0]
    want, bound = D.evaluate_f64(rois[:1], deltas[:1], info, 1)
    assert want[0].tolist() == got[0].tolist() and bool((bound > 0).all())


def test_export_is_declared_and_checks_its_arguments(L):
    """Every call here returns before a launch: the pointers are only compared with NULL and tested for alignment."""
    from wssdl_bus_amd import _lib
    assert "wssdl_decode_detections" in _lib.SYMBOLS
    f = L.wssdl_decode_detections
    x = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4100)

    def call(rois=x, deltas=x, R=10, K=3, info=x, stride=4, n=2, bounds=x, boxes=x):
        return f(rois, deltas, R, K, info, stride, n, bounds, boxes, None)
    assert call(R=-1) == INVALID
    assert call(K=1) == INVALID and call(K=0) == INVALID and call(K=66) == INVALID
    assert call(n=0) == INVALID and call(n=-3) == INVALID
    assert call(stride=2) == INVALID and call(stride=0) == INVALID
    assert call(rois=None) == INVALID and call(deltas=None) == INVALID
    assert call(info=None) == INVALID and call(boxes=None) == INVALID
    assert call(deltas=odd) == INVALID and call(boxes=odd) == INVALID
    # R == 0: a valid no-op, whatever the pointers; the other checks still hold
    assert call(R=0) == OK and call(R=0, rois=None, deltas=None, info=None, bounds=None, boxes=None) == OK
    assert call(R=0, K=1) == INVALID and call(R=0, n=0) == INVALID and call(R=0, stride=2) == INVALID
    assert L.wssdl_last_error() == b""
