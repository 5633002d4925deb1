"""Shared by test_eval_cpu.py and test_gpu_eval.py: the cases of tests/golden/eval_detections.npz (the reference's
voc_eval_bus on them, make_golden_eval.py) and the criteria both paths are held to."""
import numpy as np

from conftest import load_golden

K = 3
_cache = {}


def golden():
    if "g" not in _cache:
        g = load_golden("eval_detections")
        _cache["g"] = {k: g[k] for k in g.files}
    return _cache["g"]


def case(name):
    """(flat detections (boxes, scores, image, class), gt (boxes, classes, difficult, offsets), thresholds)"""
    g = golden()
    d = g[name + "_dets"]
    dets = (np.ascontiguousarray(d[:, :4]), np.ascontiguousarray(d[:, 4]), g[name + "_image"], g[name + "_class"])
    gt = (g[name + "_gt_boxes"].astype(np.float64), g[name + "_gt_class"], g[name + "_gt_difficult"], g[name + "_gt_offsets"])
    return dets, gt, g["thresholds"]


def to_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def segment(r, name, c):
    o = to_np(r["class_offsets"])
    return to_np(r[name])[o[c - 1]:o[c]]


def check_thresholded(r, name, gt, base):
    """ni, nok, num_all_fps for all 21 thresholds; arr_ok and num_fp_per_img at thresholds[base]"""
    g = golden()
    off, gc = gt[3], gt[1]
    gimg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    for c in (1, 2):
        p = "%s_c%d_" % (name, c)
        assert int(r["ni"][c - 1]) == int(g[p + "ni"])
        assert np.array_equal(r["nok"][c - 1], g[p + "nok"])
        assert np.array_equal(r["num_all_fps"][c - 1], g[p + "num_all_fps"])
        assert np.array_equal(r["num_fp_per_img"][c - 1], g[p + "num_fp_per_img"][base])
        has = np.zeros(len(off) - 1, bool)
        has[gimg[gc == c]] = True
        want = g[p + "arr_ok"][base]                     # the reference's: entry k = k-th image with a box of the class
        assert np.array_equal(r["arr_ok"][c - 1][has], want[:has.sum()] != 0) and not want[has.sum():].any()
        assert not r["arr_ok"][c - 1][~has].any()


def check_small(r, gt, base):
    """Every value of the reference on `small`: integers, rec, prec and the 11-point AP bit-equal; the area AP within
    1e-12 absolute (a sum of at most D + 1 products, each <= 1: D * eps ~ 3e-13 at D = 2560, less here)."""
    g = golden()
    check_thresholded(r, "small", gt, base)
    for c in (1, 2):
        p = "small_c%d_" % c
        assert np.array_equal(segment(r, "rec", c), g[p + "rec"])
        assert np.array_equal(segment(r, "prec", c), g[p + "prec"])
        assert float(r["ap07"][c - 1]) == float(g[p + "ap07"])
        assert abs(float(r["ap_area"][c - 1]) - float(g[p + "ap_area"])) <= 1e-12
        tp, fp = segment(r, "tp", c), segment(r, "fp", c)
        assert np.array_equal(tp / float(r["npos"][c - 1]), g[p + "rec"]) and len(tp) == len(fp)


def check_runs(r, gt, base):
    """What the reference gives on `runs` whatever the order among equal scores"""
    g = golden()
    check_thresholded(r, "runs", gt, base)
    for c in (1, 2):
        p = "runs_c%d_" % c
        assert int(r["npos"][c - 1]) == int(g[p + "npos"])
        assert [int(segment(r, "tp", c)[-1]), int(segment(r, "fp", c)[-1])] == list(g[p + "tp_fp_total"])


def check_same(a, b, area_tol=1e-12):
    """two results of this package (device / host path, or two layouts): everything bit-equal but the area AP, whose
    summation order is free"""
    for k in ("class_offsets", "npos", "ni", "nok", "num_all_fps", "arr_ok", "num_fp_per_img", "order", "tp", "fp", "rec", "prec", "ap07"):
        assert np.array_equal(to_np(a[k]), to_np(b[k]), equal_nan=k in ("rec", "prec", "ap07")), k
    assert np.allclose(a["ap_area"], b["ap_area"], rtol=0, atol=area_tol, equal_nan=True)
