"""Detection evaluation without a GPU: the module's host path against the reference's voc_eval_bus
(tests/golden/eval_detections.npz), voc_ap, evaluate_detections' assembly of what bus.py:_do_python_eval reports,
the host-side entry points of the C ABI, and the fixture generator."""
import os
import sys

import numpy as np
import pytest
import torch

from eval_cases import K, case, check_runs, check_same, check_small, golden, segment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from wssdl_bus_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def base_first(thresholds, base=10):
    """the thresholds with thresholds[base] in front: arr_ok and num_fp_per_img are those of the first
    (np.arange(1.0, -0.01, -0.05)[10] is 0.49999999999999956, not the 0.5 of the reference's CorLoc call; no
    3-decimal score lies between the two)"""
    return [thresholds[base]] + list(thresholds)


def drop_first(r):
    r = dict(r)
    r["nok"], r["num_all_fps"] = r["nok"][:, 1:], r["num_all_fps"][:, 1:]
    return r


def test_host_path_matches_reference_on_small():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case("small")
    r = eval_detections(dets, gt, K, score_thresh=base_first(thr))
    assert np.array_equal(r["nok"][:, 0], r["nok"][:, 11])
    check_small(drop_first(r), gt, 10)


def test_host_path_matches_reference_on_runs():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case("runs")
    r = eval_detections(dets, gt, K, score_thresh=base_first(thr))
    check_runs(drop_first(r), gt, 10)
    for c in (1, 2):                                     # ties keep their input order
        o = segment(r, "order", c)
        q = np.rint(dets[1][o].astype(np.float64) * 1000.0)
        assert np.all((q[:-1] > q[1:]) | ((q[:-1] == q[1:]) & (o[:-1] < o[1:])))


def test_host_path_layouts_agree():
    from wssdl_bus_amd.datasets import eval_detections, flatten_batched
    dets, gt, thr = case("small")
    n_images, P = len(gt[3]) - 1, 8
    b = np.zeros((n_images, K - 1, P, 5), np.float32)
    n = np.zeros((n_images, K - 1), np.int32)
    for k in range(len(dets[1])):
        i, j = dets[2][k], dets[3][k] - 1
        b[i, j, n[i, j], :4], b[i, j, n[i, j], 4] = dets[0][k], dets[1][k]
        n[i, j] += 1
    r = eval_detections((b, n), gt, K, score_thresh=base_first(thr))
    check_small(drop_first(r), gt, 10)
    flat = flatten_batched(b, n)
    rf = eval_detections(flat[:4], gt, K, score_thresh=base_first(thr))
    rf["order"] = np.where(rf["order"] >= 0, flat[4][rf["order"]], -1)
    for k in ("order", "tp", "fp", "rec", "prec"):       # the batched layout reports slots: live ones first, as here
        r[k] = r[k][:len(rf[k])]
    check_same(r, rf)


def test_voc_ap_matches_reference():
    from wssdl_bus_amd.datasets import voc_ap
    g = golden()
    for c in (1, 2):
        p = "small_c%d_" % c
        assert voc_ap(g[p + "rec"], g[p + "prec"], True) == float(g[p + "ap07"])
        assert abs(voc_ap(g[p + "rec"], g[p + "prec"]) - float(g[p + "ap_area"])) <= 1e-12
    assert voc_ap(np.array([0.5, 1.0]), np.array([1.0, 1.0]), True) == sum([1.0 / 11.] * 11)
    assert voc_ap(np.array([0.5, 1.0]), np.array([1.0, 0.5])) == 0.75


def test_evaluate_detections_assembles_like_bus_py():
    from wssdl_bus_amd.datasets import evaluate_detections
    dets, gt, thr = case("small")
    g = golden()
    n_images = len(gt[3]) - 1
    all_boxes = [[[] for _ in range(n_images)] for _ in range(K)]
    for j in (1, 2):
        for i in range(n_images):
            m = (dets[2] == i) & (dets[3] == j)
            if m.any():
                all_boxes[j][i] = np.concatenate((dets[0][m], dets[1][m][:, None]), 1)
    gt_roidb = [dict(boxes=gt[0][gt[3][i]:gt[3][i + 1]].astype(np.int64), gt_classes=gt[1][gt[3][i]:gt[3][i + 1]],
                     difficult=gt[2][gt[3][i]:gt[3][i + 1]]) for i in range(n_images)]
    r = evaluate_detections(all_boxes, gt_roidb, ("__background__", "benign", "malignant"))
    ni = [float(g["small_c%d_ni" % c]) for c in (1, 2)]
    nok = [g["small_c%d_nok" % c].astype(np.float64) for c in (1, 2)]
    fps = [g["small_c%d_num_all_fps" % c].astype(np.float64) for c in (1, 2)]
    assert r["aps"] == [float(g["small_c1_ap07"]), float(g["small_c2_ap07"])]
    assert r["mean_ap"] == np.mean(r["aps"])
    assert r["corloc_list"] == [nok[0][10] / ni[0], nok[1][10] / ni[1], (nok[0][10] + nok[1][10]) / (ni[0] + ni[1])]
    pts = [[(fps[c][t] / ni[c], nok[c][t] / ni[c]) for t in range(21)] for c in range(2)]
    assert r["froc_curve_pts"][1] == pts[0] and r["froc_curve_pts"][2] == pts[1]
    assert r["froc_curve_pts"][0] == [((pts[0][t][0] + pts[1][t][0]) / 2, (pts[0][t][1] + pts[1][t][1]) / 2) for t in range(21)]
    assert np.array_equal(r["all_arr_ok"], np.concatenate((g["small_c1_arr_ok"][10], g["small_c2_arr_ok"][10])))
    assert np.array_equal(r["num_fp_per_img"], g["small_c1_num_fp_per_img"][10] + g["small_c2_num_fp_per_img"][10])


def test_class_without_boxes_reports_nan_corloc():
    from wssdl_bus_amd.datasets import evaluate_detections
    all_boxes = [[[]], [np.array([[0, 0, 10, 10, 0.9]], np.float32)], [[]]]
    r = evaluate_detections(all_boxes, [dict(boxes=np.array([[1, 1, 11, 11]]), gt_classes=[1], difficult=[0])], ("bg", "a", "b"))
    assert r["corloc_list"][0] == 1.0 and np.isnan(r["corloc_list"][1]) and r["corloc_list"][2] == 1.0
    assert r["aps"][0] == sum([1.0 / 11.] * 11) and r["aps"][1] == -1.0   # (eleven times 1 / 11. in f64, as the reference adds)


def test_accumulator_on_host_tensors():
    from wssdl_bus_amd.datasets import DetectionAccumulator, eval_detections
    dets, gt, thr = case("small")
    n_images, P = len(gt[3]) - 1, 8
    b = np.zeros((n_images, K - 1, P, 5), np.float32)
    n = np.zeros((n_images, K - 1), np.int32)
    for k in range(len(dets[1])):
        i, j = dets[2][k], dets[3][k] - 1
        b[i, j, n[i, j], :4], b[i, j, n[i, j], 4] = dets[0][k], dets[1][k]
        n[i, j] += 1
    acc = DetectionAccumulator(K)
    for first in (8, 0, 4):                              # batches in any order
        acc.add(torch.from_numpy(b[first:first + 4]), torch.from_numpy(n[first:first + 4]), first)
    check_same(acc.evaluate(gt, score_thresh=list(thr)), eval_detections((b, n), gt, K, score_thresh=list(thr)))


def test_workspace_query_is_pure_host(lib):
    n = lib.wssdl_eval_detections_workspace_bytes(300000 * 2, 3000, 1000, 3)
    assert n >= 2 * 600000 * 8 + 600000 * (8 + 4 + 12)
    assert lib.wssdl_eval_detections_workspace_bytes(0, 0, 0, 2) > 0
    assert lib.wssdl_eval_detections_workspace_bytes(-1, 0, 0, 2) == 0
    assert lib.wssdl_eval_detections_workspace_bytes(10, 0, 0, 1) == 0


def test_invalid_arguments_return_status_not_crash(lib):
    from wssdl_bus_amd import _lib

    def call(flags=1, D=0, N=0, P=0, G=0, n_images=0, K=3, T=1, base=0, ws=1 << 20, bufs=True):
        p = _lib.ctypes.c_void_p(4096) if bufs else None     # never dereferenced: every case below is rejected on the host
        return lib.wssdl_eval_detections(flags, p, p, p, p, D, p, p, N, P, 0, p, p, p, p, G, n_images, K, 0.5, p, T, base,
                                         p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, None)
    E = _lib.ERR_INVALID_ARGUMENT
    assert call(D=-1) == E and call(G=-1) == E and call(n_images=-1) == E
    assert call(T=0) == E and call(K=1) == E and call(K=66) == E
    assert call(base=1) == E and call(base=-1) == E
    assert call(flags=2, N=-1) == E and call(flags=2, N=1, P=-1) == E
    assert call(flags=4) == E
    assert call(D=(1 << 24) + 1) == E
    assert call(D=4096, ws=1024) == E                    # a too-small workspace
    assert call(bufs=False) == E                         # missing pointers


@pytest.mark.skipif(not os.path.exists("/root/reference"), reason="the reference is only in the build container")
def test_generator_reproduces_the_committed_fixture():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_golden_eval
    finally:
        sys.path.pop(0)
    fresh, stored = make_golden_eval.generate(), golden()
    assert sorted(fresh) == sorted(stored)
    for k in stored:
        a, b = np.asarray(fresh[k]), stored[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
