"""wssdl_eval_detections on the GPU: against the reference's voc_eval_bus (tests/golden/eval_detections.npz) and,
where the reference's order among equal scores is an accident, against the module's host path under the stated tie
rule (input order)."""
import numpy as np
import pytest
import torch

from eval_cases import K, case, check_runs, check_same, check_small, to_np

pytestmark = pytest.mark.gpu


def dev(dets):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in dets)


def with_base(thr, base=10):
    return [thr[base]] + list(thr)


def drop_first(r):
    r = dict(r)
    r["nok"], r["num_all_fps"] = r["nok"][:, 1:], r["num_all_fps"][:, 1:]
    return r


def batched_of(dets, n_images, P):
    b = np.zeros((n_images, K - 1, P, 5), np.float32)
    n = np.zeros((n_images, K - 1), np.int32)
    slot = np.zeros(len(dets[1]), np.int64)
    for k in range(len(dets[1])):
        i, j = dets[2][k], dets[3][k] - 1
        b[i, j, n[i, j], :4], b[i, j, n[i, j], 4] = dets[0][k], dets[1][k]
        slot[k] = (i * (K - 1) + j) * P + n[i, j]
        n[i, j] += 1
    return b, n, slot


def random_case(seed, n_images, D, n_gt, score_values=200):
    rs = np.random.RandomState(seed)
    x, y = rs.uniform(0, 300, D), rs.uniform(0, 300, D)
    boxes = np.stack((x, y, x + rs.uniform(10, 150, D), y + rs.uniform(10, 150, D)), 1).astype(np.float32)
    scores = (rs.randint(0, score_values + 1, D) / float(score_values)).astype(np.float32)
    image = np.sort(rs.randint(0, n_images, D)).astype(np.int32)
    cls = rs.randint(1, K, D).astype(np.int32)
    gx, gy = rs.randint(1, 300, n_gt), rs.randint(1, 300, n_gt)
    gb = np.stack((gx, gy, gx + rs.randint(10, 150, n_gt), gy + rs.randint(10, 150, n_gt)), 1).astype(np.float64)
    gimg = np.sort(rs.randint(0, n_images, n_gt))
    off = np.searchsorted(gimg, np.arange(n_images + 1)).astype(np.int32)
    gt = (gb, rs.randint(1, K, n_gt).astype(np.int32), (rs.rand(n_gt) < 0.2).astype(np.uint8), off)
    return (boxes, scores, image, cls), gt


def test_small_matches_reference():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case("small")
    r = eval_detections(dev(dets), gt, K, score_thresh=with_base(thr))
    assert r["rec"].is_cuda and r["order"].is_cuda
    check_small(drop_first(r), gt, 10)
    check_same(r, eval_detections(dets, gt, K, score_thresh=with_base(thr)))


def test_runs_matches_reference_and_host_path():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case("runs")
    r = eval_detections(dev(dets), gt, K, score_thresh=with_base(thr))
    check_runs(drop_first(r), gt, 10)
    check_same(r, eval_detections(dets, gt, K, score_thresh=with_base(thr)))     # the order index for index


@pytest.mark.parametrize("name,P", [("small", 8), ("runs", 64), ("runs", 70)])
def test_both_layouts_agree(name, P):
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case(name)
    b, n, slot = batched_of(dets, len(gt[3]) - 1, P)
    flat = eval_detections(dev(dets), gt, K, score_thresh=list(thr))
    bat = eval_detections((torch.from_numpy(b).cuda(), torch.from_numpy(n).cuda()), gt, K, score_thresh=list(thr))
    D = len(dets[1])
    for k in ("order", "tp", "fp", "rec", "prec"):
        tail = to_np(bat[k])[D:]
        assert np.all(tail == (-1 if k == "order" else 0))
        bat[k] = to_np(bat[k])[:D]
    flat["order"] = slot[to_np(flat["order"])]
    for k in flat:
        if k not in ("thresholds", "base_threshold", "ap"):
            assert np.array_equal(to_np(flat[k]), to_np(bat[k])), k              # the area AP too: the same sums


def test_first_image_offset():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case("small")
    b, n, _ = batched_of(dets, 12, 8)
    whole = eval_detections((torch.from_numpy(b).cuda(), torch.from_numpy(n).cuda()), gt, K, score_thresh=list(thr))
    part = eval_detections((torch.from_numpy(b[5:]).cuda(), torch.from_numpy(n[5:]).cuda(), 5), gt, K, score_thresh=list(thr))
    keep = dets[2] >= 5
    want = eval_detections(tuple(a[keep] for a in dets), gt, K, score_thresh=list(thr))
    assert np.array_equal(part["nok"], want["nok"]) and np.array_equal(part["num_all_fps"], want["num_all_fps"])
    assert np.array_equal(part["ap07"], want["ap07"]) and np.array_equal(part["num_fp_per_img"], want["num_fp_per_img"])
    assert not np.array_equal(part["num_all_fps"], whole["num_all_fps"])


@pytest.mark.parametrize("name", ["small", "runs"])
def test_without_quantisation_matches_host_path(name):
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case(name)
    r = eval_detections(dev(dets), gt, K, score_thresh=list(thr), as_result_file=False)
    check_same(r, eval_detections(dets, gt, K, score_thresh=list(thr), as_result_file=False))


def test_quantisation_flag_decides_what_is_scored():
    """box [0,0,9,9] + 1 is the ground-truth box (overlap 1), as it stands it overlaps it by 81 / 119; the score
    0.9004 is written as 0.900, below the threshold 0.9003"""
    from wssdl_bus_amd.datasets import eval_detections
    gt = (np.array([[1., 1, 10, 10]]), np.array([1], np.int32), np.array([0], np.uint8), np.array([0, 1], np.int32))
    dets = (np.array([[0, 0, 9, 9]], np.float32), np.array([0.9004], np.float32), np.array([0], np.int32), np.array([1], np.int32))
    q = eval_detections(dev(dets), gt, K, ovthresh=0.9, score_thresh=(0.9003,))
    assert to_np(q["tp"]).tolist() == [1] and q["nok"][0, 0] == 0 and q["num_all_fps"][0, 0] == 0
    r = eval_detections(dev(dets), gt, K, ovthresh=0.9, score_thresh=(0.9003,), as_result_file=False)
    assert to_np(r["tp"]).tolist() == [0] and to_np(r["fp"]).tolist() == [1] and r["num_all_fps"][0, 0] == 1
    assert r["num_fp_per_img"][0, 0] == 1 and q["num_fp_per_img"][0, 0] == 0


def test_empty_inputs_and_empty_classes():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case("small")
    none = tuple(a[:0] for a in dets)
    r = eval_detections(dev(none), gt, K, score_thresh=list(thr))                 # D == 0
    assert list(r["ap07"]) == [-1.0, -1.0] and list(r["ap_area"]) == [-1.0, -1.0] and not r["nok"].any()
    check_same(r, eval_detections(none, gt, K, score_thresh=list(thr)))
    no_gt = (gt[0][:0], gt[1][:0], gt[2][:0], np.zeros_like(gt[3]))               # G == 0
    r = eval_detections(dev(dets), no_gt, K, score_thresh=list(thr))
    assert not r["ni"].any() and not r["npos"].any() and not to_np(r["tp"]).any()
    check_same(r, eval_detections(dets, no_gt, K, score_thresh=list(thr)))
    one = tuple(a[dets[3] == 2] for a in dets)                                    # class 1 without detections
    r = eval_detections(dev(one), gt, K, score_thresh=list(thr))
    assert r["ap07"][0] == -1.0 and r["ap07"][1] >= 0 and r["ni"][0] > 0
    check_same(r, eval_detections(one, gt, K, score_thresh=list(thr)))
    r = eval_detections(dev(none), no_gt, K, score_thresh=(0.5,))                 # both
    assert list(r["ap07"]) == [-1.0, -1.0]


@pytest.mark.parametrize("n_images,D,n_gt", [(1, 9001, 7), (37, 4097, 90), (5, 2048, 0), (3, 2049, 11)])
def test_random_cases_match_host_path(n_images, D, n_gt):
    """more than one sort run and scan block, odd sizes, heavy score ties; (1, ...) = all detections in one image"""
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt = random_case(n_images * 1000 + D, n_images, D, n_gt)
    thr = np.arange(1.0, -0.01, -0.05)
    for quantise in (True, False):
        r = eval_detections(dev(dets), gt, K, score_thresh=list(thr), as_result_file=quantise)
        check_same(r, eval_detections(dets, gt, K, score_thresh=list(thr), as_result_file=quantise))


def test_ignored_detections_and_boxes():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt = random_case(5, 4, 300, 20)
    dets[2][::7] = 9                                     # an image outside the ground truth
    dets[3][::5] = 0                                     # background / unknown classes
    dets[3][3::11] = K
    gt[1][::4] = K + 2
    r = eval_detections(dev(dets), gt, K, score_thresh=(0.5, 0.1))
    check_same(r, eval_detections(dets, gt, K, score_thresh=(0.5, 0.1)))
    assert r["class_offsets"][-1] < 300


def test_two_runs_give_the_same_bits():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = case("runs")
    a = eval_detections(dev(dets), gt, K, score_thresh=list(thr))
    b = eval_detections(dev(dets), gt, K, score_thresh=list(thr))
    for k in a:
        if k not in ("thresholds", "base_threshold"):
            assert to_np(a[k]).tobytes() == to_np(b[k]).tobytes(), k


def test_accumulator_after_post_detections_matches_host_route():
    """post_detections_batched_device -> DetectionAccumulator -> one op, against the host all_boxes of the same
    batch through the module's host path"""
    from wssdl_bus_amd.datasets import DetectionAccumulator, evaluate_detections
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device, postprocess_detections_batch
    rs = np.random.RandomState(11)
    n_images, rows = 3, 60
    R = n_images * rows
    centers = rs.uniform(40, 260, (R, 2))
    size = rs.uniform(20, 120, (R, K, 2))
    boxes = np.concatenate([np.concatenate((centers - size[:, j] / 2, centers + size[:, j] / 2), 1) for j in range(K)], 1).astype(np.float32)
    e = np.exp(rs.normal(0, 2, (R, K)))
    scores = (e / e.sum(1, keepdims=True)).astype(np.float32)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(n_images), rows)
    s, b, r = (torch.from_numpy(a).cuda() for a in (scores, boxes, rois))
    gt_roidb = []
    for i in range(n_images):
        c = centers[i * rows + rs.randint(0, rows, 3)]
        gt_roidb.append(dict(boxes=np.rint(np.concatenate((c - 35, c + 35), 1)).astype(np.int64) + 1, gt_classes=np.array([1, 2, 1]),
                             difficult=np.array([0, 0, 1])))
    classes = ("__background__", "benign", "malignant")
    per_image = postprocess_detections_batch(s, b, r, n_images, K, 0.05, 20)
    all_boxes = [[[] for _ in range(n_images)] for _ in range(K)]
    for i, d in enumerate(per_image):
        for j in range(1, K):
            all_boxes[j][i] = d[j].cpu().numpy()
    assert sum(len(all_boxes[j][i]) for j in (1, 2) for i in range(n_images)) > 10
    want = evaluate_detections(all_boxes, gt_roidb, classes)
    acc = DetectionAccumulator(K)
    for i0 in (0, 2):                                    # two batches: images 0-1, image 2
        m = (r[:, 0] >= i0) & (r[:, 0] < i0 + 2)
        rr = r[m].clone()
        rr[:, 0] -= i0
        dets, counts = post_detections_batched_device(s[m], b[m], rr, min(2, n_images - i0), K, 0.05, 20, max_rows_per_image=rows)
        acc.add(dets, counts, i0)
    got = evaluate_detections(acc, gt_roidb, classes)
    for k in ("aps", "mean_ap", "corloc_list", "froc_curve_pts"):
        assert got[k] == want[k], k
    assert np.array_equal(got["all_arr_ok"], want["all_arr_ok"]) and np.array_equal(got["num_fp_per_img"], want["num_fp_per_img"])
    for k in ("tp", "fp", "rec", "prec"):
        n = want["result"]["class_offsets"][-1]
        assert np.array_equal(to_np(got["result"][k])[:n], want["result"][k][:n]), k
