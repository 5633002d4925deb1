"""Class-agnostic post-detection step on the device (cfg.TEST.CLS_AGNOSTIC_NMS): wssdl_post_detections_agnostic_batched
against the single-image op on every image's rows (bit for bit), against the NumPy statement of the reference
(tests/post_agnostic_reference.py), against the per-class op for K = 2 (bit for bit) and against the step-by-step form
of test_bus.postprocess_detections (bit for bit); the routing of post_detections.postprocess_detections /
postprocess_detections_batch, the overflow flag, and accumulate_images under the flag."""
import contextlib

import numpy as np
import pytest

import post_agnostic_reference as REF

pytestmark = pytest.mark.gpu

THRESH = 0.05


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    _lib.lib()
    return torch


@contextlib.contextmanager
def _cfg_test(**kv):
    from wssdl_bus_amd.fast_rcnn.config import cfg
    missing = object()
    old = {k: cfg.TEST.get(k, missing) for k in kv}
    try:
        for k, v in kv.items():
            cfg.TEST[k] = v
        yield cfg
    finally:
        for k, v in old.items():
            if v is missing:
                del cfg.TEST[k]
            else:
                cfg.TEST[k] = v


def _same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _image_rows(rs, n, K, ties):
    """n rows of one image: scores [n,K] in [0,1), class-wise boxes [n,4K]; the class boxes of one row share a centre
    (the union pass has a lot to suppress); with `ties` the first eight rows of class 1 share one score and sit far
    apart (no two of them suppress each other)."""
    ctr = rs.uniform(50, 900, size=(n, 1, 2)) * [1.0, 0.6] + rs.normal(0, 6, size=(n, K, 2))
    wh = rs.uniform(30, 220, size=(n, K, 2))
    boxes = np.concatenate((ctr - wh / 2, ctr + wh / 2), axis=2).reshape(n, 4 * K).astype(np.float32)
    scores = rs.uniform(0, 1, size=(n, K)).astype(np.float32)
    if ties and n > 8:
        scores[:8, 1] = np.float32(0.625)
        boxes[:8, 4:8] = boxes[:8, 4:8] + np.arange(8, dtype=np.float32)[:, None] * 1500
    return scores, boxes


def _blob(rs, counts, K, padded=None, ties=False, low=()):
    """RoI blob of len(counts) images in ascending order: compact (padded=None) or padded to `padded` rows per
    image with dead rows (batch index -1, garbage values).  Images listed in `low` score below every threshold."""
    rois, scores, boxes, per_image = [], [], [], []
    for i, n in enumerate(counts):
        s, b = _image_rows(rs, n, K, ties)
        if i in low:
            s[:] = np.float32(0.01)
        per_image.append((s, b))
        r = np.zeros((n, 5), np.float32)
        r[:, 0] = i
        r[:, 1:] = rs.uniform(0, 500, size=(n, 4))
        rois.append(r)
        scores.append(s)
        boxes.append(b)
        if padded is not None:
            d = padded - n
            dr = rs.uniform(0, 500, size=(d, 5)).astype(np.float32)
            dr[:, 0] = -1
            rois.append(dr)
            scores.append(rs.uniform(0, 1, size=(d, K)).astype(np.float32))
            boxes.append(rs.uniform(0, 900, size=(d, 4 * K)).astype(np.float32))
    cat = lambda xs, w: np.concatenate(xs) if xs else np.zeros((0, w), np.float32)      # noqa: E731
    return cat(rois, 5), cat(scores, K), cat(boxes, 4 * K), per_image


def _canon(a):
    """rows of EQUAL score come in an order the reference leaves to argsort"""
    a = np.asarray(a).reshape(-1, 5)
    return a[np.lexsort((a[:, 0], a[:, 1], -a[:, 4]))] if len(a) else a


# (counts per image, K, max_per_image, padded pitch or None, ties, images scoring below thresh)
CASES = [
    ((300,), 3, 300, None, True, ()),
    ((63, 64, 65), 3, 5, None, True, ()),                           # U = 2 * 65: the chunk edge inside the union
    ((0, 1, 300), 2, 300, 300, False, ()),
    ((64, 0, 65, 300, 1, 63, 17, 200), 3, 0, 300, True, ()),
    ((40, 90, 12, 77, 5, 64, 31, 100), 3, 5, None, False, (2,)),
    (tuple([0, 1, 63, 64, 65] * 8), 3, 300, None, False, ()),       # 40 images
    ((21, 22, 0, 5), 9, 7, 22, True, ()),                           # U = 176, eight classes, the cap inside the union
    ((0,), 3, 300, None, False, ()),                                # no row at all
]


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_batched(torch, rois, scores, boxes, N, K, cap, P, agnostic=True):
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device
    dets, counts = post_detections_batched_device(_t(torch, scores), _t(torch, boxes), _t(torch, rois), N, K, thresh=THRESH,
                                                  max_per_image=cap, max_rows_per_image=P, agnostic=agnostic)
    return dets.cpu().numpy(), counts.cpu().numpy()


def _run_single(torch, s, b, K, cap, agnostic=True):
    from wssdl_bus_amd.fast_rcnn.post_detections import post_detections_device
    d1, c1 = post_detections_device(_t(torch, s), _t(torch, b), K, thresh=THRESH, max_per_image=cap, agnostic=agnostic)
    return d1.cpu().numpy(), c1.cpu().numpy()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_agnostic_op_single_batched_oracle_and_step_by_step(torch_cuda, case):
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.test_bus import postprocess_detections
    counts_in, K, cap, padded, ties, low = CASES[case]
    rs = np.random.RandomState(300 + case)
    rois, scores, boxes, per_image = _blob(rs, counts_in, K, padded, ties, low)
    nms_thresh = cfg.TEST.NMS
    # precondition (CPU): equal scores above the threshold never belong to boxes that could suppress each other, so
    # the reference's undefined argsort order among them cannot show in its result
    for s, b in per_image:
        assert REF.ties_are_harmless(s, b, K, THRESH, nms_thresh), case
    N = len(counts_in)
    P = padded if padded is not None else max(max(counts_in), 1)
    dets, counts = _run_batched(torch, rois, scores, boxes, N, K, cap, P)
    assert dets.shape == (N, K - 1, P, 5) and counts.shape == (N, K - 1)
    if K == 2:
        # 3. nothing is left for the union pass to suppress: the per-class op, bit for bit
        pd, pc = _run_batched(torch, rois, scores, boxes, N, K, cap, P, agnostic=False)
        assert np.array_equal(counts, pc), case
        for i in range(N):
            assert _same_bits(dets[i, 0, :counts[i, 0]], pd[i, 0, :pc[i, 0]]), (case, i)
    removed = 0
    for i, (s, b) in enumerate(per_image):
        n = s.shape[0]
        # 1. bit for bit the single-image agnostic op on the image's rows alone
        d1, c1 = _run_single(torch, s, b, K, cap)
        assert np.array_equal(counts[i], c1), (case, i)
        for c in range(K - 1):
            assert _same_bits(dets[i, c, :counts[i, c]], d1[c, :c1[c]]), (case, i, c)
        # 2. the NumPy statement of the reference
        want = REF.post_detections(s, b, K, THRESH, cap, nms_thresh)
        for j in range(1, K):
            got = dets[i, j - 1, :counts[i, j - 1]]
            assert np.array_equal(_canon(got), _canon(want[j])), (case, i, j)
            assert np.all(got[:-1, 4] >= got[1:, 4])
        if i in low:
            assert not counts[i].any()
        removed += sum(len(v) for v in REF.post_detections(s, b, K, THRESH, 0, nms_thresh, agnostic=False).values()) - \
            sum(len(v) for v in REF.post_detections(s, b, K, THRESH, 0, nms_thresh).values())
        # 4. the step-by-step form (per-class hip_nms calls, concatenation, one more hip_nms, masks), bit for bit
        with _cfg_test(CLS_AGNOSTIC_NMS=True, FUSED_POST_DETECTIONS=False):
            steps = postprocess_detections(_t(torch, s), _t(torch, b), K, thresh=THRESH, max_per_image=cap)
        for j in range(1, K):
            assert _same_bits(dets[i, j - 1, :counts[i, j - 1]], steps[j].cpu().numpy()), (case, i, j)
        assert n > 0 or not counts[i].any()
    # the union pass is not idle in the cases with more than one object class and rows above the threshold
    if K > 2 and sum(counts_in) > 8:
        assert removed > 0, case


# Unions beyond one mask segment, where launch_rank_topk and launch_nms_two_pass change kernels (K = 3, U = 2 * rows):
# 2208 -- mask and sweep in one launch (2048 <= U <= 2240); 2600 -- the general sweep (more than 2240 to keep), here
# for two images at once; 4208 -- the bucketed ranking (4096 and up).
LARGE = [((1104,), 300), ((1300, 700), 0), ((2104,), 300)]


@pytest.mark.parametrize("case", range(len(LARGE)))
def test_agnostic_op_large_unions(torch_cuda, case):
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.test_bus import postprocess_detections
    counts_in, cap = LARGE[case]
    K = 3
    rs = np.random.RandomState(400 + case)
    rois, scores, boxes, per_image = _blob(rs, counts_in, K)
    for s, b in per_image:
        assert REF.ties_are_harmless(s, b, K, THRESH, cfg.TEST.NMS), case
    N, P = len(counts_in), max(counts_in)
    dets, counts = _run_batched(torch, rois, scores, boxes, N, K, cap, P)
    for i, (s, b) in enumerate(per_image):
        d1, c1 = _run_single(torch, s, b, K, cap)
        assert np.array_equal(counts[i], c1), (case, i)
        want = REF.post_detections(s, b, K, THRESH, cap, cfg.TEST.NMS)
        with _cfg_test(CLS_AGNOSTIC_NMS=True, FUSED_POST_DETECTIONS=False):
            steps = postprocess_detections(_t(torch, s), _t(torch, b), K, thresh=THRESH, max_per_image=cap)
        for j in range(1, K):
            got = dets[i, j - 1, :counts[i, j - 1]]
            assert _same_bits(got, d1[j - 1, :c1[j - 1]]), (case, i, j)
            assert np.array_equal(_canon(got), _canon(want[j])), (case, i, j)
            assert np.all(got[:-1, 4] >= got[1:, 4])
            assert _same_bits(got, steps[j].cpu().numpy()), (case, i, j)
        assert counts[i].sum() > 0


def test_two_classes_with_equal_scores(torch_cuda):
    """K = 2 with equal scores among the kept rows: the union ranks them by the later kept row first, as hip_nms on
    the concatenation does -- the step-by-step form bit for bit, the per-class op only up to the order of the ties."""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.test_bus import postprocess_detections
    K, counts_in = 2, (20, 64)
    rs = np.random.RandomState(77)
    rois, scores, boxes, per_image = _blob(rs, counts_in, K, ties=True)
    dets, counts = _run_batched(torch, rois, scores, boxes, 2, K, 300, 64)
    pd, pc = _run_batched(torch, rois, scores, boxes, 2, K, 300, 64, agnostic=False)
    assert np.array_equal(counts, pc)
    for i, (s, b) in enumerate(per_image):
        assert REF.ties_are_harmless(s, b, K, THRESH, cfg.TEST.NMS)
        got = dets[i, 0, :counts[i, 0]]
        assert (got[:, 4] == np.float32(0.625)).sum() == 8
        assert np.array_equal(_canon(got), _canon(REF.post_detections(s, b, K, THRESH, 300, cfg.TEST.NMS)[1]))
        assert np.array_equal(_canon(got), _canon(pd[i, 0, :pc[i, 0]]))
        with _cfg_test(CLS_AGNOSTIC_NMS=True, FUSED_POST_DETECTIONS=False):
            steps = postprocess_detections(_t(torch, s), _t(torch, b), K, thresh=THRESH, max_per_image=300)
        assert _same_bits(got, steps[1].cpu().numpy()), i
        d1, c1 = _run_single(torch, s, b, K, 300)
        assert np.array_equal(counts[i], c1) and _same_bits(got, d1[0, :c1[0]]), i


def _raise_hip_nms(*a, **k):
    raise RuntimeError("step-by-step form reached")


def test_flag_routes_to_the_device_op(torch_cuda, monkeypatch):
    """Under CLS_AGNOSTIC_NMS both entry points take the device op (no hip_nms call, and the op itself reads nothing
    back); beyond the union bound or with FUSED_POST_DETECTIONS off the step-by-step form is still what runs."""
    torch = torch_cuda
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.fast_rcnn import post_detections, test_bus
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device, postprocess_detections_batch
    rs = np.random.RandomState(17)
    K, counts_in = 3, (120, 0, 300, 64)
    rois, scores, boxes, per_image = _blob(rs, counts_in, K, padded=300)
    monkeypatch.setattr(test_bus, "hip_nms", _raise_hip_nms)
    with _cfg_test(CLS_AGNOSTIC_NMS=True):
        got = postprocess_detections_batch(_t(torch, scores), _t(torch, boxes), _t(torch, rois), 4, K, thresh=THRESH,
                                           max_per_image=50)
        assert len(got) == 4
        for i, (s, b) in enumerate(per_image):
            assert REF.ties_are_harmless(s, b, K, THRESH, cfg.TEST.NMS)
            want = REF.post_detections(s, b, K, THRESH, 50, cfg.TEST.NMS)
            one = post_detections.postprocess_detections(_t(torch, s), _t(torch, b), K, thresh=THRESH, max_per_image=50)
            for j in range(1, K):
                assert np.array_equal(_canon(got[i][j].cpu().numpy()), _canon(want[j])), (i, j)
                assert _same_bits(got[i][j].cpu().numpy(), one[j].cpu().numpy()), (i, j)
        # the flag decides: the per-class detections are more
        n_agnostic = sum(int(d[j].shape[0]) for d in got for j in range(1, K))
        # the batched op enqueues and returns: no read-back, no synchronisation
        ts, tb, tr = _t(torch, scores), _t(torch, boxes), _t(torch, rois)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            dets, counts = post_detections_batched_device(ts, tb, tr, 4, K, THRESH, 50)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert int(counts.clamp(min=0).sum()) == n_agnostic
    per_class = postprocess_detections_batch(_t(torch, scores), _t(torch, boxes), _t(torch, rois), 4, K, thresh=THRESH,
                                             max_per_image=0)
    with _cfg_test(CLS_AGNOSTIC_NMS=True):
        agnostic = postprocess_detections_batch(_t(torch, scores), _t(torch, boxes), _t(torch, rois), 4, K, thresh=THRESH,
                                                max_per_image=0)
    count = lambda ds: sum(int(d[j].shape[0]) for d in ds for j in range(1, K))      # noqa: E731
    assert count(agnostic) < count(per_class)
    # the fallback is still there: FUSED_POST_DETECTIONS off ...
    s0, b0 = per_image[0]
    with _cfg_test(CLS_AGNOSTIC_NMS=True, FUSED_POST_DETECTIONS=False):
        with pytest.raises(RuntimeError, match="step-by-step form reached"):
            post_detections.postprocess_detections(_t(torch, s0), _t(torch, b0), K, thresh=THRESH)
        with pytest.raises(RuntimeError, match="step-by-step form reached"):
            postprocess_detections_batch(_t(torch, scores), _t(torch, boxes), _t(torch, rois), 4, K, thresh=THRESH)
    # ... and a union over the declared bound, (K-1) * R of one image
    over = _lib.POST_AGNOSTIC_MAX_UNION // (K - 1) + 1
    big_s = np.zeros((over, K), np.float32)
    big_b = np.zeros((over, 4 * K), np.float32)
    big_s[:len(s0)], big_b[:len(b0)] = s0, b0
    with _cfg_test(CLS_AGNOSTIC_NMS=True):
        with pytest.raises(RuntimeError, match="step-by-step form reached"):
            post_detections.postprocess_detections(_t(torch, big_s), _t(torch, big_b), K, thresh=THRESH)
        with _cfg_test(RPN_POST_NMS_TOP_N=over):
            # a batch whose pitch puts the union over the bound loops over the images with postprocess_detections,
            # which takes every image by its own rows (here the single-image device op): the same detections
            looped = postprocess_detections_batch(_t(torch, scores), _t(torch, boxes), _t(torch, rois), 4, K, thresh=THRESH,
                                                  max_per_image=50)
            for i in range(4):
                for j in range(1, K):
                    assert _same_bits(looped[i][j].cpu().numpy(), got[i][j].cpu().numpy()), (i, j)
            with pytest.raises(ValueError, match="WSSDL_POST_AGNOSTIC_MAX_UNION"):
                post_detections_batched_device(_t(torch, scores), _t(torch, boxes), _t(torch, rois), 4, K, THRESH)
    # without the flag the same shapes take the per-class device op as before
    post_detections.postprocess_detections(_t(torch, big_s), _t(torch, big_b), K, thresh=THRESH)


def test_agnostic_overflow_flag_and_raise(torch_cuda):
    """An image with more live rows than max_rows_per_image: counts[i, 0] == -1 on the device, the other images equal
    their single-image results, and postprocess_detections_batch raises."""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    rs = np.random.RandomState(5)
    K = 3
    rois, scores, boxes, per_image = _blob(rs, (30, 50, 20), K)
    dets, counts = _run_batched(torch, rois, scores, boxes, 3, K, 300, 40)
    assert counts[1].tolist() == [-1, 0]
    for i in (0, 2):
        d1, c1 = _run_single(torch, per_image[i][0], per_image[i][1], K, 300)
        assert np.array_equal(counts[i], c1) and c1.sum() > 0
        for c in range(K - 1):
            assert _same_bits(dets[i, c, :counts[i, c]], d1[c, :c1[c]]), (i, c)
    with _cfg_test(CLS_AGNOSTIC_NMS=True, RPN_POST_NMS_TOP_N=40):
        with pytest.raises(ValueError, match="more RoI rows"):
            postprocess_detections_batch(_t(torch, scores), _t(torch, boxes), _t(torch, rois), 3, K)


def test_accumulate_images_scores_the_agnostic_detections(torch_cuda, monkeypatch):
    """accumulate_images under the flag -> evaluate_detections, against evaluate_detections on the host lists of
    postprocess_detections_batch, value for value; and not what the flag-off run gives.  (The network is replaced by
    one synthetic blob: 3 images x 40 rows, K = 3.)"""
    torch = torch_cuda
    from wssdl_bus_amd.datasets.voc_eval_bus import evaluate_detections
    from wssdl_bus_amd.fast_rcnn import eval_batch
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    K, n_images, rows = 3, 3, 40
    rs = np.random.RandomState(23)
    rois, scores, boxes, per_image = _blob(rs, (rows,) * n_images, K)
    s, b, r = _t(torch, scores), _t(torch, boxes), _t(torch, rois)
    gt_roidb = []
    for i in range(n_images):
        # ground truth = three of the image's own class boxes
        pick = rs.choice(rows, 3, replace=False)
        cls = np.array([1, 2, 1])
        gtb = np.stack([per_image[i][1][p, 4 * c:4 * c + 4] for p, c in zip(pick, cls)])
        gt_roidb.append(dict(boxes=np.rint(gtb).astype(np.int64) + 1, gt_classes=cls, difficult=np.array([0, 0, 1])))
    classes = ("__background__", "benign", "malignant")
    monkeypatch.setattr(eval_batch, "get_test_blobs", lambda planes, net_name: (torch.zeros((len(planes), 4, 4, 3)), None))
    monkeypatch.setattr(eval_batch, "im_detect_batch", lambda net, data, info: (s, b, r))
    planes = [None] * n_images

    def host_route():
        per = postprocess_detections_batch(s, b, r, n_images, K, THRESH, 20)
        all_boxes = [[[] for _ in range(n_images)] for _ in range(K)]
        for i, d in enumerate(per):
            for j in range(1, K):
                all_boxes[j][i] = d[j].cpu().numpy()
        return all_boxes

    keys = ("aps", "mean_ap", "corloc_list", "froc_curve_pts")
    with _cfg_test(CLS_AGNOSTIC_NMS=True):
        all_boxes = host_route()
        want = evaluate_detections(all_boxes, gt_roidb, classes)
        got = evaluate_detections(eval_batch.accumulate_images(None, planes, "Resnet", batch_size=8, thresh=THRESH,
                                                               max_per_image=20), gt_roidb, classes)
    for k in keys:
        assert got[k] == want[k], k
    assert np.array_equal(got["all_arr_ok"], want["all_arr_ok"]) and np.array_equal(got["num_fp_per_img"], want["num_fp_per_img"])
    # flag off: more detections (the union pass removes some), another result
    off_boxes = host_route()
    n_on = sum(len(all_boxes[j][i]) for j in (1, 2) for i in range(n_images))
    n_off = sum(len(off_boxes[j][i]) for j in (1, 2) for i in range(n_images))
    uncapped = lambda flag: sum(len(v) for sb in per_image        # noqa: E731
                                for v in REF.post_detections(sb[0], sb[1], K, THRESH, 0, 0.3, agnostic=flag).values())
    assert uncapped(True) < uncapped(False) and n_on > 10 and n_off >= n_on
    off = evaluate_detections(eval_batch.accumulate_images(None, planes, "Resnet", batch_size=8, thresh=THRESH,
                                                           max_per_image=20), gt_roidb, classes)
    assert off["result"]["class_offsets"][-1] == n_off
    assert got["result"]["class_offsets"][-1] == n_on
    assert any(off[k] != got[k] for k in keys) or not np.array_equal(off["num_fp_per_img"], got["num_fp_per_img"])
