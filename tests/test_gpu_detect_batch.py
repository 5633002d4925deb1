"""Batched test-time detection (f3 over a batch): wssdl_post_detections_batched against the single-image op on every
image's rows (bit for bit) and against the NumPy oracle, and the Python path (get_test_blobs -> im_detect_batch ->
postprocess_detections_batch) against im_detect's single-image arithmetic on the same network outputs."""
import numpy as np
import pytest

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    _lib.lib()
    return torch


def _same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _image_rows(rs, n, K, ties):
    """n rows of one image: scores [n,K] in [0,1), class-wise boxes [n,4K]; with `ties` the first eight rows of
    class 1 share one score and sit far apart (no two of them suppress each other)."""
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


def _oracle(scores, boxes, K, thresh, cap, nms_thresh):
    want = {}
    for j in range(1, K):
        inds = np.where(scores[:, j] > thresh)[0]
        d = np.hstack((boxes[inds, 4 * j:4 * j + 4], scores[inds, j:j + 1])).astype(np.float32)
        want[j] = d[O.nms(d, nms_thresh)] if len(d) else d.reshape(0, 5)
    alls = np.hstack([want[j][:, 4] for j in range(1, K)])
    if cap > 0 and len(alls) > cap:
        th = np.sort(alls)[-cap]
        for j in range(1, K):
            want[j] = want[j][want[j][:, 4] >= th]
    return want


def _canon(a):
    """rows of EQUAL score come in an order the reference leaves to argsort"""
    a = np.asarray(a).reshape(-1, 5)
    return a[np.lexsort((a[:, 0], a[:, 1], -a[:, 4]))] if len(a) else a


# (counts per image, K, max_per_image, padded pitch or None, ties, images scoring below thresh)
CASES = [
    ((300,), 3, 300, None, True, ()),
    ((63, 64, 65), 3, 5, None, True, ()),
    ((0, 1, 300), 2, 300, 300, False, ()),
    ((64, 0, 65, 300, 1, 63, 17, 200), 3, 0, 300, True, ()),
    ((40, 90, 12, 77, 5, 64, 31, 100), 2, 5, None, False, (2,)),
    (tuple([0, 1, 63, 64, 65] * 8), 3, 300, None, False, ()),     # 40 images, 80 segments
    (tuple([0, 1, 63, 64, 65] * 8), 2, 5, 65, True, (7,)),         # 40 images, padded
    ((64, 1, 65), 65, 300, None, False, ()),                       # 64 classes: 192 segments
    ((65, 0, 20), 65, 5, 65, True, ()),
    ((0,), 3, 300, None, False, ()),                               # no row at all
]


def _run_batched(torch, rois, scores, boxes, N, K, cap, P):
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    dets, counts = post_detections_batched_device(t(scores), t(boxes), t(rois), N, K, thresh=0.05, max_per_image=cap,
                                                  max_rows_per_image=P)
    return dets.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_batched_op_matches_single_image_op_and_oracle(torch_cuda, case):
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.test_bus import post_detections_device
    counts_in, K, cap, padded, ties, low = CASES[case]
    rs = np.random.RandomState(100 + case)
    rois, scores, boxes, per_image = _blob(rs, counts_in, K, padded, ties, low)
    N = len(counts_in)
    P = padded if padded is not None else max(max(counts_in), 1)
    dets, counts = _run_batched(torch, rois, scores, boxes, N, K, cap, P)
    assert dets.shape == (N, K - 1, P, 5) and counts.shape == (N, K - 1)
    for i, (s, b) in enumerate(per_image):
        n = s.shape[0]
        # 1. bit for bit the single-image op on the image's rows alone
        d1, c1 = post_detections_device(torch.from_numpy(s).cuda(), torch.from_numpy(b).cuda(), K, thresh=0.05,
                                        max_per_image=cap)
        d1, c1 = d1.cpu().numpy(), c1.cpu().numpy()
        assert np.array_equal(counts[i], c1), (case, i)
        for c in range(K - 1):
            assert _same_bits(dets[i, c, :counts[i, c]], d1[c, :c1[c]]), (case, i, c)
        # 2. the oracle: NMS + the cap formula
        want = _oracle(s, b, K, 0.05, cap, cfg.TEST.NMS) if n else {j: np.zeros((0, 5), np.float32) for j in range(1, K)}
        for j in range(1, K):
            got = dets[i, j - 1, :counts[i, j - 1]]
            assert np.array_equal(_canon(got), _canon(want[j])), (case, i, j)
            assert np.all(got[:-1, 4] >= got[1:, 4])
        if i in low:
            assert not counts[i].any()


def test_batched_op_overflow_flag_and_raise(torch_cuda):
    """An image with more live rows than max_rows_per_image: counts[i, 0] == -1 on the device (the other images
    are unaffected), and postprocess_detections_batch raises."""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    rs = np.random.RandomState(5)
    rois, scores, boxes, _ = _blob(rs, (30, 50, 20), 3)
    dets, counts = _run_batched(torch, rois, scores, boxes, 3, 3, 300, 40)
    assert counts[1].tolist() == [-1, 0]
    _, ref = _run_batched(torch, rois, scores, boxes, 3, 3, 300, 50)
    assert np.array_equal(counts[[0, 2]], ref[[0, 2]])
    old = cfg.TEST.RPN_POST_NMS_TOP_N
    try:
        cfg.TEST.RPN_POST_NMS_TOP_N = 40
        t = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
        with pytest.raises(ValueError, match="more RoI rows"):
            postprocess_detections_batch(t(scores), t(boxes), t(rois), 3, 3)
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N = old


def test_batched_fallbacks_equal_per_image_loop(torch_cuda):
    """CLS_AGNOSTIC_NMS and FUSED_POST_DETECTIONS off take the per-image loop of postprocess_detections; the device
    path gives the same as that loop too."""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    from wssdl_bus_amd.fast_rcnn.test_bus import postprocess_detections
    rs = np.random.RandomState(9)
    rois, scores, boxes, per_image = _blob(rs, (120, 0, 300, 64), 3, padded=300)
    t = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    for key, value in ((None, None), ("CLS_AGNOSTIC_NMS", True), ("FUSED_POST_DETECTIONS", False)):
        old = cfg.TEST[key] if key else None
        try:
            if key:
                cfg.TEST[key] = value
            got = postprocess_detections_batch(t(scores), t(boxes), t(rois), 4, 3, thresh=0.05, max_per_image=50)
            assert len(got) == 4
            for i, (s, b) in enumerate(per_image):
                want = postprocess_detections(t(s), t(b), 3, thresh=0.05, max_per_image=50)
                for j in (1, 2):
                    assert _same_bits(got[i][j].cpu().numpy(), want[j].cpu().numpy()), (key, i, j)
        finally:
            if key:
                cfg.TEST[key] = old


@pytest.fixture(scope="module")
def resnet18(torch_cuda):
    torch = torch_cuda
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(3)
    net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
    net.eval()
    return net


def _planes():
    rs = np.random.RandomState(21)
    return [rs.randint(0, 256, size=shape).astype(np.uint8) for shape in ((300, 420), (380, 290), (260, 520), (410, 330))]


def _check_end_to_end(torch, net, padded):
    """im_detect_batch + postprocess_detections_batch against im_detect's arithmetic and postprocess_detections on
    every image's rows of the SAME network outputs."""
    from wssdl_bus_amd.fast_rcnn.bbox_transform import bbox_transform_inv
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.detect_batch import get_test_blobs, im_detect_batch, postprocess_detections_batch
    from wssdl_bus_amd.fast_rcnn.test_bus import _clip_boxes, postprocess_detections
    data, info = get_test_blobs(_planes(), "Resnet")
    assert data.shape[0] == 4 and info.shape == (4, 3)
    assert len({tuple(r) for r in info.cpu().numpy().tolist()}) == 4          # four distinct im_info rows
    assert (info[:, 0] < data.shape[1]).any() and (info[:, 1] < data.shape[2]).any()    # padding is involved
    old = cfg.PADDED_ROIS, cfg.TEST.RPN_PRE_NMS_TOP_N
    try:
        cfg.PADDED_ROIS = padded
        # at most 250 proposals per image against a pitch of RPN_POST_NMS_TOP_N = 300: the padded blob has dead rows
        cfg.TEST.RPN_PRE_NMS_TOP_N = 250
        if padded:
            # nothing in the forward or the decode reads the device back
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                scores, boxes, rois = im_detect_batch(net, data, info)
            finally:
                torch.cuda.set_sync_debug_mode(0)
        else:
            scores, boxes, rois = im_detect_batch(net, data, info)
        layers = net.layers
        got = postprocess_detections_batch(scores, boxes, rois, 4, scores.shape[1])
    finally:
        cfg.PADDED_ROIS, cfg.TEST.RPN_PRE_NMS_TOP_N = old
    K = scores.shape[1]
    batch = layers['rpn_rois'][:, 0]
    assert bool((batch < 0).any()) == padded
    n_det = 0
    for i in range(4):
        rows = torch.nonzero(batch == i).reshape(-1)
        assert rows.numel() > 0
        r_i, s_i, d_i = layers['rpn_rois'][rows], layers['cls_prob'][rows], layers['bbox_pred'][rows]
        # im_detect's single-image arithmetic (test_bus.py im_detect), verbatim
        scale = float(info[i, 2])
        b = r_i[:, 1:5] / scale
        pred = bbox_transform_inv(b, d_i)
        pred = _clip_boxes(pred, (float(info[i, 0]) / scale, float(info[i, 1]) / scale))
        assert _same_bits(boxes[rows].cpu().numpy(), pred.cpu().numpy()), (padded, i)
        want = postprocess_detections(s_i, pred, K)
        for j in range(1, K):
            assert _same_bits(got[i][j].cpu().numpy(), want[j].cpu().numpy()), (padded, i, j)
            n_det += int(want[j].shape[0])
    assert n_det > 0
    return scores


def test_end_to_end_batch_equals_single_image_arithmetic(torch_cuda, resnet18):
    _check_end_to_end(torch_cuda, resnet18, padded=False)


def test_end_to_end_padded_rois_sync_free(torch_cuda, resnet18):
    _check_end_to_end(torch_cuda, resnet18, padded=True)


def test_detect_images_structure(torch_cuda, resnet18):
    """detect_images: all_boxes[j][i] numpy [n,5] for every class j >= 1 and image i, batches of 3 over 4 images
    (a full batch and a short one), best first.  (Not compared with other forwards: the convolutions and GEMMs may
    round differently from one forward to another.)"""
    from wssdl_bus_amd.fast_rcnn.detect_batch import detect_images
    planes = _planes()
    all_boxes = detect_images(resnet18, planes, "Resnet", batch_size=3)
    K = len(all_boxes)
    assert K == 3 and all(len(all_boxes[j]) == 4 for j in range(K))
    for j in range(1, K):
        for i in range(4):
            a = all_boxes[j][i]
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 5
            assert np.all(a[:-1, 4] >= a[1:, 4]) and np.all(a[:, 4] > 0.05)
    assert sum(len(all_boxes[j][i]) for j in range(1, K) for i in range(4)) > 0
    assert all_boxes[0] == [[], [], [], []]
