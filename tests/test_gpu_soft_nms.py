"""Soft-NMS on the device: wssdl_post_detections_soft against the NumPy statement (tests/soft_nms_reference.py), counts
equal and dets[:count] the same bits in the same order, for the hard, linear and Gaussian methods, on the segment sizes
where the kernel changes its path (lane, wave, workgroup edges, the LDS limit); method 0 against
wssdl_post_detections_views on the same device inputs; the cap below, at and above the number emitted; a floor that
retires rows in the middle of the loop; the overflow flag; the Python routes under every cfg.TEST.SOFT_NMS value;
detect_images under FLIP_AUG + SOFT_NMS end to end; the memory and stream-order contracts."""
import contextlib
import functools

import numpy as np
import pytest

import guarded_alloc
import soft_nms_reference as S
import stream_order
import tta_reference as T

pytestmark = pytest.mark.gpu

METHODS = (S.HARD, S.LINEAR, S.GAUSSIAN)
NAMES = {S.LINEAR: "linear", S.GAUSSIAN: "gaussian"}


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
    old = {k: cfg.TEST[k] for k in kv}
    try:
        for k, v in kv.items():
            cfg.TEST[k] = v
        yield cfg
    finally:
        for k, v in old.items():
            cfg.TEST[k] = v


def _t(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: the shared cases are read-only arrays)


# candidates per (image, class) segment: nothing, one, two; one short of a wave, a wave, one more; the same around the
# workgroup of 256; segment (4, 2) stays as drawn (about 265 of its 280 rows)
EDGES = {(0, 1): 0, (0, 2): 1, (1, 1): 2, (1, 2): 63, (2, 1): 64, (2, 2): 65, (3, 1): 255, (3, 2): 256, (4, 1): 257}

# (seed, rows per view of every image, views, K, builder keywords, max_per_image)
GRID = [
    (11, (12,), 1, 2, dict(mirrored=()), 300),
    (12, (140,) * 5, 2, 3, dict(mirrored=(1,), counts=EDGES), 0),                            # no cap: every pick is checked
    (13, (20, 0, 7), 2, 3, dict(mirrored=(1,), padded=40, plant="nms", low=((2, 1),)), 6),   # dead rows, an empty image
    (14, (15, 11), 3, 2, dict(mirrored=(1, 2), empty=((0, 2),), cap_ties=True), 2),
    (15, (24, 9), 1, 3, dict(mirrored=(), tie=True), 300),                                   # the planted decayed tie
    (16, (8,), 1, 65, dict(mirrored=()), 300),
    (17, (4096,), 1, 2, dict(mirrored=(), counts={(0, 1): 4096}, width=6000.0), 300),         # WSSDL_POST_SOFT_MAX_ROWS
]


@functools.lru_cache(maxsize=None)
def _case(i):
    seed, rows, views, K, kw, cap = GRID[i]
    c = S.build_case(seed, rows, views, K, **kw)
    c["cap"] = cap
    c["pitch"] = T.pitch_of(c)
    for k in ("rois", "scores", "boxes", "flip_width"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want(i, method, cap=None, floor=S.FLOOR):
    c = _case(i)
    return S.post_soft(c["rois"], c["scores"], c["boxes"], c["n_images"], c["views"], c["flip_width"], c["K"], S.THRESH,
                       c["cap"] if cap is None else cap, method, S.NMS, S.SIGMA, floor, pitch=c["pitch"])


def _run(torch, c, method, pitch=None, cap=None, floor=S.FLOOR):
    from wssdl_bus_amd.fast_rcnn.soft_nms import post_detections_soft_device
    ins = [_t(torch, c[k]) for k in ("scores", "boxes", "rois", "flip_width")]
    keep = [x.clone() for x in ins]
    dets, counts = post_detections_soft_device(ins[0], ins[1], ins[2], c["n_images"], c["views"], ins[3], c["K"],
                                               thresh=S.THRESH, max_per_image=c["cap"] if cap is None else cap, method=method,
                                               max_rows_per_image=pitch or c["pitch"], nms_thresh=S.NMS, sigma=S.SIGMA,
                                               min_score=floor)
    for a, b in zip(ins, keep):
        assert torch.equal(a, b), "the op wrote to an input"
    return dets.cpu().numpy(), counts.cpu().numpy()


def _rows_of(dets, counts, t, j):
    return dets[t, j - 1, :max(counts[t, j - 1], 0)]


def _assert_equal(c, got, want, tag):
    dets, counts = got
    N, K = c["n_images"], c["K"]
    assert dets.shape[:2] == (N, K - 1) and dets.shape[3] == 5 and counts.shape == (N, K - 1)
    for t in range(N):
        if want[t] is None:
            assert counts[t].tolist() == [-1] + [0] * (K - 2), (tag, t)
            continue
        for j in range(1, K):
            g = _rows_of(dets, counts, t, j)
            assert counts[t, j - 1] == len(want[t][j]), (tag, t, j, counts[t, j - 1], len(want[t][j]))
            assert T.same_bits(g, want[t][j]), (tag, t, j)
            assert np.all(g[:-1, 4] >= g[1:, 4])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", range(len(GRID)))
def test_op_equals_the_statement(torch_cuda, case, method):
    """the op == the statement: counts, bits and order, every image, every class; a second run gives the same bits"""
    c = _case(case)
    want = _want(case, method)
    got = _run(torch_cuda, c, method)
    print("soft case %d method %d: %d detections, %d exp calls in the Gaussian statement"
          % (case, method, int(got[1].sum()), c["exp_calls"]))
    _assert_equal(c, got, want, (case, method))
    assert got[1].sum() > 0
    again = _run(torch_cuda, c, method)
    assert np.array_equal(again[1], got[1])
    for t in range(c["n_images"]):
        for j in range(1, c["K"]):
            assert T.same_bits(_rows_of(*again, t, j), _rows_of(*got, t, j))


def test_the_grid_holds_what_it_is_there_for():
    """the segment sizes of the edge case, the limit, the planted pair and the planted tie are live in the statement"""
    c = _case(1)
    for (t, j), n in EDGES.items():
        s, _, _ = T.image_rows(c["rois"], c["scores"], c["boxes"], t, 2, 5, c["flip_width"])
        assert int((s[:, j] > np.float32(S.THRESH)).sum()) == n
        assert len(_want(1, S.GAUSSIAN)[t][j]) <= n
    assert len(_want(1, S.LINEAR)[4][1]) > 200                     # far more picks than one wave or one block holds
    from wssdl_bus_amd import _lib
    c = _case(6)
    assert c["pitch"] == _lib.POST_SOFT_MAX_ROWS == int((c["scores"][:, 1] > np.float32(S.THRESH)).sum())
    assert len(_want(6, S.GAUSSIAN, cap=0)[0][1]) > 1000
    # the pair at IoU = f32(0.3): gone under hard, decayed under linear
    hard, lin = _want(2, S.HARD, cap=0)[0][1], _want(2, S.LINEAR, cap=0)[0][1]
    assert (hard[:, 4] == np.float32(0.979)).sum() == 0 and (lin[:, 4] == np.float32(0.979)).sum() == 0
    assert (lin[:, 4] == np.float32(0.979) * (np.float32(1) - np.float32(0.3))).sum() == 1
    # the decayed tie: the later row (x1 = 275) first
    for m in (S.LINEAR, S.GAUSSIAN):
        w = _want(4, m)[0][1]
        i = int(np.where(w[:, 0] == 275)[0][0])
        assert w[i + 1, 0] == 325 and w[i, 4] == w[i + 1, 4]
    # the cap with ties: four rows share the top score, a cap of two keeps all four
    w = _want(3, S.LINEAR)[0][1]
    assert (w[:, 4] == np.float32(0.9975)).sum() == 4


@pytest.mark.parametrize("case", (0, 1, 2, 3, 4))
def test_method_0_is_the_views_op(torch_cuda, case):
    """hard method == wssdl_post_detections_views (agnostic 0, no voting) on the same device inputs: counts, bits, order"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_views_device
    c = _case(case)
    dets, counts = _run(torch, c, S.HARD, floor=S.THRESH)
    ins = [_t(torch, c[k]) for k in ("scores", "boxes", "rois", "flip_width")]
    vd, vc = post_detections_views_device(ins[0], ins[1], ins[2], c["n_images"], c["views"], ins[3], c["K"], thresh=S.THRESH,
                                          max_per_image=c["cap"], max_rows_per_image=c["pitch"], agnostic=False,
                                          vote_thresh=0.0)
    vd, vc = vd.cpu().numpy(), vc.cpu().numpy()
    assert np.array_equal(counts, vc) and counts.sum() > 0
    for t in range(c["n_images"]):
        for j in range(1, c["K"]):
            assert T.same_bits(_rows_of(dets, counts, t, j), _rows_of(vd, vc, t, j)), (t, j)


@pytest.mark.parametrize("method", (S.LINEAR, S.GAUSSIAN))
def test_cap_below_at_and_above_the_number_emitted(torch_cuda, method):
    c = _case(2)
    free = _want(2, method, cap=0)
    emitted = sum(len(free[0][j]) for j in (1, 2))
    assert emitted > 8
    for cap in (1, emitted - 1, emitted, emitted + 1, 0):
        want = _want(2, method, cap=cap)
        _assert_equal(c, _run(torch_cuda, c, method, cap=cap), want, (method, cap))
        kept = sum(len(want[0][j]) for j in (1, 2))
        assert kept == (emitted if cap == 0 else min(cap, emitted))


@pytest.mark.parametrize("method", (S.LINEAR, S.GAUSSIAN))
def test_a_high_floor_retires_rows_in_the_middle_of_the_loop(torch_cuda, method):
    c = _case(1)
    low, high = _want(1, method), _want(1, method, floor=0.3)
    n_low = sum(len(low[t][j]) for t in range(5) for j in (1, 2))
    n_high = sum(len(high[t][j]) for t in range(5) for j in (1, 2))
    above = sum(int((_case(1)["scores"][:, j] > np.float32(0.3)).sum()) for j in (1, 2))
    assert n_high < above and n_high < n_low / 2, "most decayed rows drop although they started above the floor"
    _assert_equal(c, _run(torch_cuda, c, method, floor=0.3), high, method)


def test_overflow_flag_and_raise(torch_cuda):
    """an output image whose views span more rows than the pitch: counts[t, 0] = -1, zeros in its other counts, the other
    images as before; postprocess_detections_batch raises"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    c = dict(S.build_case(41, (10, 22, 8), 2, 3), cap=300)
    c["pitch"] = 44
    want = S.post_soft(c["rois"], c["scores"], c["boxes"], 3, 2, c["flip_width"], 3, S.THRESH, 300, S.LINEAR, pitch=40)
    assert want[1] is None and want[0] is not None
    _assert_equal(c, _run(torch, c, S.LINEAR, pitch=40), want, "overflow")
    with _cfg_test(RPN_POST_NMS_TOP_N=20, SOFT_NMS="linear"):
        with pytest.raises(ValueError, match="more RoI rows"):
            postprocess_detections_batch(_t(torch, c["scores"]), _t(torch, c["boxes"]), _t(torch, c["rois"]), 3, 3, views=2,
                                         flip_width=_t(torch, c["flip_width"]))


# ------------------------------------------------------------------------------------------- Python routes ---
@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("method", (S.LINEAR, S.GAUSSIAN))
def test_python_routes_equal_the_statement(torch_cuda, monkeypatch, method, fused):
    """postprocess_detections_batch and the single-image postprocess_detections under cfg.TEST.SOFT_NMS, on the device
    op (the host path would raise) and, with FUSED_POST_DETECTIONS off, on the host path (the op would raise)"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn import soft_nms
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    from wssdl_bus_amd.fast_rcnn.post_detections import postprocess_detections

    def boom(*a, **k):
        raise AssertionError("the other route was taken")
    monkeypatch.setattr(soft_nms, "postprocess_soft_host" if fused else "post_detections_soft_device", boom)
    c = _case(2)
    N, V, K = c["n_images"], c["views"], c["K"]
    want = _want(2, method)
    with _cfg_test(SOFT_NMS=NAMES[method], FUSED_POST_DETECTIONS=fused, RPN_POST_NMS_TOP_N=40):
        got = postprocess_detections_batch(_t(torch, c["scores"]), _t(torch, c["boxes"]), _t(torch, c["rois"]), N, K,
                                           thresh=S.THRESH, max_per_image=c["cap"], views=V,
                                           flip_width=_t(torch, c["flip_width"]))
        s0, b0, _ = T.image_rows(c["rois"], c["scores"], c["boxes"], 0, V, N, c["flip_width"])
        one = postprocess_detections(_t(torch, s0), _t(torch, b0), K, S.THRESH, c["cap"])
    for t in range(N):
        for j in range(1, K):
            assert got[t][j].is_cuda and T.same_bits(got[t][j].cpu().numpy(), want[t][j]), (t, j)
    for j in range(1, K):
        assert T.same_bits(one[j].cpu().numpy(), want[0][j]), j


def test_off_is_the_parent_behaviour(torch_cuda, monkeypatch):
    """cfg.TEST.SOFT_NMS = 'off': the batched and the views op answer, bit for bit, and nothing of soft_nms runs"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn import soft_nms
    from wssdl_bus_amd.fast_rcnn.detect_batch import (post_detections_batched_device, post_detections_views_device,
                                                      postprocess_detections_batch)

    def boom(*a, **k):
        raise AssertionError("soft route reached")
    for name in ("postprocess_soft_batch", "postprocess_soft", "post_detections_soft_device"):
        monkeypatch.setattr(soft_nms, name, boom)
    c = _case(2)
    N, V, K = c["n_images"], c["views"], c["K"]
    ins = [_t(torch, c[k]) for k in ("scores", "boxes", "rois", "flip_width")]
    with _cfg_test(SOFT_NMS="off", RPN_POST_NMS_TOP_N=40):
        got = postprocess_detections_batch(ins[0], ins[1], ins[2], N, K, thresh=S.THRESH, max_per_image=6, views=V,
                                           flip_width=ins[3])
        vd, vc = post_detections_views_device(ins[0], ins[1], ins[2], N, V, ins[3], K, S.THRESH, 6)
        for t in range(N):
            for j in range(1, K):
                assert T.same_bits(got[t][j].cpu().numpy(), _rows_of(vd.cpu().numpy(), vc.cpu().numpy(), t, j))
        one = T.build_case(21, (30, 0, 17), 1, 3, mirrored=(), padded=40)
        a = [_t(torch, one[k]) for k in ("scores", "boxes", "rois")]
        got = postprocess_detections_batch(a[0], a[1], a[2], 3, 3, thresh=S.THRESH, max_per_image=7)
        bd, bc = post_detections_batched_device(a[0], a[1], a[2], 3, 3, S.THRESH, 7)
        for t in range(3):
            for j in (1, 2):
                assert T.same_bits(got[t][j].cpu().numpy(), _rows_of(bd.cpu().numpy(), bc.cpu().numpy(), t, j))


# ------------------------------------------------------------------------------------------------ contracts ---
def _dets_up_to_counts(result):
    """the defined region: rows of dets at and beyond a class's count are not written (include/wssdl_bus_hip.h)"""
    dets, counts = result
    n = counts.clamp_min(0).cpu().tolist()
    return [[dets[t, c, :n[t][c]] for c in range(dets.shape[1])] for t in range(dets.shape[0])], counts


CONTRACT = [(1, S.GAUSSIAN), (2, S.LINEAR), (3, S.GAUSSIAN), (4, S.HARD)]


def _contract_case(torch, i):
    from wssdl_bus_amd.fast_rcnn.soft_nms import post_detections_soft_device
    case, method = CONTRACT[i]
    c = _case(case)
    inputs = {k: _t(torch, c[k]) for k in ("scores", "boxes", "rois", "flip_width")}

    def fn(inp):
        return post_detections_soft_device(inp["scores"], inp["boxes"], inp["rois"], c["n_images"], c["views"],
                                           inp["flip_width"], c["K"], thresh=S.THRESH, max_per_image=c["cap"], method=method,
                                           max_rows_per_image=c["pitch"], nms_thresh=S.NMS, sigma=S.SIGMA, min_score=S.FLOOR)
    return fn, inputs


@pytest.mark.parametrize("i", range(len(CONTRACT)))
def test_memory_contract(torch_cuda, i):
    fn, inputs = _contract_case(torch_cuda, i)
    guarded_alloc.run_case(fn, inputs, name="post-soft-%d" % i, min_allocations=3, defined=_dets_up_to_counts)


@pytest.mark.parametrize("i", range(len(CONTRACT)))
def test_stream_order_contract(torch_cuda, i):
    fn, inputs = _contract_case(torch_cuda, i)
    stream_order.run_case(fn, inputs, name="post-soft-%d" % i, defined=_dets_up_to_counts)
    stream_order.assert_sync_free(fn, inputs, name="post-soft-%d" % i)


# ----------------------------------------------------------------------------------------------- end to end ---
def _planes():
    rs = np.random.RandomState(22)
    return [rs.randint(0, 256, size=shape).astype(np.uint8) for shape in ((300, 420), (380, 290), (260, 520))]


@pytest.fixture(scope="module")
def resnet18(torch_cuda):
    """random weights with scores all over (0, 1) and boxes that move: the rescaling of tests/test_gpu_tta.py"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import get_test_blobs, im_detect_batch
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(3)
    net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
    net.eval()
    data, info = get_test_blobs(_planes()[:1], "Resnet", flip_aug=False)
    im_detect_batch(net, data, info)
    with torch.no_grad():
        logits = net.layers['cls_score'].float()
        k = 1.0 / float((logits - logits.mean(0)).std())
        net.cls_score.weight.mul_(k)
        net.cls_score.bias.copy_(-k * logits.mean(0))
        net.bbox_pred.weight.mul_(0.2 / float(net.layers['bbox_pred'].std()))
    return net


def test_detect_images_under_flip_aug_and_soft_nms(torch_cuda, resnet18, monkeypatch):
    """detect_images under FLIP_AUG + SOFT_NMS == the statement applied to im_detect_batch's own outputs (one forward,
    its outputs handed to both); accumulate_images keeps the same detections on the device"""
    from wssdl_bus_amd.fast_rcnn import detect_batch, eval_batch
    from wssdl_bus_amd.fast_rcnn.config import cfg
    planes = _planes()
    seen = []
    real = detect_batch.im_detect_batch

    def once(net, data, info):
        if not seen:
            seen.append(real(net, data, info))
        assert data.shape[0] == 6
        return seen[0]
    monkeypatch.setattr(detect_batch, "im_detect_batch", once)
    monkeypatch.setattr(eval_batch, "im_detect_batch", once)
    fw = np.asarray([-1, 420, -1, 290, -1, 520], np.float32)
    for method in (S.LINEAR, S.GAUSSIAN):
        with _cfg_test(FLIP_AUG=True, SOFT_NMS=NAMES[method], RPN_PRE_NMS_TOP_N=250):
            all_boxes = detect_batch.detect_images(resnet18, planes, "Resnet", batch_size=3, max_per_image=40)
            acc = eval_batch.accumulate_images(resnet18, planes, "Resnet", batch_size=3, max_per_image=40)
            scores, boxes, rois = (x.cpu().numpy() for x in seen[0])
            K = scores.shape[1]
            if method == S.GAUSSIAN:
                case = dict(rois=rois, scores=scores, boxes=boxes, flip_width=fw, n_images=3, views=2, K=K)
                assert S.gaussian_is_safe(case, nms_thresh=cfg.TEST.NMS)[0], "an exp of this forward is not safe"
            want = S.post_soft(rois, scores, boxes, 3, 2, fw, K, 0.05, 40, method, cfg.TEST.NMS, cfg.TEST.SOFT_NMS_SIGMA,
                               cfg.TEST.SOFT_NMS_MIN_SCORE)
        n_det = 0
        for t in range(3):
            for j in range(1, K):
                assert T.same_bits(all_boxes[j][t], want[t][j]), (method, t, j)
                n_det += len(want[t][j])
        assert n_det >= 40
        assert acc is not None and acc.num_classes == K
