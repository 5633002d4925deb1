"""GPU: the proposal-recall op (wssdl_proposal_recall through datasets.recall.evaluate_recall_table) against the
package's host path on the cases of tests/recall_cases.py, and the RPN-only forward of rpn_msr/generate.py against
the networks' own forward.  Every comparison is bit for bit: integers equal, f64 overlaps with array_equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from recall_cases import cases, roidb_of  # noqa: E402

pytestmark = pytest.mark.gpu

_HOST = {}


def host_table(name):
    """The host path's table of a case with its match table, computed once."""
    from wssdl_bus_amd.datasets import recall
    if name not in _HOST:
        case = cases()[name]
        with np.errstate(all="ignore"):
            _HOST[name] = (recall.pack_recall_gt(roidb_of(case)),
                           recall.evaluate_recall_host(case["candidates"], roidb_of(case), case["areas"], case["limits"], return_matches=True))
    return _HOST[name]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_cells_equal(got, want, where):
    assert list(got) == list(want), where
    for k in want:
        g, w = got[k], want[k]
        assert g["num_pos"] == w["num_pos"], (where, k)
        for what in ("hits", "recalls", "thresholds", "gt_overlaps"):
            assert same(g[what], w[what]), (where, k, what)
        assert same(np.float64(g["ar"]), np.float64(w["ar"])), (where, k)
        if "matches" in w:
            for col in ("image", "gt", "box", "overlap"):               # row for row, in round order
                assert same(g["matches"][col], w["matches"][col]), (where, k, col)


@pytest.mark.parametrize("name", [n for n, c in cases().items() if not c["raises"]])
def test_device_table_equals_host_path(name):
    from wssdl_bus_amd.datasets import recall
    case = cases()[name]
    gt, want = host_table(name)
    with np.errstate(all="ignore"):
        got = recall.evaluate_recall_table(case["candidates"], gt, case["areas"], case["limits"], return_matches=True)
    assert_cells_equal(got, want, name)
    assert sum(len(c["matches"]["gt"]) for c in want.values()) > 0


def test_multi_cell_call_equals_one_cell_per_call():
    from wssdl_bus_amd.datasets import recall
    for name in ("mixed", "random200"):
        case = cases()[name]
        gt, _ = host_table(name)
        with np.errstate(all="ignore"):
            table = recall.evaluate_recall_table(case["candidates"], gt, case["areas"], case["limits"], return_matches=True)
            for area in case["areas"]:
                for limit in case["limits"]:
                    one = recall.evaluate_recall_table(case["candidates"], gt, (area,), (limit,), return_matches=True)
                    assert_cells_equal(one, {(area, limit): table[(area, limit)]}, (name, area, limit))


def test_f32_rows_with_scale_equal_the_f64_form():
    """The proposal layer's layout (rois [N, P, 5] f32, counts, scales): the op's f32 division, widened, against the
    f64 form fed f32(box) / f32(scale) computed on the host."""
    import torch
    from wssdl_bus_amd.datasets import recall
    case = cases()["random200"]
    gt, _ = host_table("random200")
    rs = np.random.RandomState(5)
    N = len(case["candidates"])
    P = max(len(c) for c in case["candidates"]) + 3
    scales = rs.uniform(0.4, 2.7, N).astype(np.float32)
    rois = rs.uniform(0, 50, (N, P, 5)).astype(np.float32)              # rows past an image's count: never read as boxes
    counts = np.array([len(c) for c in case["candidates"]], np.int32)
    lists = []
    for i, c in enumerate(case["candidates"]):
        rois[i, :len(c), 1:] = (c * np.float64(scales[i])).astype(np.float32)
        lists.append((rois[i, :len(c), 1:] / scales[i]).astype(np.float64))
        assert lists[-1].dtype == np.float64 and (rois[i, :len(c), 1:] / scales[i]).dtype == np.float32
    assert any((l != c).any() for l, c in zip(lists, case["candidates"]) if len(c))     # the division rounds
    triple = (torch.from_numpy(rois).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(scales).cuda())
    with np.errstate(all="ignore"):
        want_host = recall.evaluate_recall_host(lists, gt, case["areas"], case["limits"], return_matches=True)
        got = recall.evaluate_recall_table(triple, gt, case["areas"], case["limits"], return_matches=True)
        got64 = recall.evaluate_recall_table(lists, gt, case["areas"], case["limits"], return_matches=True)
    assert_cells_equal(got, got64, "f32 + scale against f64")
    assert_cells_equal(got, want_host, "f32 + scale against the host path")
    # without a scale the f32 rows are widened as they are
    plain = [rois[i, :n, 1:].astype(np.float64) for i, n in enumerate(counts)]
    with np.errstate(all="ignore"):
        got = recall.evaluate_recall_table((triple[0], triple[1], None), gt, ("all",), (None, 10))
        want = recall.evaluate_recall_host(plain, gt, ("all",), (None, 10))
    assert_cells_equal(got, want, "f32 without scale")


def test_fewer_boxes_than_gts_is_flagged_not_a_fault():
    import ctypes
    import torch
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.datasets import recall
    case = cases()["too_few"]
    gt = recall.pack_recall_gt(roidb_of(case))
    with pytest.raises(AssertionError, match="image 0 has 1 usable"):
        recall.evaluate_recall_table(case["candidates"], gt, case["areas"], case["limits"])
    # the op itself: two rounds, the second finds no box
    L = _lib.lib()
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    boxes, counts = t(case["candidates"][0].reshape(1, 1, 4)), t(np.array([1], np.int32))
    d_gt, d_ar = t(gt["boxes"]), t(gt["areas"])
    rng, lim, thr = t(np.array([[0.0, 1e10]])), t(np.array([0], np.int32)), t(np.array([0.5]))
    out = torch.full((3,), 7, dtype=torch.int32, device=dev)
    m_gt, m_box = torch.full((2,), 7, dtype=torch.int32, device=dev), torch.full((2,), 7, dtype=torch.int32, device=dev)
    m_ov = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    n = L.wssdl_proposal_recall_workspace_bytes(1, 1, 2)
    ws = torch.empty((n,), dtype=torch.uint8, device=dev)
    _lib.check(L.wssdl_proposal_recall(None, None, _lib.ptr(boxes), 4, _lib.ptr(counts), 1, 1, _lib.ptr(d_gt), _lib.ptr(d_ar),
                                       _lib.host_ptr(gt["offsets"]), 2, _lib.ptr(rng), 1, _lib.ptr(lim), 1, _lib.ptr(thr), 1,
                                       _lib.ptr(out[0:1]), _lib.ptr(out[1:2]), _lib.ptr(out[2:3]), _lib.ptr(m_gt), _lib.ptr(m_box),
                                       _lib.ptr(m_ov), _lib.ptr(ws), n, _lib.stream()), "wssdl_proposal_recall")
    assert out.cpu().tolist() == [1, 2, 1]                              # hits, num_pos, flag
    assert m_gt.cpu().tolist() == [0, 1] and m_box.cpu().tolist() == [0, -1] and m_ov.cpu().tolist() == [1.0, -1.0]
    # and the device goes on working
    case = cases()["tie_box"]
    got = recall.evaluate_recall_table(case["candidates"], roidb_of(case), ("all",))[("all", None)]
    assert got["gt_overlaps"].tolist() == [0.5] and got["recalls"][0] == 1.0


@pytest.fixture(scope="module")
def resnet18():
    import torch
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(3)
    net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
    net.eval()
    return net


@pytest.fixture
def small_test_scale():
    from wssdl_bus_amd.fast_rcnn.config import cfg
    old = cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.PADDED_ROIS, cfg.FUSED_RPN_SOFTMAX
    cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.PADDED_ROIS = (160,), 288, False
    yield cfg
    cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.PADDED_ROIS, cfg.FUSED_RPN_SOFTMAX = old


def _planes(shapes):
    rs = np.random.RandomState(22)
    return [rs.randint(0, 256, size=s).astype(np.uint8) for s in shapes]


@pytest.mark.parametrize("fused", [False, True])
def test_rpn_proposals_batch_equals_the_test_forward(resnet18, small_test_scale, fused):
    import torch
    from wssdl_bus_amd.fast_rcnn.detect_batch import get_test_blobs
    from wssdl_bus_amd.rpn_msr.generate import rpn_proposals_batch
    from wssdl_bus_amd.rpn_msr.proposal_layer_tf_bus import compact_rois
    cfg, net = small_test_scale, resnet18
    cfg.FUSED_RPN_SOFTMAX = fused
    data, info = get_test_blobs(_planes(((150, 210), (190, 145))), "Resnet")
    assert data.shape[0] == 2 and (info[:, 0] < data.shape[1]).any() and (info[:, 1] < data.shape[2]).any()
    with torch.no_grad():
        want = net(data, info, None, None, is_training=False, is_ws=False, test_net=True)["rpn_rois"]
    calls = []
    hook = net.head.register_forward_hook(lambda *a: calls.append(1))
    try:
        net.train()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                         # nothing is read back
        try:
            rois, counts = rpn_proposals_batch(net, data, info)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert net.training                                             # the training flag is restored
    finally:
        hook.remove()
        net.eval()
    assert calls == []                                                  # no head
    assert rois.shape == (2, cfg.TEST.RPN_POST_NMS_TOP_N, 5) and rois.dtype == torch.float32
    assert counts.shape == (2,) and counts.dtype == torch.int32 and bool((counts > 0).all())
    got = compact_rois(rois, counts)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_imdb_proposals_batch_equals_im_proposals(resnet18, small_test_scale, tmp_path):
    from PIL import Image
    from wssdl_bus_amd.datasets.bus import bus
    from wssdl_bus_amd.rpn_msr.generate import im_proposals, imdb_proposals
    planes = _planes(((150, 210), (150, 210)))
    for d in ("TIFFImages", os.path.join("ImageSets", "Main")):
        os.makedirs(str(tmp_path / d))
    for i, p in enumerate(planes):
        Image.fromarray(p).save(str(tmp_path / "TIFFImages" / ("IM%d.tif" % i)))
    (tmp_path / "ImageSets" / "Main" / "s_test.txt").write_text("IM0\nIM1\n")
    got = imdb_proposals(resnet18, bus("s_test", str(tmp_path)), batch_size=2)
    assert len(got) == 2
    for i, p in enumerate(planes):
        want = im_proposals(resnet18, p, "Resnet")
        assert want.dtype == np.float32 and want.ndim == 2 and want.shape[1] == 4 and len(want) > 0
        assert got[i].dtype == np.float32 and got[i].shape == want.shape and np.array_equal(got[i], want), i
