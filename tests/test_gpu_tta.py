"""Test-time flip augmentation and box voting on the device: wssdl_post_detections_views against the NumPy statement
(tests/tta_reference.py) bit for bit, against the single-image call image by image, against the batched ops of before
(views = 1; and a host-rewritten blob, an independent route), the mirrored-copy identity, the voters' bounds, the
overflow flag, the memory and stream-order contracts, get_test_blobs' mirrored half, and detect_images /
evaluate_images end to end under cfg.TEST.FLIP_AUG + BBOX_VOTE."""
import contextlib
import functools

import numpy as np
import pytest

import guarded_alloc
import stream_order
import tta_reference as T
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

VOTE = 0.5


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


# (seed, rows per view of every image, views, K, mirrored views, padded, builder keywords, max_per_image)
GRID = [
    (11, (12,), 1, 2, (), None, {}, 300),
    (12, (17, 40), 2, 3, (1,), None, dict(plant="vote"), 300),
    (13, (20, 0, 7), 2, 3, (1,), 40, dict(plant="nms", low=((2, 1),)), 6),          # dead rows between the views
    (14, (15, 11), 3, 2, (1, 2), None, dict(empty=((0, 2),), cap_ties=True), 2),
    (15, (33, 1, 40), 3, 3, (1,), 40, dict(empty=((1, 0),), low=((0, 2),)), 5),
    (16, (40, 23), 2, 2, (0, 1), None, dict(plant="vote", cap_ties=True), 3),       # both views mirrored
    (17, (300,) * 8, 2, 3, (1,), 300, {}, 300),                                     # the working size
]


@functools.lru_cache(maxsize=None)
def _case(i):
    seed, rows, views, K, mirrored, padded, kw, cap = GRID[i]
    c = T.build_case(seed, rows, views, K, mirrored=mirrored, padded=padded, **kw)
    c["cap"] = cap
    c["pitch"] = T.pitch_of(c)
    for k in ("rois", "scores", "boxes", "flip_width"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want(i, agnostic, vote):
    c = _case(i)
    return T.post_views(c["rois"], c["scores"], c["boxes"], c["n_images"], c["views"], c["flip_width"], c["K"], T.THRESH,
                        c["cap"], T.NMS, agnostic, VOTE if vote else 0.0, pitch=c["pitch"])


def _run(torch, c, agnostic, vote, pitch=None, rois=None, scores=None, boxes=None, flip_width="case", n_images=None,
         views=None):
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_views_device
    fw = c["flip_width"] if isinstance(flip_width, str) else flip_width
    ins = [_t(torch, c["scores"] if scores is None else scores), _t(torch, c["boxes"] if boxes is None else boxes),
           _t(torch, c["rois"] if rois is None else rois), None if fw is None else _t(torch, fw)]
    keep = [None if x is None else x.clone() for x in ins]
    dets, counts = post_detections_views_device(ins[0], ins[1], ins[2], c["n_images"] if n_images is None else n_images,
                                                c["views"] if views is None else views, ins[3], c["K"], thresh=T.THRESH,
                                                max_per_image=c["cap"], max_rows_per_image=pitch or c["pitch"],
                                                agnostic=agnostic, vote_thresh=VOTE if vote else 0.0)
    for a, b in zip(ins, keep):
        assert a is None or torch.equal(a, b), "the op wrote to an input"
    return dets.cpu().numpy(), counts.cpu().numpy()


def _rows_of(dets, counts, t, j):
    return dets[t, j - 1, :max(counts[t, j - 1], 0)]


@pytest.mark.parametrize("vote", (False, True))
@pytest.mark.parametrize("agnostic", (False, True))
@pytest.mark.parametrize("case", range(len(GRID)))
def test_op_equals_the_statement(torch_cuda, case, agnostic, vote):
    """1. the op == the statement bit for bit, every image, every class; the single-image call == the batched call;
    5. every voted coordinate within its voters' coordinates; 7. inputs untouched (in _run), a second run the same"""
    torch = torch_cuda
    c = _case(case)
    N, V, K = c["n_images"], c["views"], c["K"]
    want = _want(case, agnostic, vote)
    dets, counts = _run(torch, c, agnostic, vote)
    assert dets.shape == (N, K - 1, c["pitch"], 5) and counts.shape == (N, K - 1) and (counts >= 0).all()
    differing = 0
    for t in range(N):
        for j in range(1, K):
            got = _rows_of(dets, counts, t, j)
            assert len(got) == len(want[t][j]), (case, t, j)
            a, b = T.canon(got), T.canon(want[t][j])
            differing += int((a.view(np.uint32) != b.view(np.uint32)).sum())
            assert np.all(got[:-1, 4] >= got[1:, 4])
    print("tta case %d agnostic=%d vote=%d: %d detections, %d differing bits" % (case, agnostic, vote, counts.sum(), differing))
    assert differing == 0
    assert counts.sum() > 0
    # a second run: the same bits
    d2, c2 = _run(torch, c, agnostic, vote)
    assert np.array_equal(counts, c2)
    for t in range(N):
        for j in range(1, K):
            assert T.same_bits(_rows_of(dets, counts, t, j), _rows_of(d2, c2, t, j))
    # the single-image call on an image's rows alone (all of them for the small cases, two at the working size)
    col = c["rois"][:, 0]
    for t in (range(N) if N <= 3 else (0, N - 1)):
        rows = np.where((col >= t * V) & (col < (t + 1) * V))[0]
        if len(rows) == 0:
            assert not counts[t].any()
            continue
        sl = slice(rows[0], rows[-1] + 1)                       # with the dead rows between its views
        r1 = np.array(c["rois"][sl])
        r1[r1[:, 0] >= 0, 0] -= t * V
        d1, c1 = _run(torch, c, agnostic, vote, rois=r1, scores=c["scores"][sl], boxes=c["boxes"][sl],
                      flip_width=c["flip_width"][t * V:(t + 1) * V], n_images=1)
        assert np.array_equal(c1[0], counts[t]), (case, t)
        for j in range(1, K):
            assert T.same_bits(_rows_of(d1, c1, 0, j), _rows_of(dets, counts, t, j)), (case, t, j)
    if vote:
        plain, pc = _run(torch, c, agnostic, False)
        assert np.array_equal(pc, counts)
        moved = 0
        for t in range(N):
            s, b, _ = T.image_rows(c["rois"], c["scores"], c["boxes"], t, V, N, c["flip_width"])
            for j in range(1, K):
                got, was = _rows_of(dets, counts, t, j), _rows_of(plain, pc, t, j)
                assert T.same_bits(got[:, 4], was[:, 4])                        # scores and order unchanged
                if len(got) == 0:
                    continue
                cand = b[s[:, j] > T.THRESH, 4 * j:4 * j + 4]
                ov = O.bbox_overlaps(np.ascontiguousarray(cand, dtype=np.float64),
                                     np.ascontiguousarray(was[:, :4], dtype=np.float64))
                for i in range(len(got)):
                    voters = cand[ov[:, i] >= VOTE]
                    assert len(voters) >= 1
                    assert np.all(got[i, :4] >= voters.min(0)) and np.all(got[i, :4] <= voters.max(0)), (case, t, j, i)
                    moved += int(not T.same_bits(got[i], was[i]))
        assert moved > 0 or case == 0 or counts.sum() < 3


def test_cap_ties_and_planted_pairs_are_live(torch_cuda):
    """the grid's special rows do what they are there for: the four tied rows all pass a cap of two or three; the
    pair planted at IoU = nms_thresh loses its second box; the one planted at IoU = vote_thresh moves the first box"""
    for case in (3, 5):
        c = _case(case)
        w = _want(case, False, False)[0]
        assert sum(len(w[j]) for j in range(1, c["K"])) > c["cap"]
        assert (w[1][:, 4] == np.float32(0.9975)).sum() == 4
    w = _want(2, False, False)[0][1]
    assert (w[:, 4] == np.float32(0.989)).sum() == 1 and (w[:, 4] == np.float32(0.979)).sum() == 0
    c = _case(1)
    plain, voted = _want(1, False, False)[0][1], _want(1, False, True)[0][1]
    assert np.array_equal(plain[0, :4], [500, 800, 509, 809]) and 509 < voted[0, 2] < 519 and voted[0, 0] == 500


@pytest.mark.parametrize("agnostic", (False, True))
def test_one_view_is_the_batched_op(torch_cuda, agnostic):
    """2. views = 1, no flip, voting off == wssdl_post_detections_batched / _agnostic_batched, bit for bit, order
    included (no canonical sort here: the same launches ran)"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device
    c = dict(T.build_case(21, (30, 0, 17, 40), 1, 3, mirrored=(), padded=40, cap_ties=True), cap=7)
    c["pitch"] = 40
    for fw in (None, c["flip_width"]):                          # a NULL array and one of -1 entries
        dets, counts = _run(torch, c, agnostic, False, flip_width=fw)
        bd, bc = post_detections_batched_device(_t(torch, c["scores"]), _t(torch, c["boxes"]), _t(torch, c["rois"]), 4, 3,
                                                thresh=T.THRESH, max_per_image=7, max_rows_per_image=40, agnostic=agnostic)
        bd, bc = bd.cpu().numpy(), bc.cpu().numpy()
        assert np.array_equal(counts, bc) and counts.sum() > 7
        for t in range(4):
            for j in (1, 2):
                assert T.same_bits(_rows_of(dets, counts, t, j), _rows_of(bd, bc, t, j)), (t, j)


@pytest.mark.parametrize("case", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("agnostic", (False, True))
def test_voting_off_equals_the_batched_op_on_a_rewritten_blob(torch_cuda, case, agnostic):
    """3. an independent route: the batch column rewritten to the output image and the mirrored rows un-mirrored on the
    host in f32, then the batched op of before"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device
    c = _case(case)
    N, V, K = c["n_images"], c["views"], c["K"]
    rois, boxes = np.array(c["rois"]), np.array(c["boxes"])
    live = rois[:, 0] >= 0
    src = rois[:, 0].astype(np.int64)
    for s in range(N * V):
        if c["flip_width"][s] >= 0:
            m = live & (src == s)
            boxes[m] = T.unmirror(boxes[m], c["flip_width"][s])
    rois[live, 0] = src[live] // V
    bd, bc = post_detections_batched_device(_t(torch, c["scores"]), _t(torch, boxes), _t(torch, rois), N, K, thresh=T.THRESH,
                                            max_per_image=c["cap"], max_rows_per_image=c["pitch"], agnostic=agnostic)
    bd, bc = bd.cpu().numpy(), bc.cpu().numpy()
    dets, counts = _run(torch, c, agnostic, False)
    assert np.array_equal(counts, bc)
    for t in range(N):
        for j in range(1, K):
            assert T.same_bits(_rows_of(dets, counts, t, j), _rows_of(bd, bc, t, j)), (t, j)


def test_mirrored_copy_of_a_view_changes_nothing(torch_cuda):
    """4. view 1 = view 0 mirrored, on quarter-pixel coordinates, voting off: every copy ties with its original at
    IoU 1 and one of the two goes, so boxes and scores are those of view 0 alone.  A flip off by one pixel shows here."""
    torch = torch_cuda
    one = dict(T.build_case(31, (25, 40), 1, 3, mirrored=()), cap=10)
    one["pitch"] = 40
    R, S, B, fw = [], [], [], []
    for t in range(2):
        m = one["rois"][:, 0] == t
        for v in range(2):
            r = np.array(one["rois"][m])
            r[:, 0] = 2 * t + v
            R.append(r)
            S.append(one["scores"][m])
            B.append(T.mirror_into_view(one["boxes"][m], 1000.0) if v else one["boxes"][m])
            fw.append(1000.0 if v else -1.0)
    two = dict(one, rois=np.concatenate(R), scores=np.concatenate(S), boxes=np.concatenate(B),
               flip_width=np.asarray(fw, np.float32), views=2, pitch=80)
    for agnostic in (False, True):
        d1, c1 = _run(torch, one, agnostic, False)
        d2, c2 = _run(torch, two, agnostic, False)
        assert np.array_equal(c1, c2) and c1.sum() > 10
        for t in range(2):
            for j in (1, 2):
                assert T.same_bits(_rows_of(d1, c1, t, j), _rows_of(d2, c2, t, j)), (agnostic, t, j)
        # and a width off by one pixel does show
        d3, c3 = _run(torch, two, agnostic, False, flip_width=np.asarray([-1, 1001, -1, 1001], np.float32))
        assert not all(T.same_bits(_rows_of(d1, c1, t, j), _rows_of(d3, c3, t, j)) for t in range(2) for j in (1, 2))


def test_overflow_flag_and_raise(torch_cuda):
    """6. an output image whose views span more rows than the pitch: counts[t, 0] = -1, zeros in its other counts, the
    other images as before; postprocess_detections_batch raises"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    c = dict(T.build_case(41, (10, 22, 8), 2, 3), cap=300)
    c["pitch"] = 44
    for vote in (False, True):
        full, fc = _run(torch, c, False, vote)
        dets, counts = _run(torch, c, False, vote, pitch=40)
        assert counts[1].tolist() == [-1, 0]
        for t in (0, 2):
            assert np.array_equal(counts[t], fc[t]) and fc[t].sum() > 0
            for j in (1, 2):
                assert T.same_bits(_rows_of(dets, counts, t, j), _rows_of(full, fc, t, j))
    with _cfg_test(RPN_POST_NMS_TOP_N=20, BBOX_VOTE=True):
        with pytest.raises(ValueError, match="more RoI rows"):
            postprocess_detections_batch(_t(torch, c["scores"]), _t(torch, c["boxes"]), _t(torch, c["rois"]), 3, 3, views=2,
                                         flip_width=_t(torch, c["flip_width"]))
    with _cfg_test(RPN_POST_NMS_TOP_N=22, BBOX_VOTE=True):
        got = postprocess_detections_batch(_t(torch, c["scores"]), _t(torch, c["boxes"]), _t(torch, c["rois"]), 3, 3,
                                           thresh=T.THRESH, views=2, flip_width=_t(torch, c["flip_width"]))
    want = T.post_views(c["rois"], c["scores"], c["boxes"], 3, 2, c["flip_width"], 3, T.THRESH, 300, T.NMS, False, VOTE)
    for t in range(3):
        for j in (1, 2):
            assert T.same_bits(T.canon(got[t][j].cpu().numpy()), T.canon(want[t][j]))


def test_fallback_on_gpu_tensors_equals_the_op(torch_cuda):
    """FUSED_POST_DETECTIONS off: the step-by-step route (hip_nms per class, host voting) gives the op's bits"""
    torch = torch_cuda
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    c = _case(2)
    for agnostic in (False, True):
        dets, counts = _run(torch, c, agnostic, True)
        with _cfg_test(FUSED_POST_DETECTIONS=False, CLS_AGNOSTIC_NMS=agnostic, BBOX_VOTE=True, BBOX_VOTE_THRESH=VOTE):
            got = postprocess_detections_batch(_t(torch, c["scores"]), _t(torch, c["boxes"]), _t(torch, c["rois"]),
                                               c["n_images"], c["K"], thresh=T.THRESH, max_per_image=c["cap"], views=c["views"],
                                               flip_width=_t(torch, c["flip_width"]))
        for t in range(c["n_images"]):
            for j in range(1, c["K"]):
                assert T.same_bits(got[t][j].cpu().numpy(), _rows_of(dets, counts, t, j)), (agnostic, t, j)


# ------------------------------------------------------------------------------------------------ contracts ---
def _dets_up_to_counts(result):
    """the defined region: "Rows of dets at and beyond a class's count are not written: they keep what the caller's
    buffer held." (include/wssdl_bus_hip.h)"""
    dets, counts = result
    n = counts.clamp_min(0).cpu().tolist()
    return [[dets[t, c, :n[t][c]] for c in range(dets.shape[1])] for t in range(dets.shape[0])], counts


CONTRACT = [(1, False, True), (2, True, True), (3, False, False), (4, True, True), (6, False, True)]


def _contract_case(torch, i):
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_views_device
    case, agnostic, vote = CONTRACT[i]
    c = _case(case)
    inputs = {k: _t(torch, c[k]) for k in ("scores", "boxes", "rois", "flip_width")}

    def fn(inp):
        return post_detections_views_device(inp["scores"], inp["boxes"], inp["rois"], c["n_images"], c["views"],
                                            inp["flip_width"], c["K"], thresh=T.THRESH, max_per_image=c["cap"],
                                            max_rows_per_image=c["pitch"], agnostic=agnostic, vote_thresh=VOTE if vote else 0.0)
    return fn, inputs


@pytest.mark.parametrize("i", range(len(CONTRACT)))
def test_memory_contract(torch_cuda, i):
    fn, inputs = _contract_case(torch_cuda, i)
    guarded_alloc.run_case(fn, inputs, name="post-views-%d" % i, min_allocations=3, defined=_dets_up_to_counts)


@pytest.mark.parametrize("i", range(len(CONTRACT)))
def test_stream_order_contract(torch_cuda, i):
    fn, inputs = _contract_case(torch_cuda, i)
    stream_order.run_case(fn, inputs, name="post-views-%d" % i, defined=_dets_up_to_counts)
    stream_order.assert_sync_free(fn, inputs, name="post-views-%d" % i)


def test_op_is_capturable(torch_cuda):
    """no read-back, no allocation inside the op: it records into a graph and replays with the eager bits"""
    torch = torch_cuda
    from wssdl_bus_amd import _lib
    c = _case(1)
    N, V, K, P = c["n_images"], c["views"], c["K"], c["pitch"]
    eager, ec = _run(torch, c, True, True)
    L = _lib.lib()
    s, b, r, fw = (_t(torch, c[k]) for k in ("scores", "boxes", "rois", "flip_width"))
    dets = torch.zeros((N, K - 1, P, 5), dtype=torch.float32, device="cuda")
    counts = torch.zeros((N, K - 1), dtype=torch.int32, device="cuda")
    n = L.wssdl_post_detections_views_workspace_bytes(N, V, P, K)
    ws = torch.empty((n,), dtype=torch.uint8, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        _lib.check(L.wssdl_post_detections_views(_lib.ptr(r), _lib.ptr(s), _lib.ptr(b), r.shape[0], N, V, _lib.ptr(fw), P, K,
                                                 T.THRESH, T.NMS, 1, VOTE, c["cap"], _lib.ptr(dets), _lib.ptr(counts),
                                                 _lib.ptr(ws), n, _lib.stream()), "wssdl_post_detections_views")
    for _ in range(2):
        counts.zero_()
        g.replay()
    torch.cuda.synchronize()
    gc, gd = counts.cpu().numpy(), dets.cpu().numpy()
    assert np.array_equal(gc, ec)
    for t in range(N):
        for j in range(1, K):
            assert T.same_bits(_rows_of(gd, gc, t, j), _rows_of(eager, ec, t, j))


# ----------------------------------------------------------------------------------------------- end to end ---
def _planes():
    rs = np.random.RandomState(22)
    return [rs.randint(0, 256, size=shape).astype(np.uint8) for shape in ((300, 420), (380, 290), (260, 520))]


def test_mirrored_half_of_the_blob(torch_cuda):
    """8. image 2i+1 of get_test_blobs(flip_aug=True) == the blob of the column-reversed plane, image 2i == the plain one"""
    from wssdl_bus_amd.fast_rcnn.detect_batch import get_test_blobs
    planes = _planes()
    data, info, fw = get_test_blobs(planes, "Resnet", flip_aug=True)
    plain, pinfo = get_test_blobs(planes, "Resnet", flip_aug=False)
    rev, rinfo = get_test_blobs([np.ascontiguousarray(p[:, ::-1]) for p in planes], "Resnet")
    assert data.shape[0] == 6 and tuple(data.shape[1:]) == tuple(plain.shape[1:]) == tuple(rev.shape[1:])
    assert fw.cpu().tolist() == [-1, 420, -1, 290, -1, 520]
    for i in range(3):
        assert T.same_bits(data[2 * i].cpu().numpy(), plain[i].cpu().numpy()), i
        assert T.same_bits(data[2 * i + 1].cpu().numpy(), rev[i].cpu().numpy()), i
        assert not T.same_bits(data[2 * i + 1].cpu().numpy(), plain[i].cpu().numpy())
        assert info[2 * i].tolist() == info[2 * i + 1].tolist() == pinfo[i].tolist() == rinfo[i].tolist()


@pytest.fixture(scope="module")
def resnet18(torch_cuda):
    torch = torch_cuda
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(3)
    net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
    net.eval()
    # The class layer is drawn at std 0.01 and the box layer at 0.001: every score is 1/3 up to 1e-5 and equal scores on
    # overlapping boxes abound, which leaves the statement's NMS order to argsort.  One forward measures the spread of
    # the class logits around their column means and of the box deltas; the class layer is rescaled to a spread of 1
    # (its bias takes the column means out, so no class saturates the softmax) and the box layer to 0.2: still random
    # weights, with scores all over (0, 1) and boxes that move.
    from wssdl_bus_amd.fast_rcnn.detect_batch import get_test_blobs, im_detect_batch
    data, info = get_test_blobs(_planes()[:1], "Resnet", flip_aug=False)
    im_detect_batch(net, data, info)
    with torch.no_grad():
        logits = net.layers['cls_score'].float()
        k = 1.0 / float((logits - logits.mean(0)).std())
        net.cls_score.weight.mul_(k)
        net.cls_score.bias.copy_(-k * logits.mean(0))
        net.bbox_pred.weight.mul_(0.2 / float(net.layers['bbox_pred'].std()))
    return net


def _raise_hip_nms(*a, **k):
    raise RuntimeError("step-by-step form reached")


@pytest.mark.parametrize("padded", (False, True))
def test_detect_and_evaluate_images_end_to_end(torch_cuda, resnet18, monkeypatch, padded):
    """9. detect_images under FLIP_AUG + BBOX_VOTE == the statement applied to im_detect_batch's own outputs (one
    forward, its outputs handed to both), in original-image coordinates; evaluate_images scores those detections, on
    the device op (a hip_nms call would raise)"""
    torch = torch_cuda
    import post_agnostic_reference as PA
    from wssdl_bus_amd.datasets.voc_eval_bus import evaluate_detections
    from wssdl_bus_amd.fast_rcnn import detect_batch, eval_batch, test_bus
    from wssdl_bus_amd.fast_rcnn.config import cfg
    planes = _planes()
    seen = []
    real = detect_batch.im_detect_batch

    def once(net, data, info):
        if not seen:
            seen.append(real(net, data, info))
        assert data.shape[0] == 6 and info.shape == (6, 3)         # batch_size counts original images
        return seen[0]
    monkeypatch.setattr(detect_batch, "im_detect_batch", once)
    monkeypatch.setattr(eval_batch, "im_detect_batch", once)
    monkeypatch.setattr(test_bus, "hip_nms", _raise_hip_nms)
    old = cfg.PADDED_ROIS
    try:
        cfg.PADDED_ROIS = padded
        with _cfg_test(FLIP_AUG=True, BBOX_VOTE=True, BBOX_VOTE_THRESH=VOTE, RPN_PRE_NMS_TOP_N=250):
            all_boxes = detect_batch.detect_images(resnet18, planes, "Resnet", batch_size=3, max_per_image=40)
            scores, boxes, rois = (x.cpu().numpy() for x in seen[0])
            K = scores.shape[1]
            fw = np.asarray([-1, 420, -1, 290, -1, 520], np.float32)
            assert bool((rois[:, 0] < 0).any()) == padded
            want = T.post_views(rois, scores, boxes, 3, 2, fw, K, 0.05, 40, cfg.TEST.NMS, False, VOTE)
            plain = T.post_views(rois, scores, boxes, 3, 2, fw, K, 0.05, 40, cfg.TEST.NMS, False, 0.0)
            n_det = moved = 0
            for t in range(3):
                s, b, _ = T.image_rows(rois, scores, boxes, t, 2, 3, fw)
                assert PA.ties_are_harmless(s, b, K, 0.05, cfg.TEST.NMS)
                assert len(np.unique(rois[(rois[:, 0] >= 2 * t) & (rois[:, 0] < 2 * t + 2), 0])) == 2     # both views have rows
                for j in range(1, K):
                    assert T.same_bits(T.canon(all_boxes[j][t]), T.canon(want[t][j])), (t, j)
                    n_det += len(want[t][j])
                    moved += int(not T.same_bits(T.canon(want[t][j]), T.canon(plain[t][j])))
                    a = all_boxes[j][t]
                    assert np.all(a[:, 0] >= 0) and np.all(a[:, 2] <= planes[t].shape[1])
            assert n_det > 0 and moved > 0
            # ground truth: two of every image's own detections
            gt_roidb = []
            for t in range(3):
                gtb = np.vstack([all_boxes[j][t][:1, :4] for j in range(1, K) if len(all_boxes[j][t])][:2])
                cls = np.asarray([j for j in range(1, K) if len(all_boxes[j][t])][:2])
                gt_roidb.append(dict(boxes=np.rint(gtb).astype(np.int64) + 1, gt_classes=cls,
                                     difficult=np.zeros(len(cls), np.int64)))
            classes = ["__background__"] + ["class_%d" % j for j in range(1, K)]
            want_eval = evaluate_detections(all_boxes, gt_roidb, classes)
            got_eval = eval_batch.evaluate_images(resnet18, planes, gt_roidb, "Resnet", batch_size=3, classes=classes,
                                                  max_per_image=40)
    finally:
        cfg.PADDED_ROIS = old
    for k in ("aps", "mean_ap", "corloc_list", "froc_curve_pts"):
        assert got_eval[k] == want_eval[k], k
    assert np.array_equal(got_eval["num_fp_per_img"], want_eval["num_fp_per_img"])
    assert got_eval["result"]["class_offsets"][-1] == n_det
