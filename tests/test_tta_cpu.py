"""Test-time flip augmentation and box voting without a GPU: the C-ABI surface of wssdl_post_detections_views (symbols,
workspace query, the argument validation table -- nothing is launched, every device pointer is NULL), the NumPy
statement (tests/tta_reference.py) on hand-computed cases, the host fallback of postprocess_detections_batch against
the statement bit for bit (its NMS calls answered by the oracle's cpu_nms), get_test_blobs with and without the
mirrored views, and the three cfg.TEST keys."""
import contextlib

import numpy as np
import pytest

import tta_reference as T
from oracle import np_oracle as O


@pytest.fixture(scope="module")
def L():
    from wssdl_bus_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


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


# ------------------------------------------------------------------------------------------------- C surface ---
def test_symbols_and_workspace_query(L):
    from wssdl_bus_amd import _lib
    for name in ("wssdl_post_detections_views_workspace_bytes", "wssdl_post_detections_views"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    q = L.wssdl_post_detections_views_workspace_bytes
    # one query serves both values of `agnostic`: the class-agnostic batched op's workspace where that op exists ...
    for n, v, p, k in ((1, 1, 1, 2), (8, 2, 600, 3), (3, 3, 120, 3), (2, 8, 64, 9)):
        assert q(n, v, p, k) == L.wssdl_post_detections_agnostic_batched_workspace_bytes(n, p, k)
        assert q(n, v, p, k) >= L.wssdl_post_detections_batched_workspace_bytes(n, p, k)
    # ... and the per-class one beyond the union limit
    assert q(1, 2, 7000, 3) == L.wssdl_post_detections_batched_workspace_bytes(1, 7000, 3)
    assert q(0, 2, 300, 3) > 0 and q(2, 0, 300, 3) > 0 and q(2, 2, 0, 3) > 0 and q(2, 2, 300, 1) > 0


def test_invalid_arguments_return_status_without_launch(L):
    from wssdl_bus_amd import _lib
    f = L.wssdl_post_detections_views
    INVALID = _lib.ERR_INVALID_ARGUMENT

    def call(R=10, n_images=2, views=2, P=600, K=3, thresh=0.05, agnostic=0, vote=0.0, counts=None):
        return f(None, None, None, R, n_images, views, None, P, K, thresh, 0.3, agnostic, vote, 300, None, counts, None, 0,
                 None)

    assert call(views=0) == INVALID
    assert call(views=9) == INVALID
    assert call(views=-1) == INVALID
    assert call(n_images=-1) == INVALID
    assert call(K=1) == INVALID
    assert call(K=66) == INVALID                                # K - 1 > 64
    assert call(P=0) == INVALID                                 # max_rows_per_image < 1 with R > 0
    assert call(R=-1) == INVALID
    assert call(n_images=64, P=4097, K=65) == INVALID           # n_images * (K-1) * P > 2^24
    assert call(n_images=65536, P=1, K=2) == INVALID            # more than 65535 (image, class) segments
    assert call(P=6001, K=3, agnostic=1) == INVALID             # union over WSSDL_POST_AGNOSTIC_MAX_UNION
    assert call(vote=1.0000001) == INVALID                      # vote_thresh > 1
    assert call(vote=float("nan")) == INVALID
    assert call(vote=0.5, thresh=-0.1) == INVALID               # voting needs positive weights
    assert call() == INVALID                                    # NULL pointers with R > 0
    # valid and nothing to do: no image; views and vote_thresh at their ends
    assert call(n_images=0) == 0
    assert call(n_images=0, views=8, vote=1.0) == 0
    assert call(R=0, n_images=0, P=0) == 0
    assert call(n_images=0, vote=0.0, thresh=-0.1) == 0         # no voting: any score threshold


# ------------------------------------------------------------------------------------------ the statement ---
def _dets(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 5)


def test_iou_exactly_at_the_vote_threshold():
    """[0,0,9,9] (100 pixels) inside [0,0,19,9] (200 pixels): IoU exactly 0.5.  The second votes at 0.5 and not at the
    next double above it."""
    from wssdl_bus_amd.fast_rcnn.detect_batch import vote_boxes_host
    d = _dets([0, 0, 9, 9, 0.9])
    cands = _dets([0, 0, 9, 9, 0.9], [0, 0, 19, 9, 0.6])
    assert O.bbox_overlaps(cands[:, :4].astype(np.float64), d[:, :4].astype(np.float64))[1, 0] == 0.5
    s1, s2 = float(np.float32(0.9)), float(np.float32(0.6))
    want = np.float32((s1 * 9.0 + s2 * 19.0) / (s1 + s2))
    for vote in (T.vote, vote_boxes_host):
        got = vote(d, cands, 0.5)
        assert got.dtype == np.float32 and got[0, 2] == want and 9 < got[0, 2] < 19
        assert got[0, 0] == 0 and got[0, 1] == 0 and got[0, 3] == 9 and got[0, 4] == np.float32(0.9)
        above = vote(d, cands, np.nextafter(0.5, 1.0))
        assert T.same_bits(above, d)


def test_lone_detection_is_unchanged():
    """(s * c) / s in f64 is c: the product of two f32 is exact, and so is its quotient by s"""
    from wssdl_bus_amd.fast_rcnn.detect_batch import vote_boxes_host
    rs = np.random.RandomState(1)
    for _ in range(50):
        xy = rs.uniform(0, 500, size=2)
        d = _dets(list(xy) + list(xy + rs.uniform(1, 300, size=2)) + [rs.uniform(0.06, 1)])
        far = d.copy()
        far[0, :4] += 2000
        far[0, 4] = 0.5
        cands = np.vstack((far, d))
        for vote in (T.vote, vote_boxes_host):
            assert T.same_bits(vote(d, cands, 0.5), d)
            assert T.same_bits(vote(d, d, 1.0), d)             # vote_thresh = 1: the detection alone


def test_voting_order_is_serial_in_row_order():
    """three voters whose f64 sum depends on the order: the statement adds them in ascending row order"""
    from wssdl_bus_amd.fast_rcnn.detect_batch import vote_boxes_host
    d = _dets([100, 100, 199.25, 180.5, 0.7])
    cands = _dets([101.25, 99.5, 203.75, 181.25, 0.3], [100, 100, 199.25, 180.5, 0.7], [98.5, 102.25, 197, 179.75, 0.1])
    sw, sx = 0.0, [0.0] * 4
    for c in cands:
        sw += float(c[4])
        for k in range(4):
            sx[k] += float(c[4]) * float(c[k])
    want = np.asarray([np.float32(v / sw) for v in sx])
    for vote in (T.vote, vote_boxes_host):
        got = vote(d, cands, 0.5)
        assert T.same_bits(got[0, :4], want)
        lo, hi = cands[:, :4].min(0), cands[:, :4].max(0)
        assert np.all(got[0, :4] >= lo) and np.all(got[0, :4] <= hi)


def test_unmirror_quarter_pixels_and_clamp():
    """quarter-pixel coordinates mirror exactly, twice is the identity; x2 beyond w - 1 (the decode's clip bound can
    pass it by a fraction of a pixel) gives x1' < 0, which the clamp takes to 0"""
    import torch
    from wssdl_bus_amd.fast_rcnn.detect_batch import unmirror_boxes
    w = 640.0
    own = np.asarray([[10.25, 3, 200.75, 90.5, 0, 1, 639, 2], [0, 0, 639, 10, 320.5, 7, 320.5, 9]], np.float32)
    seen = T.mirror_into_view(own, w)
    assert np.array_equal(seen[0, :4], np.asarray([438.25, 3, 628.75, 90.5], np.float32))
    assert T.same_bits(T.unmirror(seen, w), own)
    over = np.asarray([[600.5, 5, 639.75, 50, 0.25, 5, 639.25, 50]], np.float32)        # x2 = w - 1 + 0.75 and + 0.25
    want = np.asarray([[0, 5, 38.5, 50, 0, 5, 638.75, 50]], np.float32)
    assert T.same_bits(T.unmirror(over, w), want)
    # the product's torch form: source 1 of 2 is mirrored, source 0 is not, one dead row
    boxes = np.vstack((own, seen, over, over))
    rois = np.zeros((6, 5), np.float32)
    rois[:, 0] = [0, 0, 1, 1, 1, -1]
    got, image = unmirror_boxes(torch.from_numpy(boxes), torch.from_numpy(rois), 1, 2, torch.tensor([-1.0, w]))
    assert image.tolist() == [0, 0, 0, 0, 0, -1]
    assert T.same_bits(got.numpy(), np.vstack((own, own, want, over)))
    assert np.array_equal(boxes, np.vstack((own, seen, over, over)))                     # the input is not modified


# ------------------------------------------------------------------------------------- the host fallback ---
def _oracle_nms(dets, thresh):
    import torch
    d = np.ascontiguousarray(dets.detach().cpu().numpy(), dtype=np.float32)
    return torch.as_tensor(np.asarray(O.nms(d, thresh), dtype=np.int64).reshape(-1))


# (seed, rows per view and image, views, K, mirrored views, padded, kwargs of the builder, max_per_image)
FALLBACK = [
    (1, (12,), 1, 2, (), None, {}, 300),
    (2, (17, 9), 2, 3, (1,), None, dict(plant="vote"), 300),
    (3, (20, 0, 7), 2, 3, (1,), 24, dict(plant="nms", low=((2, 1),)), 6),
    (4, (15, 11), 3, 2, (1, 2), None, dict(empty=((0, 2),), cap_ties=True), 2),
]


@pytest.mark.parametrize("case", range(len(FALLBACK)))
@pytest.mark.parametrize("agnostic", (False, True))
@pytest.mark.parametrize("vote", (False, True))
def test_host_fallback_equals_the_statement(monkeypatch, case, agnostic, vote):
    import torch
    from wssdl_bus_amd.fast_rcnn import test_bus
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    seed, rows, views, K, mirrored, padded, kw, cap = FALLBACK[case]
    c = T.build_case(seed, rows, views, K, mirrored=mirrored, padded=padded, **kw)
    monkeypatch.setattr(test_bus, "hip_nms", _oracle_nms)
    keep = {k: c[k].copy() for k in ("rois", "scores", "boxes", "flip_width")}
    with _cfg_test(CLS_AGNOSTIC_NMS=agnostic, BBOX_VOTE=vote, BBOX_VOTE_THRESH=0.5):
        got = postprocess_detections_batch(torch.from_numpy(c["scores"]), torch.from_numpy(c["boxes"]),
                                           torch.from_numpy(c["rois"]), c["n_images"], K, thresh=T.THRESH, max_per_image=cap,
                                           views=views, flip_width=torch.from_numpy(c["flip_width"]))
    want = T.post_views(c["rois"], c["scores"], c["boxes"], c["n_images"], views, c["flip_width"], K, T.THRESH, cap, T.NMS,
                        agnostic, 0.5 if vote else 0.0)
    assert len(got) == c["n_images"]
    total = 0
    for t in range(c["n_images"]):
        for j in range(1, K):
            g = got[t][j].numpy()
            assert T.same_bits(T.canon(g), T.canon(want[t][j])), (t, j)
            assert np.all(g[:-1, 4] >= g[1:, 4])
            total += len(g)
    assert total > 0
    for k, v in keep.items():
        assert np.array_equal(c[k], v), k
    if vote:
        plain = T.post_views(c["rois"], c["scores"], c["boxes"], c["n_images"], views, c["flip_width"], K, T.THRESH, cap,
                             T.NMS, agnostic, 0.0)
        moved = sum(not T.same_bits(T.canon(plain[t][j]), T.canon(want[t][j])) for t in range(c["n_images"])
                    for j in range(1, K))
        assert moved > 0, "voting moved no box: the case tests nothing"


def test_defaults_take_the_path_of_before(monkeypatch):
    """views = 1, no flip_width, BBOX_VOTE off: postprocess_detections_batch never reaches the views route"""
    import torch
    from wssdl_bus_amd.fast_rcnn import detect_batch, test_bus
    c = T.build_case(7, (9, 5), 1, 3, mirrored=())
    monkeypatch.setattr(test_bus, "hip_nms", _oracle_nms)

    def boom(*a, **k):
        raise AssertionError("views route reached")
    monkeypatch.setattr(detect_batch, "_postprocess_views", boom)
    got = detect_batch.postprocess_detections_batch(torch.from_numpy(c["scores"]), torch.from_numpy(c["boxes"]),
                                                    torch.from_numpy(c["rois"]), 2, 3, thresh=T.THRESH)
    want = T.post_views(c["rois"], c["scores"], c["boxes"], 2, 1, None, 3, T.THRESH, 300, T.NMS, False, 0.0)
    for t in range(2):
        for j in (1, 2):
            assert T.same_bits(T.canon(got[t][j].numpy()), T.canon(want[t][j]))
    with _cfg_test(BBOX_VOTE=True):
        with pytest.raises(AssertionError, match="views route reached"):
            detect_batch.postprocess_detections_batch(torch.from_numpy(c["scores"]), torch.from_numpy(c["boxes"]),
                                                      torch.from_numpy(c["rois"]), 2, 3, thresh=T.THRESH)


# ------------------------------------------------------------------------------------------------- blobs, cfg ---
def test_get_test_blobs_with_and_without_flip(monkeypatch):
    """flip_aug=False: today's pair from today's calls (no `flipped` keyword reaches prep_im_for_blob); flip_aug=True:
    image 2i plain, image 2i+1 through prep_im_for_blob(..., flipped=True, is_training=False), im_info [2n,3] and
    flip_width [2n] = -1 / the plane's width"""
    import torch
    from wssdl_bus_amd.fast_rcnn import detect_batch
    from wssdl_bus_amd.utils import blob
    calls = []

    def fake_prep(g, net_name, means, stds, target, max_size, **kw):
        calls.append(dict(kw, shape=g.shape))
        return torch.zeros((g.shape[0] * 2, g.shape[1] * 2, 3)), 2.0

    def fake_list(ims):
        return torch.zeros((len(ims), max(i.shape[0] for i in ims), max(i.shape[1] for i in ims), 3))
    monkeypatch.setattr(blob, "prep_im_for_blob", fake_prep)
    monkeypatch.setattr(blob, "im_list_to_blob", fake_list)
    planes = [np.zeros((30, 40), np.uint8), np.zeros((25, 64), np.uint8)]
    out = detect_batch.get_test_blobs(planes, "Resnet", flip_aug=False)
    assert len(out) == 2 and tuple(out[0].shape) == (2, 60, 128, 3)
    assert out[1].tolist() == [[60, 80, 2], [50, 128, 2]]
    assert calls == [dict(is_training=False, shape=(30, 40)), dict(is_training=False, shape=(25, 64))]
    assert len(detect_batch.get_test_blobs(planes, "Resnet")) == 2                      # the default reads cfg: off
    del calls[:]
    with _cfg_test(FLIP_AUG=True):
        data, info, fw = detect_batch.get_test_blobs(planes, "Resnet")
    assert tuple(data.shape) == (4, 60, 128, 3)
    assert info.tolist() == [[60, 80, 2], [60, 80, 2], [50, 128, 2], [50, 128, 2]]
    assert fw.dtype == torch.float32 and fw.tolist() == [-1, 40, -1, 64]
    assert calls == [dict(is_training=False, shape=(30, 40)), dict(is_training=False, flipped=True, shape=(30, 40)),
                     dict(is_training=False, shape=(25, 64)), dict(is_training=False, flipped=True, shape=(25, 64))]


def test_config_keys_and_cfg_from_list():
    from wssdl_bus_amd.fast_rcnn.config import cfg, cfg_from_list
    assert cfg.TEST.FLIP_AUG is False and cfg.TEST.BBOX_VOTE is False and cfg.TEST.BBOX_VOTE_THRESH == 0.5
    with _cfg_test(FLIP_AUG=False, BBOX_VOTE=False, BBOX_VOTE_THRESH=0.5):
        cfg_from_list(["TEST.FLIP_AUG", "True", "TEST.BBOX_VOTE", "True", "TEST.BBOX_VOTE_THRESH", "0.65"])
        assert cfg.TEST.FLIP_AUG is True and cfg.TEST.BBOX_VOTE is True and cfg.TEST.BBOX_VOTE_THRESH == 0.65
    assert cfg.TEST.FLIP_AUG is False and cfg.TEST.BBOX_VOTE is False and cfg.TEST.BBOX_VOTE_THRESH == 0.5
