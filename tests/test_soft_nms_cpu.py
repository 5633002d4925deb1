"""Soft-NMS without a GPU: the NumPy statement (tests/soft_nms_reference.py) on hand-computed cases, its method 0
against the hard statement, the order and tie-break properties, the package's host path (soft_nms_host,
postprocess_soft_host, postprocess_detections_batch on CPU tensors) against the statement bit for bit, the cfg keys
and their errors, and the C surface of wssdl_post_detections_soft (symbols, workspace query, the argument validation
table -- nothing is launched, every device pointer is NULL)."""
import contextlib
import functools
import math

import numpy as np
import pytest

import post_agnostic_reference as PA
import soft_nms_reference as S
import tta_reference as T

F32 = np.float32


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


@functools.lru_cache(maxsize=None)
def _builder_case(seed):
    return S.build_case(seed, [60, 37], 2, 3)


def _host(dets, method, nt, sigma, floor):
    from wssdl_bus_amd.fast_rcnn.soft_nms import soft_nms_host
    return soft_nms_host(dets, method, nt, sigma, floor)


def _statement(dets, method, nt, sigma, floor):
    return S.soft_class(dets, method, nt, sigma, floor)


# ------------------------------------------------------------------------------------------ the statement ---
@pytest.mark.parametrize("fn", (_statement, _host))
def test_hand_computed_linear(fn):
    """A (0.9) first; B at IoU 0.5 takes the weight 0.5, C at 2/13 none; then C (0.7), whose IoU 0.25 with B is below
    0.3: B stays at 0.4.  At Nt = 0.2 that second pick costs B the weight 0.75."""
    d = S.hand_case()
    got = fn(d, S.LINEAR, 0.3, 0.5, 0.001)
    b = F32(0.8) * F32(0.5)
    assert T.same_bits(got, np.vstack((d[0], d[2], np.append(d[1, :4], b))))
    got = fn(d, S.LINEAR, 0.2, 0.5, 0.001)
    assert T.same_bits(got, np.vstack((d[0], d[2], np.append(d[1, :4], b * F32(0.75)))))
    # a floor above 0.4 * 0.75: B leaves in the middle of the loop, after C's pick
    got = fn(d, S.LINEAR, 0.2, 0.5, 0.35)
    assert T.same_bits(got, np.vstack((d[0], d[2])))


@pytest.mark.parametrize("fn", (_statement, _host))
def test_hand_computed_gaussian(fn):
    """sigma 0.5: after A, B = 0.8 * exp(-0.25 / 0.5) and C = 0.7 * exp(-(2/13)^2 / 0.5); C leads and costs B
    exp(-0.0625 / 0.5) more.  Every weight is one f64 exp rounded once to f32, every product one f32 product."""
    d = S.hand_case()
    got = fn(d, S.GAUSSIAN, 0.3, 0.5, 0.001)
    ov_ac = float(F32(20) / F32(130))
    c = F32(0.7) * F32(math.exp(-(ov_ac * ov_ac) / 0.5))
    b = F32(0.8) * F32(math.exp(-0.25 / 0.5))
    b = b * F32(math.exp(-0.0625 / 0.5))
    assert c > b
    assert T.same_bits(got, np.vstack((d[0], np.append(d[2, :4], c), np.append(d[1, :4], b))))
    assert abs(float(c) - 0.7 * math.exp(-(2 / 13) ** 2 / 0.5)) < 1e-6 and abs(float(b) - 0.8 * math.exp(-0.625)) < 1e-6


@pytest.mark.parametrize("fn", (_statement, _host))
def test_pair_exactly_at_the_threshold(fn):
    """IoU 36 / 120: f32(0.3) as a double is >= 0.3, so the pair decays under linear and goes under hard (the >= side)"""
    d = S.hand_case_at_threshold()
    assert float(F32(36) / F32(120)) >= 0.3
    got = fn(d, S.LINEAR, 0.3, 0.5, 0.001)
    assert T.same_bits(got, np.vstack((d[0], np.append(d[1, :4], F32(0.8) * (F32(1) - F32(0.3))))))
    assert got[1, 4] < F32(0.8)
    assert T.same_bits(fn(d, S.HARD, 0.3, 0.5, 0.001), d[:1])
    assert T.same_bits(fn(d, S.LINEAR, float(np.nextafter(float(F32(0.3)), 1.0)), 0.5, 0.001), d)


@pytest.mark.parametrize("seed", range(3))
def test_method_0_is_the_hard_statement(seed):
    c = _builder_case(seed)
    ties = []
    got = S.post_soft(c["rois"], c["scores"], c["boxes"], 2, 2, c["flip_width"], 3, S.THRESH, 20, S.HARD, ties=ties)
    segments = 0
    for t in range(2):
        s, b, _ = T.image_rows(c["rois"], c["scores"], c["boxes"], t, 2, 2, c["flip_width"])
        want = PA.cap(PA.per_class(s, b, 3, S.THRESH, S.NMS), 3, 20)
        for j in (1, 2):
            assert T.same_bits(got[t][j], want[j]), (t, j)
            segments += len(want[j]) > 0
    assert segments == 4 and not ties
    assert c["exp_calls"] > 1000


@pytest.mark.parametrize("method", (S.LINEAR, S.GAUSSIAN))
@pytest.mark.parametrize("seed", range(3))
def test_emitted_scores_never_increase(seed, method):
    c = _builder_case(seed)
    got = S.post_soft(c["rois"], c["scores"], c["boxes"], 2, 2, c["flip_width"], 3, S.THRESH, 0, method)
    hard = S.post_soft(c["rois"], c["scores"], c["boxes"], 2, 2, c["flip_width"], 3, S.THRESH, 0, S.HARD)
    for t in range(2):
        for j in (1, 2):
            g = got[t][j]
            assert np.all(g[:-1, 4] >= g[1:, 4]) and np.all(g[:, 4] > F32(S.FLOOR))
            assert len(g) > len(hard[t][j]) > 0, "Soft-NMS keeps what hard NMS deletes"


@pytest.mark.parametrize("method", (S.LINEAR, S.GAUSSIAN))
def test_planted_decayed_tie_goes_later_row_first(method):
    c = S.build_case(9, [12], 1, 2, mirrored=(), tie=True)
    ties = []
    got = S.post_soft(c["rois"], c["scores"], c["boxes"], 1, 1, c["flip_width"], 2, S.THRESH, 0, method, ties=ties)[0][1]
    assert ties, "the two decayed scores are equal"
    i = int(np.where(got[:, 0] == 275)[0][0])
    assert got[i + 1, 0] == 325 and got[i, 4] == got[i + 1, 4] < F32(0.9)       # row 2 (x1 = 275) before row 1 (x1 = 325)
    s, b, _ = T.image_rows(c["rois"], c["scores"], c["boxes"], 0, 1, 1, c["flip_width"])
    inds = np.where(s[:, 1] > F32(S.THRESH))[0]
    host = _host(np.hstack((b[inds, 4:8], s[inds, 1:2])), method, S.NMS, S.SIGMA, S.FLOOR)
    assert T.same_bits(host, got)


# ------------------------------------------------------------------------------------------- the host path ---
# (seed, rows per view and image, views, K, mirrored views, padded, kwargs of the builder, max_per_image)
HOST = [
    (1, (12,), 1, 2, (), None, {}, 300),
    (2, (17, 9), 2, 3, (1,), None, dict(tie=True), 300),
    (3, (20, 0, 7), 2, 3, (1,), 24, dict(plant="nms", low=((2, 1),)), 6),
    (4, (15, 11), 3, 2, (1, 2), None, dict(empty=((0, 2),), cap_ties=True), 2),
]


@pytest.mark.parametrize("case", range(len(HOST)))
@pytest.mark.parametrize("name", ("linear", "gaussian"))
def test_host_path_equals_the_statement(case, name):
    import torch
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    from wssdl_bus_amd.fast_rcnn.post_detections import postprocess_detections
    seed, rows, views, K, mirrored, padded, kw, cap = HOST[case]
    c = S.build_case(seed, rows, views, K, mirrored=mirrored, padded=padded, **kw)
    method = dict(linear=S.LINEAR, gaussian=S.GAUSSIAN)[name]
    keep = {k: c[k].copy() for k in ("rois", "scores", "boxes", "flip_width")}
    with _cfg_test(SOFT_NMS=name):
        got = postprocess_detections_batch(torch.from_numpy(c["scores"]), torch.from_numpy(c["boxes"]),
                                           torch.from_numpy(c["rois"]), c["n_images"], K, thresh=S.THRESH, max_per_image=cap,
                                           views=views, flip_width=torch.from_numpy(c["flip_width"]))
        # the single-image path on image 0's merged, un-mirrored rows
        s0, b0, _ = T.image_rows(c["rois"], c["scores"], c["boxes"], 0, views, c["n_images"], c["flip_width"])
        one = postprocess_detections(torch.from_numpy(np.array(s0)), torch.from_numpy(np.array(b0)), K, S.THRESH, cap)
    want = S.post_soft(c["rois"], c["scores"], c["boxes"], c["n_images"], views, c["flip_width"], K, S.THRESH, cap, method)
    total = 0
    for t in range(c["n_images"]):
        for j in range(1, K):
            assert T.same_bits(got[t][j].numpy(), want[t][j]), (t, j)
            total += len(want[t][j])
    assert total > 0
    for j in range(1, K):
        assert T.same_bits(one[j].numpy(), want[0][j]), j
    for k, v in keep.items():
        assert np.array_equal(c[k], v), k


def test_off_takes_the_path_of_before(monkeypatch):
    import torch
    from wssdl_bus_amd.fast_rcnn import detect_batch, soft_nms
    c = T.build_case(7, (9, 5), 1, 3, mirrored=())

    def boom(*a, **k):
        raise AssertionError("soft route reached")
    monkeypatch.setattr(soft_nms, "postprocess_soft_batch", boom)
    monkeypatch.setattr(detect_batch, "postprocess_detections", lambda *a, **k: "before")
    args = (torch.from_numpy(c["scores"]), torch.from_numpy(c["boxes"]), torch.from_numpy(c["rois"]), 2, 3)
    assert detect_batch.postprocess_detections_batch(*args, thresh=T.THRESH) == ["before", "before"]
    with _cfg_test(SOFT_NMS="linear"):
        with pytest.raises(AssertionError, match="soft route reached"):
            detect_batch.postprocess_detections_batch(*args, thresh=T.THRESH)


# ----------------------------------------------------------------------------------------------------- cfg ---
def test_config_keys_errors_and_cfg_from_list():
    import torch
    from wssdl_bus_amd.fast_rcnn.config import cfg, cfg_from_list
    from wssdl_bus_amd.fast_rcnn.detect_batch import postprocess_detections_batch
    from wssdl_bus_amd.fast_rcnn.post_detections import postprocess_detections
    from wssdl_bus_amd.fast_rcnn.soft_nms import soft_nms_method
    assert cfg.TEST.SOFT_NMS == "off" and cfg.TEST.SOFT_NMS_SIGMA == 0.5 and cfg.TEST.SOFT_NMS_MIN_SCORE == 0.001
    assert soft_nms_method() is None
    with _cfg_test(SOFT_NMS="off", SOFT_NMS_SIGMA=0.5, SOFT_NMS_MIN_SCORE=0.001):
        cfg_from_list(["TEST.SOFT_NMS", "gaussian", "TEST.SOFT_NMS_SIGMA", "0.25", "TEST.SOFT_NMS_MIN_SCORE", "0.01"])
        assert cfg.TEST.SOFT_NMS == "gaussian" and cfg.TEST.SOFT_NMS_SIGMA == 0.25 and cfg.TEST.SOFT_NMS_MIN_SCORE == 0.01
        assert soft_nms_method() == 2
    assert cfg.TEST.SOFT_NMS == "off"
    c = T.build_case(7, (9, 5), 1, 3, mirrored=())
    args = (torch.from_numpy(c["scores"]), torch.from_numpy(c["boxes"]), torch.from_numpy(c["rois"]), 2, 3)
    for kv in (dict(SOFT_NMS="linear", CLS_AGNOSTIC_NMS=True), dict(SOFT_NMS="gaussian", BBOX_VOTE=True),
               dict(SOFT_NMS="Linear"), dict(SOFT_NMS="hard"), dict(SOFT_NMS="gaussian", SOFT_NMS_SIGMA=0.0),
               dict(SOFT_NMS="linear", SOFT_NMS_MIN_SCORE=0.0), dict(SOFT_NMS="linear", SOFT_NMS_MIN_SCORE=1.0)):
        with _cfg_test(**kv):
            with pytest.raises(ValueError):
                postprocess_detections_batch(*args, thresh=T.THRESH)
            with pytest.raises(ValueError):
                postprocess_detections(args[0][:9], args[1][:9], 3, T.THRESH)


# ------------------------------------------------------------------------------------------------- C surface ---
def test_symbols_and_workspace_query(L):
    from wssdl_bus_amd import _lib
    for name in ("wssdl_post_detections_soft_workspace_bytes", "wssdl_post_detections_soft"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    q = L.wssdl_post_detections_soft_workspace_bytes
    top = _lib.POST_SOFT_MAX_ROWS
    assert top == 4096 and top * 24 <= 160 * 1024
    last = 0
    for p in (1, 2, 63, 64, 300, 600, 601, 2048, top):
        now = q(8, 2, p, 3)
        assert now >= last and now >= 8 * 2 * p * 5 * 4
        last = now
    assert q(1, 1, 300, 2) <= q(2, 1, 300, 2) <= q(2, 1, 300, 3) <= q(2, 8, 300, 3)
    assert q(8, 2, top + 1, 3) == 0 and q(1, 1, 1 << 30, 2) == 0
    assert q(0, 2, 300, 3) == 0 and q(2, 0, 300, 3) == 0 and q(2, 9, 300, 3) == 0 and q(2, 2, 0, 3) == 0
    assert q(2, 2, 300, 1) == 0 and q(2, 2, 300, 66) == 0


def test_invalid_arguments_return_status_without_launch(L):
    from wssdl_bus_amd import _lib
    f = L.wssdl_post_detections_soft
    INVALID = _lib.ERR_INVALID_ARGUMENT
    tiny = float(np.finfo(np.float32).tiny)

    def call(R=10, n_images=2, views=2, P=600, K=3, thresh=0.05, method=1, nt=0.3, sigma=0.5, floor=0.001):
        return f(None, None, None, R, n_images, views, None, P, K, thresh, method, nt, sigma, floor, 300, None, None, None,
                 0, None)

    assert call(views=0) == INVALID
    assert call(views=9) == INVALID
    assert call(method=-1) == INVALID
    assert call(method=3) == INVALID
    for sigma in (0.0, -0.5, float("inf"), float("nan")):
        assert call(method=2, sigma=sigma, n_images=0) == INVALID
        assert call(method=1, sigma=sigma, n_images=0) == 0         # sigma is not read there
    for nt in (0.0, -0.1, 1.0000001, float("nan")):
        assert call(method=0, nt=nt, n_images=0) == INVALID
        assert call(method=1, nt=nt, n_images=0) == INVALID
        assert call(method=2, nt=nt, n_images=0) == 0               # nms_thresh is not read there
    assert call(nt=1.0, n_images=0) == 0
    for floor in (0.0, -1.0, tiny / 2, 1.0, 2.0, float("nan")):
        assert call(floor=floor, n_images=0) == INVALID
    assert call(floor=tiny, n_images=0) == 0
    assert call(floor=float(np.nextafter(np.float32(1), np.float32(0))), n_images=0) == 0
    assert call(thresh=-0.1, n_images=0) == INVALID
    assert call(thresh=float("nan"), n_images=0) == INVALID
    assert call(thresh=0.0, n_images=0) == 0
    assert call(K=1) == INVALID
    assert call(K=66) == INVALID                                # K - 1 > 64
    assert call(P=_lib.POST_SOFT_MAX_ROWS + 1) == INVALID
    assert call(P=_lib.POST_SOFT_MAX_ROWS + 1, n_images=0) == INVALID
    assert call(P=0) == INVALID                                 # max_rows_per_image < 1 with R > 0
    assert call(R=-1) == INVALID
    assert call(n_images=-1) == INVALID
    assert call(n_images=65, P=4096, K=65) == INVALID           # n_images * (K-1) * P > 2^24
    assert call(n_images=65536, P=1, K=2) == INVALID            # more than 65535 (image, class) segments
    assert call() == INVALID                                    # NULL pointers with R > 0
    assert call(R=0) == INVALID                                 # NULL counts with images to report
    # valid and nothing to do
    assert call(n_images=0) == 0
    assert call(R=0, n_images=0, P=0, views=8, method=2) == 0
