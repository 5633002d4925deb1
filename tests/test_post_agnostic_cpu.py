"""Class-agnostic post-detection op, host side: the four exports, the workspace queries (pure host code), the status
codes that come back before any launch, and the NumPy statement of the contract (tests/post_agnostic_reference.py) on
hand-made cases.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import post_agnostic_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wssdl_bus_hip.h")
OK, INVALID, WORKSPACE = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    from wssdl_bus_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _max_union():
    m = re.search(r"#define\s+WSSDL_POST_AGNOSTIC_MAX_UNION\s+(\d+)", open(HEADER).read())
    assert m, "the header states the bound on the union segment"
    return int(m.group(1))


def test_symbols_resolve_and_bound_is_declared(L):
    from wssdl_bus_amd import _lib
    for name in ("wssdl_post_detections_agnostic_batched_workspace_bytes", "wssdl_post_detections_agnostic_batched",
                 "wssdl_post_detections_agnostic_workspace_bytes", "wssdl_post_detections_agnostic"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    # the per-class pair keeps its argument lists
    assert _lib.SYMBOLS["wssdl_post_detections_agnostic"] == _lib.SYMBOLS["wssdl_post_detections"]
    assert _lib.SYMBOLS["wssdl_post_detections_agnostic_batched"] == _lib.SYMBOLS["wssdl_post_detections_batched"]
    assert _max_union() >= 4096 and _max_union() == _lib.POST_AGNOSTIC_MAX_UNION


def test_workspace_queries(L):
    q = L.wssdl_post_detections_agnostic_batched_workspace_bytes
    per_class = L.wssdl_post_detections_batched_workspace_bytes
    for n, p, k in ((1, 1, 2), (1, 300, 3), (8, 300, 3), (40, 65, 3), (4, 22, 9), (1, 4096, 2), (2, 6000, 3)):
        assert q(n, p, k) >= per_class(n, p, k), (n, p, k)
        # the union's suppression matrix alone: U x pitch(U) words per image, U = (K-1) * P padded to 16
        u = ((k - 1) * p + 15) // 16 * 16
        assert q(n, p, k) >= per_class(n, p, k) + n * u * (((u + 63) // 64 + 15) // 16 * 16) * 8, (n, p, k)
    assert q(8, 300, 3) > q(4, 300, 3) > q(1, 300, 3)               # grows with N
    assert q(8, 600, 3) > q(8, 301, 3) > q(8, 300, 3)               # ... with P
    assert q(8, 300, 9) > q(8, 300, 4) > q(8, 300, 3)               # ... with K
    for bad in ((0, 300, 3), (-1, 300, 3), (8, 0, 3), (8, -5, 3), (8, 300, 1), (8, 300, 0)):
        assert q(*bad) == 256, bad
    single = L.wssdl_post_detections_agnostic_workspace_bytes
    for r, k in ((1, 2), (300, 3), (63, 9), (4096, 2)):
        assert single(r, k) == q(1, r, k)
    assert single(0, 3) == 256 and single(300, 1) == 256


def test_status_codes_without_a_launch(L):
    """Every call here returns before the first launch: NULL pointers are never dereferenced."""
    f = L.wssdl_post_detections_agnostic_batched
    g = L.wssdl_post_detections_agnostic
    counts = (ctypes.c_int32 * 64)()
    cp = ctypes.cast(counts, ctypes.c_void_p)
    x = ctypes.c_void_p(256)            # a non-NULL pointer value that is only compared with NULL
    big = ctypes.c_size_t(1 << 40)
    mu = _max_union()
    # rois, scores, boxes, R, n_images, P, K, thresh, nms, cap, dets, counts, ws, ws_bytes, stream
    assert f(x, x, x, 10, 1, 10, 1, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID          # K < 2
    assert f(x, x, x, 10, 1, 10, 66, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID         # nc > 64
    assert f(x, x, x, 10, 1, mu // 2 + 1, 3, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID  # U over the bound
    assert f(x, x, x, 10, 2, mu + 1, 2, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID
    assert f(x, x, x, 10, 1, 0, 3, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID           # P < 1 with R > 0
    assert f(None, x, x, 10, 2, 10, 3, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID       # no blob, two images
    assert f(x, x, x, 10, 1, 10, 3, 0.05, 0.3, 300, x, None, x, big, None) == INVALID        # counts = NULL
    assert f(x, x, x, -1, 1, 10, 3, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID
    assert f(x, x, x, 10, 1, 10, 3, 0.05, 0.3, 300, x, cp, None, big, None) == INVALID       # no workspace
    # at the bound the arguments are valid: a short workspace is what is wrong
    need = L.wssdl_post_detections_agnostic_batched_workspace_bytes(1, mu // 2, 3)
    assert f(x, x, x, 10, 1, mu // 2, 3, 0.05, 0.3, 300, x, cp, x, ctypes.c_size_t(need - 1), None) == WORKSPACE
    need = L.wssdl_post_detections_agnostic_batched_workspace_bytes(2, 10, 3)
    assert need > L.wssdl_post_detections_batched_workspace_bytes(2, 10, 3)
    # what suffices for the per-class op does not suffice here
    short = ctypes.c_size_t(L.wssdl_post_detections_batched_workspace_bytes(2, 10, 3))
    assert f(x, x, x, 10, 2, 10, 3, 0.05, 0.3, 300, x, cp, x, short, None) == WORKSPACE
    assert f(x, x, x, 10, 0, 10, 3, 0.05, 0.3, 300, x, cp, x, big, None) == OK               # no image: no-op
    assert f(x, x, x, 10, 0, 10, 3, 0.05, 0.3, 300, x, None, x, big, None) == OK
    # the single-image form
    assert g(x, x, 10, 1, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID
    assert g(x, x, 10, 66, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID
    assert g(x, x, 10, 3, 0.05, 0.3, 300, x, None, x, big, None) == INVALID
    assert g(x, x, mu // 2 + 1, 3, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID
    assert g(x, x, -1, 3, 0.05, 0.3, 300, x, cp, x, big, None) == INVALID
    assert g(x, x, 10, 3, 0.05, 0.3, 300, x, cp, x, ctypes.c_size_t(1024), None) == WORKSPACE
    # the per-class exports have no such bound (their signatures and limits are unchanged)
    assert L.wssdl_post_detections_batched(x, x, x, 10, 1, mu // 2 + 1, 3, 0.05, 0.3, 300, x, cp, x,
                                           ctypes.c_size_t(1024), None) == WORKSPACE


# ---------------------------------------------------------------- the NumPy statement on hand-made cases ---
def _rows(K, rows):
    """rows: list of {class j: (x1, y1, x2, y2, score)}; a class that is not named scores 0 with a unit box"""
    scores = np.zeros((len(rows), K), np.float32)
    boxes = np.zeros((len(rows), 4 * K), np.float32)
    boxes[:, 2::4] = 1
    boxes[:, 3::4] = 1
    for r, row in enumerate(rows):
        for j, v in row.items():
            boxes[r, 4 * j:4 * j + 4] = v[:4]
            scores[r, j] = v[4]
    return scores, boxes


def test_statement_same_mass_two_classes():
    """benign and malignant boxes of one mass overlap almost completely: the lower-scored one goes, whichever class"""
    s, b = _rows(3, [{1: (100, 100, 200, 200, 0.9), 2: (102, 98, 203, 199, 0.6)},
                     {1: (400, 400, 480, 470, 0.4), 2: (401, 402, 482, 469, 0.7)},
                     {1: (700, 100, 760, 150, 0.5)}])
    per = REF.post_detections(s, b, 3, 0.05, 300, 0.3, agnostic=False)
    assert len(per[1]) == 3 and len(per[2]) == 2
    got = REF.post_detections(s, b, 3, 0.05, 300, 0.3)
    assert got[1][:, 4].tolist() == [np.float32(0.9), np.float32(0.5)]
    assert got[2][:, 4].tolist() == [np.float32(0.7)]
    assert got[1][0, :4].tolist() == [100, 100, 200, 200] and got[2][0, :4].tolist() == [401, 402, 482, 469]


def test_statement_class_emptied_by_the_union_pass():
    s, b = _rows(3, [{1: (100, 100, 200, 200, 0.9), 2: (101, 101, 201, 201, 0.8)},
                     {1: (400, 400, 480, 470, 0.7), 2: (400, 401, 481, 470, 0.3)}])
    got = REF.post_detections(s, b, 3, 0.05, 300, 0.3)
    assert len(got[1]) == 2 and got[2].shape == (0, 5) and got[2].dtype == np.float32


def test_statement_cap_cuts_inside_a_class():
    rows = [{1: (200 * i, 0, 200 * i + 50, 50, 0.9 - 0.1 * i)} for i in range(4)]
    rows += [{2: (200 * i, 300, 200 * i + 50, 350, 0.85 - 0.1 * i)} for i in range(4)]
    rows += [{2: (1, 1, 51, 49, 0.2)}]                  # class 2's copy of class 1's best box: the union pass drops it
    s, b = _rows(3, rows)
    got = REF.post_detections(s, b, 3, 0.05, 5, 0.3)
    # union survivors: .9 .8 .7 .6 (class 1), .85 .75 .65 .55 (class 2); the 5th largest is .7
    assert np.array_equal(got[1][:, 4], np.array([0.9, 0.8, 0.7], np.float32))
    assert np.array_equal(got[2][:, 4], np.array([0.85, 0.75], np.float32))
    uncapped = REF.post_detections(s, b, 3, 0.05, 0, 0.3)
    assert len(uncapped[1]) == 4 and len(uncapped[2]) == 4
    assert len(REF.post_detections(s, b, 3, 0.05, 0, 0.3, agnostic=False)[2]) == 5


def test_statement_two_classes_equal_per_class_oracle():
    """K = 2: the union pass re-runs NMS on an NMSed list and finds nothing to suppress"""
    rs = np.random.RandomState(4)
    n = 150
    ctr = rs.uniform(50, 600, size=(n, 1, 2))
    wh = rs.uniform(30, 220, size=(n, 2, 2))
    b = np.concatenate((ctr - wh / 2, ctr + wh / 2), axis=2).reshape(n, 8).astype(np.float32)
    s = rs.uniform(0, 1, size=(n, 2)).astype(np.float32)
    for cap in (0, 7, 300):
        a = REF.post_detections(s, b, 2, 0.05, cap, 0.3)
        p = REF.post_detections(s, b, 2, 0.05, cap, 0.3, agnostic=False)
        assert a[1].shape[0] > 0 and np.array_equal(a[1], p[1])
    assert REF.ties_are_harmless(s, b, 2, 0.05, 0.3)
    s[:2, 1] = 0.5
    b[1, 4:8] = b[0, 4:8]
    assert not REF.ties_are_harmless(s, b, 2, 0.05, 0.3)
