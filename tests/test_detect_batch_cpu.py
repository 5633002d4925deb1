"""The batched post-detection op's C-ABI surface without a GPU: both symbols exported and declared with the
argument counts of the ctypes table, the workspace query pure host, and bad arguments refused with a status
before anything is launched (every device pointer here is NULL)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wssdl_bus_hip.h")
SYMS = ("wssdl_post_detections_batched_workspace_bytes", "wssdl_post_detections_batched")


@pytest.fixture(scope="module")
def L():
    from wssdl_bus_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_batched_symbols_exported_and_declared(L):
    from wssdl_bus_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    text = open(HEADER).read()
    for name in SYMS:
        assert re.search(r" T %s$" % name, out, re.M), name
        m = re.search(r"WSSDL_API[^;(]*\b%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name


def test_batched_workspace_query_is_host_only_and_grows(L):
    ws = L.wssdl_post_detections_batched_workspace_bytes
    base = ws(4, 300, 3)
    assert base >= 4 * 2 * 300 * (8 + 8 + 4 + 4 + 16 + 16)
    assert ws(5, 300, 3) > base
    assert ws(4, 301, 3) > base
    assert ws(4, 300, 4) > base
    assert ws(0, 300, 3) > 0 and ws(4, 0, 3) > 0 and ws(4, 300, 1) > 0     # degenerate sizes: a small non-zero block
    # the single-image op is the one-image case of the same carve
    assert L.wssdl_post_detections_workspace_bytes(300, 3) == ws(1, 300, 3)


def test_batched_invalid_arguments_return_status_without_launch(L):
    from wssdl_bus_amd import _lib
    f = L.wssdl_post_detections_batched
    INVALID = _lib.ERR_INVALID_ARGUMENT

    def call(R, n_images, P, K, counts=None):
        return f(None, None, None, R, n_images, P, K, 0.05, 0.3, 300, None, counts, None, 0, None)

    assert call(10, -1, 300, 3) == INVALID                      # n_images < 0
    assert call(10, 2, 300, 1) == INVALID                       # num_classes < 2
    assert call(10, 2, 300, 66) == INVALID                      # K - 1 > 64
    assert call(10, 2, 0, 3) == INVALID                         # max_rows_per_image < 1 with R > 0
    assert call(-1, 2, 300, 3) == INVALID                       # R < 0
    assert call(10, 64, 4097, 65) == INVALID                    # n_images * (K-1) * P > 2^24
    assert call(10, 65536, 1, 2) == INVALID                     # more than 65535 (image, class) segments
    assert call(10, 2, 300, 3) == INVALID                       # NULL counts
    assert call(10, 0, 300, 3) == 0                             # no image: nothing to do, nothing launched
    assert call(0, 0, 0, 3) == 0
