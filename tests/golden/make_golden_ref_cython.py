#!/usr/bin/env python3
"""Generate tests/golden/ref_cython_random.npz: the outputs of the reference's own Cython kernels
(oracle/_ref, built by oracle/build_ref.py) on the seeded random inputs of the three
`*_vs_reference_cython*` tests in tests/test_oracle_golden.py, so that those tests also pin the
oracle where oracle/_ref cannot be built.

Run where oracle/_ref is built:  python tests/golden/make_golden_ref_cython.py
Data only: inputs and outputs (IoU matrices as SHA-256 digests of their float64 bytes, keep lists
whole).  Re-running reproduces the same arrays (legacy numpy RandomState streams are frozen).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_kernels  # noqa: E402

NMS_SIZES = (1, 7, 200, 1500)
NMS_THRESH = (0.3, 0.5, 0.7)


def digest(*arrays):
    """SHA-256 of float64 C-order bytes (+ 0.0: -0.0 and 0.0 compare equal, so they hash alike)."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64) + 0.0).tobytes())
    return h.hexdigest()


def bbox_cases():
    """(boxes, query) of test_bbox_overlaps_vs_reference_cython, in order."""
    rs = np.random.RandomState(0)
    for _ in range(5):
        xy = rs.uniform(-50, 900, size=(3000, 2))
        b = np.hstack((xy, xy + rs.uniform(0, 500, size=(3000, 2))))
        q = b[rs.choice(3000, 20, replace=False)] + rs.uniform(-5, 5, size=(20, 4))
        yield b, q


def cpu_nms_cases():
    """(n, dets) of test_nms_vs_reference_cython_random, in order."""
    rs = np.random.RandomState(1)
    for n in NMS_SIZES:
        c = rs.uniform(0, 300, size=(n, 2))
        wh = rs.uniform(5, 120, size=(n, 2))
        yield n, np.hstack((c, c + wh, rs.permutation(n)[:, None] / float(n))).astype(np.float32)


def utils_nms_cases():
    """(n, dets) of test_utils_nms_vs_reference_cython_random, in order (nested boxes are common)."""
    rs = np.random.RandomState(2)
    for n in NMS_SIZES:
        c = rs.uniform(0, 300, size=(n, 2))
        wh = np.exp(rs.uniform(np.log(4), np.log(200), size=(n, 2)))
        yield n, np.hstack((c, c + wh, rs.permutation(n)[:, None] / float(n))).astype(np.float32)


def keep_key(fn, n, th):
    return "%s/n%d_t%02d" % (fn, n, int(round(th * 10)))


def main():
    if not ref_kernels.available() or ref_kernels.nms_new is None:
        sys.exit("oracle/_ref is not built (python oracle/build_ref.py)")
    out = {}
    for i, (b, q) in enumerate(bbox_cases()):
        out["bbox/%d/inputs" % i] = np.array(digest(b, q))
        out["bbox/%d/iou" % i] = np.array(digest(ref_kernels.bbox_overlaps(b, q)))
        out["bbox/%d/ui" % i] = np.array(digest(ref_kernels.bbox_overlaps_ui(b, q)))
    for n, d in cpu_nms_cases():
        out["cpu_nms/n%d_dets" % n] = d
        for th in NMS_THRESH:
            out[keep_key("cpu_nms", n, th)] = np.array(ref_kernels.cpu_nms(d, th), dtype=np.int32)
    for n, d in utils_nms_cases():
        out["utils_nms/n%d_dets" % n] = d
        for th in NMS_THRESH:
            out[keep_key("utils_nms", n, th)] = np.array(ref_kernels.nms(d, th), dtype=np.int32)
            out[keep_key("utils_nms_new", n, th)] = np.array(ref_kernels.nms_new(d, th), dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "ref_cython_random.npz"), **out)


if __name__ == "__main__":
    main()
