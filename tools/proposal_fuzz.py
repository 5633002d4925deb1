#!/usr/bin/env python3
"""Random proposal-layer cases decided by the NumPy statement of the decode kernel's arithmetic (tests/boxcode_reference.py:
decode_anchor of csrc/proposal.hip restated operation by operation, the exponential an f64 exp rounded once to f32): random
batch / map sizes, image sizes and scales, train / test, box-delta magnitudes from 0 (the anchors themselves: heavy
suppression) to 1.  Per image: the decoded boxes BIT FOR BIT, the candidate order exact (scores pairwise distinct), the
kept rows == the oracle's NMS (oracle/np_oracle.py, the reference's own Cython rule) on the STATEMENT's boxes and scores,
bit for bit -- nothing of the product on the expected side.  The precondition of bit equality is that no exp lies within
4 f64 ulps of an f32 rounding boundary: a drawn delta that does is redrawn before the case runs.  A box at the min-size
threshold is decided like any other (the statement says on which side it falls): no case is skipped, and the final line's
'filter-edge' count, kept for its readers, is always 0.
    python3 tools/proposal_fuzz.py [--cases 40] [--seed 0]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import boxcode_reference as B  # noqa: E402
from oracle import np_oracle as O  # noqa: E402
from wssdl_bus_amd.rpn_msr.proposal_layer_tf_bus import proposal_layer, proposal_layer_padded  # noqa: E402

SCALES = np.array([8, 16, 32])
ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=40)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
rs = np.random.RandomState(args.seed)
bad = redrawn = 0
for k in range(args.cases):
    N = int(rs.randint(1, 5))
    H, W = int(rs.randint(10, 65)), int(rs.randint(10, 101))
    train = bool(k % 2)
    pre, post = (12000, 2000) if train else (6000, 300)
    K = H * W * 9
    prob = np.zeros((N, H, W, 18), np.float32)
    for i in range(N):
        fg = ((rs.permutation(K) + 1).astype(np.float32) / np.float32(K + 1)).reshape(H, W, 9)     # pairwise distinct
        prob[i, :, :, 9:] = fg
        prob[i, :, :, :9] = 1 - fg
    mag = float(rs.choice([0.0, 0.05, 0.3, 1.0]))
    pred = (rs.normal(0, 1, (N, H, W, 36)) * mag).astype(np.float32)
    sizes = pred.reshape(-1, 4)[:, 2:4]                                # (a view)
    while True:
        unsafe = ~B.exp_is_safe(sizes)
        if not unsafe.any():
            break
        redrawn += int(unsafe.sum())
        sizes[unsafe] = (rs.normal(0, 1, int(unsafe.sum())) * (mag if mag else 1e-3)).astype(np.float32)
    sc = float(rs.choice([1.0, 1.0, 1.6, 0.625]))
    info = np.array([[H * 16 - rs.randint(0, 16), W * 16 - rs.randint(0, 16), sc, 1]] * N, np.float32)
    rois_p, counts, dec, sidx, scnt = [t.cpu().numpy() for t in proposal_layer_padded(prob, pred, info, train, [16], SCALES, debug=True)]
    blob = proposal_layer(prob, pred, info, train, False, [16], SCALES)
    st = B.proposal_statement(prob, pred, info)
    order = B.candidate_order(st["scores"], st["valid"], pre if 0 < pre < K else 0)
    ok, off, why = True, 0, ""
    for i in range(N):
        differ = dec[i].view(np.int32) != st["boxes"][i].view(np.int32)
        if differ.any():
            j = int(np.argwhere(differ)[0, 0])
            ok, why = False, "decode: %d values differ, first at anchor %d deltas %s got %s want %s" % (
                int(differ.sum()), j, pred[i].reshape(-1, 4)[j], dec[i][j], st["boxes"][i][j])
            break
        n = int(scnt[i])
        if n != len(order[i]) or not np.array_equal(sidx[i, :n], order[i]):
            ok, why = False, "order (%d candidates against %d)" % (n, len(order[i]))
            break
        dets = np.hstack((st["boxes"][i][order[i]], st["scores"][i][order[i]][:, None])).astype(np.float32)
        keep = np.asarray(O.nms(dets, 0.7)[:post], dtype=np.int64)
        c = int(counts[i])
        if c != len(keep) or not np.array_equal(rois_p[i, :c, 1:], dets[keep, :4]) or rois_p[i, c:].any() or \
                not np.all(rois_p[i, :c, 0] == i) or not np.array_equal(blob[off:off + c], rois_p[i, :c]):
            ok, why = False, "nms / rows (%d against %d)" % (c, len(keep))
            break
        off += c
    if not ok:
        bad += 1
        print("MISMATCH case %d N %d map %dx%d train %s scale %.3f: %s" % (k, N, H, W, train, sc, why), flush=True)
    if (k + 1) % 10 == 0:
        print("case %d ok so far (%d mismatches, %d deltas redrawn)" % (k + 1, bad, redrawn), flush=True)
print("cases %d mismatches %d filter-edge 0" % (args.cases, bad))
sys.exit(1 if bad else 0)
