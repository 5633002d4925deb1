"""The residual-join kernels of the per-RoI head (csrc/plumbing/rowbn.hip) alone, at a fixed shape: device
time of each kernel from a `rocprofv3 --kernel-trace` run of this script is set against the bytes it must
move (T = one [16R, C] f32 tensor).  Run it under the profiler; it prints the shape and T.

    rocprofv3 --kernel-trace --stats ... -- python tools/head_join_bench.py [--R 7000] [--C 2048] [--iters 10]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                       # noqa: E402

from wssdl_bus_amd.networks import _plumbing as P  # noqa: E402

# tensors each kernel must move, in T (reads + writes): the pass table of DESIGN.md section 7
PASSES = {"rowbn_join_fwd_kernel<false": 3, "rowbn_join_fwd_kernel<true": 3, "rowbn_join_bwd_kernel<false, true": 5,
          "rowbn_join_bwd_kernel<false, false": 4, "rowbn_join_bwd_kernel<true, true": 6,
          "rowbn_apply_bwd_dual_kernel": 5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=7000)
    ap.add_argument("--C", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    M = 16 * a.R
    g = torch.Generator(device="cuda").manual_seed(0)
    x3, other, dy, dres = (torch.randn((M, a.C), device="cuda", generator=g) for _ in range(4))
    mask = torch.ones((a.R,), device="cuda")
    bn = lambda: (torch.rand((a.C,), device="cuda", generator=g) + 0.5, torch.zeros((a.C,), device="cuda"), 1e-3)
    b3, bs, bn_ = bn(), bn(), bn()
    for _ in range(a.iters):
        for dual in (False, True):
            out, y, s3, ss, sn, _ = P.rowbn_join_forward(x3, b3, other, bs if dual else None, bn_, mask)
            for res in ((dres, None) if not dual else (dres,)):
                P.rowbn_join_backward(out, dy, res, x3, other if dual else None, bn_[0], sn, b3[0], s3,
                                      bs[0] if dual else None, ss if dual else None, mask)
    torch.cuda.synchronize()
    print(json.dumps({"R": a.R, "C": a.C, "T_bytes": M * a.C * 4, "passes_T": PASSES}))


if __name__ == "__main__":
    main()
