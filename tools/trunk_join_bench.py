"""The unmasked residual-join kernels (csrc/plumbing/rowbn.hip, the <*, 0> instantiations the trunk runs) alone at
one trunk shape, next to the separate kernels they replace: run it under `rocprofv3 --kernel-trace`, then let it
read the trace back and set each kernel's device time against the bytes it must move (T = one [M, C] f32 tensor;
passes from the table of DESIGN.md section 7).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/trunk_join_bench.py --M 296808 --C 256
    python tools/trunk_join_bench.py --M 296808 --C 256 --summarize DIR

Trunk shapes at 8 x 600 x 1000: group0 [296808, 256], group1 [75000, 512], group2 [19152, 1024].
"""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# tensors each kernel must move, in T (reads + writes)
PASSES = {"rowbn_join_fwd_kernel<false": 3, "rowbn_join_fwd_kernel<true": 3, "rowbn_join_bwd_kernel<false, true": 5,
          "rowbn_join_bwd_kernel<false, false": 4, "rowbn_join_bwd_kernel<true, true": 6,
          "rowbn_join_bwd_kernel<true, false": 5, "rowbn_apply_bwd_dual_kernel": 5,
          # the separate layers
          "rowbn_partial_kernel<0": 1, "rowbn_partial_kernel<1": 2, "rowbn_apply_fwd_kernel": 2,
          "rowbn_apply_bwd_kernel": 3, "CUDAFunctor_add": 3}


def run(a):
    import torch
    from wssdl_bus_amd.networks import _plumbing as P
    g = torch.Generator(device="cuda").manual_seed(0)
    x3, other, dy, dres = (torch.randn((a.M, a.C), device="cuda", generator=g) for _ in range(4))
    bn = lambda: (torch.rand((a.C,), device="cuda", generator=g) + 0.5, torch.zeros((a.C,), device="cuda"), 1e-3)
    b3, bs, bn_ = bn(), bn(), bn()
    for _ in range(a.iters):
        for dual in (False, True):
            out, y, s3, ss, sn, _ = P.rowbn_join_forward(x3, b3, other, bs if dual else None, bn_, None)
            for res in (dres, None):
                P.rowbn_join_backward(out, dy, res, x3, other if dual else None, bn_[0], sn, b3[0], s3,
                                      bs[0] if dual else None, ss if dual else None, None)
        # the separate layers of the identity form: bn3, add, next norm + ReLU; their backwards and the add
        t3, st3, _ = P.rowbn_forward(x3, b3[0], b3[1], b3[2], False)
        out = t3 + other
        y, stn, _ = P.rowbn_forward(out, bn_[0], bn_[1], bn_[2], True)
        dxn, _, _ = P.rowbn_backward(out, dy, bn_[0], stn, True)
        gg = dxn + dres
        P.rowbn_backward(x3, gg, b3[0], st3, False)
    torch.cuda.synchronize()
    print(json.dumps({"M": a.M, "C": a.C, "T_bytes": a.M * a.C * 4}))


def summarize(a):
    f = max(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    T = a.M * a.C * 4
    agg = {}
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        key = next((k for k in sorted(PASSES, key=len, reverse=True) if k in name), None)
        if key is None:
            continue
        if key.startswith("rowbn_") and key[-1] != ">":
            key = name[name.index(key):].split("(")[0]          # the full instantiation
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        agg.setdefault(key, []).append(us)
    print("# M=%d C=%d T=%.1f MB; median device time per launch" % (a.M, a.C, T / 1e6))
    for k in sorted(agg):
        v = sorted(agg[k])
        med = v[len(v) // 2]
        p = next(PASSES[q] for q in sorted(PASSES, key=len, reverse=True) if q in k)
        print("%-52s launches=%3d  %8.1f us  %dT  %.2f TB/s" % (k[:52], len(v), med, p, p * T / med / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=296808)
    ap.add_argument("--C", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--summarize", default="", metavar="DIR", help="read the kernel trace under DIR instead of running")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)


if __name__ == "__main__":
    main()
