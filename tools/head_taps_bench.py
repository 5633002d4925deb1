"""One 3x3 convolution of the per-RoI head, forward + backward, on its three routes: the dense patch GEMM
(im2col.hip + F.linear), the class-packed GEMMs with one batched call per class group, and with one call per
class (networks/_plumbing.py: TapConv3x3Fn, TAP_GEMM_GROUPED).  Prints one JSON line per (shape, route).

    python tools/head_taps_bench.py [--R 8512] [--C 512] [--iters 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                       # noqa: E402
import torch.nn.functional as F                    # noqa: E402

from wssdl_bus_amd.networks import _plumbing       # noqa: E402


def run(route, x, W, plan, R, iters):
    xx = x.clone().requires_grad_(True)
    ww = W.clone().requires_grad_(True)
    in_pm = plan.h == plan.oh and route != "dense"
    src = xx.reshape(R, -1, x.shape[-1]).transpose(0, 1).reshape(-1, x.shape[-1]).contiguous() if in_pm else xx

    def step():
        if route == "dense":
            y = F.linear(_plumbing.Im2Col3x3Fn.apply(src, plan.s, plan.oh, plan.ow, plan.pt, plan.pl), ww)
        else:
            _plumbing.TAP_GEMM_GROUPED = route == "grouped"
            y = _plumbing.TapConv3x3Fn.apply(src, ww, None, plan, in_pm, R)
        t1 = torch.cuda.Event(enable_timing=True)
        t1.record()
        y.backward(torch.ones_like(y), retain_graph=False)
        return t1

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0, t2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fwd = bwd = 0.0
    for _ in range(iters):
        t0.record()
        t1 = step()
        t2.record()
        torch.cuda.synchronize()
        fwd += t0.elapsed_time(t1)
        bwd += t1.elapsed_time(t2)
    return fwd / iters, bwd / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=8512)
    ap.add_argument("--C", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    for h, s in ((7, 2), (4, 1)):
        plan = _plumbing.tap_plan(h, h, s)
        x = torch.randn((a.R, h, h, a.C), device="cuda", generator=g)
        W = torch.randn((a.C, 9 * a.C), device="cuda", generator=g) * 0.01
        dense_flop = 2.0 * a.R * plan.oh * plan.ow * 9 * a.C * a.C
        tap_flop = 2.0 * a.R * plan.units * a.C * a.C
        for route in ("dense", "grouped", "per_class"):
            f, b = run(route, x, W, plan, a.R, a.iters)
            flop = dense_flop if route == "dense" else tap_flop
            print(json.dumps({"shape": "%dx%d s%d" % (h, h, s), "R": a.R, "C": a.C, "route": route,
                              "fwd_ms": round(f, 3), "bwd_ms": round(b, 3), "total_ms": round(f + b, 3),
                              "gemm_tflop": round(3 * flop / 1e12, 3),
                              "tflops_incl_copies": round(3 * flop / ((f + b) * 1e-3) / 1e12, 1)}), flush=True)
    _plumbing.TAP_GEMM_GROUPED = True


if __name__ == "__main__":
    main()
