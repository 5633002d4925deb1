"""The norm-applying patch gather (csrc/plumbing/taps.hip: tap_gather_kernel<true>) and the one-launch L2 decay
(csrc/plumbing/l2decay.hip) alone, next to what they replace, at fixed shapes: device time of each kernel from a
`rocprofv3 --kernel-trace` run of this script is set against the bytes it must move, which it prints.

    rocprofv3 --kernel-trace --stats ... -- python tools/tapnorm_l2decay_bench.py [--R 7000] [--C 512] [--iters 10]

Per iteration and geometry: rowbn_forward (partial, finish, apply) + tap_gather, then rowbn_stats (partial, finish) +
tap_gather_norm.  The apply pass (one read and one write of the [h*w*R, C] tensor) is what goes; the gather reads
and writes the same bytes either way.  Then the decay over a ResNet-50-sized parameter list: torch's chain forward and
backward, then the op's.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                       # noqa: E402

from wssdl_bus_amd.networks import _plumbing as P  # noqa: E402

GEOMS = [(7, 7, 2, False), (4, 4, 1, True)]        # block 1 (roi-major source), blocks 2 and 3 (position-major)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=7000)
    ap.add_argument("--C", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    R, C = a.R, a.C
    g = torch.Generator(device="cuda").manual_seed(0)
    mask = torch.ones((R,), device="cuda")
    w, b = torch.rand((C,), device="cuda", generator=g) + 0.5, torch.zeros((C,), device="cuda")
    info = {"R": R, "C": C, "geoms": []}
    for h, wd, s, in_pm in GEOMS:
        plan = P.tap_plan(h, wd, s)
        x = torch.randn((h * wd * R, C), device="cuda", generator=g)
        for _ in range(a.iters):
            y, _, _ = P.rowbn_forward(x, w, b, 1e-3, True, mask, in_pm)
            P.tap_gather(y, plan, in_pm, R)
            stats, _ = P.rowbn_stats(x, w, b, 1e-3, mask, in_pm)
            P.tap_gather_norm(x, plan, in_pm, R, stats[3], stats[4], mask)
        info["geoms"].append({"h": h, "w": wd, "s": s, "in_pm": in_pm, "x_bytes": x.numel() * 4,
                              "cols_bytes": plan.units * R * C * 4,
                              "gather_bytes_lower_bound": (x.numel() + plan.units * R * C) * 4,
                              "apply_bytes_removed": 2 * x.numel() * 4})
    # ResNet-50-sized decay list: 58 weights, about 2.6e7 floats
    shapes = [(64, 3, 7, 7)] + [(256, 64, 1, 1)] * 10 + [(128, 128, 3, 3)] * 4 + [(512, 256, 1, 1)] * 12 + \
             [(256, 256, 3, 3)] * 6 + [(1024, 512, 1, 1)] * 14 + [(512, 4608)] * 3 + [(2048, 1024)] * 7 + [(5, 2048)]
    params = [(torch.randn(sh, device="cuda", generator=g) * 0.05).requires_grad_() for sh in shapes]
    n = sum(p.numel() for p in params)
    for _ in range(a.iters):
        torch.stack([(p * p).sum() for p in params]).sum().mul(2.5e-4).backward()
        for p in params:
            p.grad = None
        P.l2_decay(params, 2.5e-4).backward()
        for p in params:
            p.grad = None
    torch.cuda.synchronize()
    info["decay"] = {"params": len(params), "floats": n, "forward_bytes": 4 * n, "backward_bytes": 8 * n}
    print(json.dumps(info))


if __name__ == "__main__":
    main()
