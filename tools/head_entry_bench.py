"""The start of the per-RoI head, kernel by kernel: the patch gather and its adjoint (csrc/plumbing/taps.hip) on
both head shapes and both input layouts, and block 1's entry gradient (rowbn.hip: wsplumb_rowbn_backward_entry)
beside the separate ops it replaces.  Prints one JSON line per kernel: event time per call, the bytes the call
must move (every input and output element once) and that as TB/s and as a share of 8 TB/s.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel times.

    python tools/head_entry_bench.py [--R 7000] [--C 512] [--iters 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                       # noqa: E402

from wssdl_bus_amd.networks import _plumbing       # noqa: E402

PEAK_TBS = 8.0


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def report(name, ms, nbytes, **kw):
    tbs = nbytes / (ms * 1e-3) / 1e12
    print(json.dumps(dict(kernel=name, ms=round(ms, 4), gbytes=round(nbytes / 1e9, 3), tb_per_s=round(tbs, 2),
                          share_of_peak=round(tbs / PEAK_TBS, 3), **kw)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=7000)
    ap.add_argument("--C", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    R, C = a.R, a.C
    g = torch.Generator(device="cuda").manual_seed(0)
    for h, s in ((7, 2), (4, 1)):
        plan = _plumbing.tap_plan(h, h, s)
        x = torch.randn((R, h, h, C), device="cuda", generator=g)
        dcols = torch.randn((plan.units * R * C,), device="cuda", generator=g)
        nbytes = 4.0 * (h * h + plan.units) * R * C
        for in_pm in ((False, True) if plan.h == plan.oh else (False,)):
            tag = dict(shape="%dx%d s%d" % (h, h, s), layout="position-major" if in_pm else "roi-major", R=R, C=C)
            src = x.view(-1, C) if in_pm else x
            report("tap_gather", timed(lambda: _plumbing.tap_gather(src, plan, in_pm, R), a.iters), nbytes, **tag)
            report("tap_col2im", timed(lambda: _plumbing.tap_col2im(dcols, plan, in_pm, R, C), a.iters), nbytes, **tag)
        del x, dcols
    if not hasattr(_plumbing, "rowbn_backward_entry"):
        return
    # block 1's pre-activation norm backward: C_in = 2 * C channels over 49 positions, 16 of them sampled
    Ci, per = 2 * C, 49
    plan = _plumbing.tap_plan(7, 7, 2)
    ns = len(plan.slots)
    x = torch.randn((R * per, Ci), device="cuda", generator=g)
    w = torch.rand((Ci,), device="cuda", generator=g) + 0.5
    b = torch.zeros((Ci,), device="cuda")
    mask = (torch.rand((R,), device="cuda", generator=g) > 0.1).float()
    dy = torch.randn((R * per, Ci), device="cuda", generator=g)
    dys = torch.randn((ns * R, Ci), device="cuda", generator=g)
    _, stats, _ = _plumbing.rowbn_forward(x, w, b, 1e-3, True, mask)
    idx = plan.subsample_index(7, 2, x.device)
    inv = plan.subsample_slots(7, 7, 2, x.device)

    def separate():
        z = torch.zeros((per, R, Ci), device="cuda").index_add_(0, idx, dys.view(ns, R, Ci))
        total = dy.view(R, per, Ci) + z.transpose(0, 1)
        return _plumbing.rowbn_backward(x, total.contiguous().view(-1, Ci), w, stats, True, mask)

    def entry():
        return _plumbing.rowbn_backward_entry(x, dy, dys, inv, ns, w, stats, mask)

    # two passes read x and the two gradient parts, the second writes dx
    nbytes = 4.0 * Ci * R * (2 * (2 * per + ns) + per)
    tag = dict(R=R, C=Ci, live=float(mask.mean()))
    report("entry backward, separate ops (scatter, add, rowbn_backward)", timed(separate, a.iters), nbytes, **tag)
    report("entry backward, rowbn_backward_entry", timed(entry, a.iters), nbytes, **tag)


if __name__ == "__main__":
    main()
