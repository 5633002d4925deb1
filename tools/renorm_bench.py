"""One batch-renormalisation layer (cfg.TRAIN.USE_BRN: rowbn_forward / rowbn_backward with the layer's renorm state,
ReLU on) next to the plain fused batch-norm layer on the SAME tensor, interleaved round by round in one process, at the
head's shapes [R*49, 1024] and [R*16, 2048] (R = 8512 RoIs) and the trunk's conv0 output [8*300*500, 64].

    python tools/renorm_bench.py [--R 8512] [--rounds 20] [--warmup 3] [--only head]

The claim it is there to confirm is structural: both forms issue the same launches and make the same passes over the
tensor (forward: column sums, finish, apply; backward: gradient sums, finish, apply), and only the two finish kernels
differ (rowbn_fwd_finish_renorm_kernel / rowbn_bwd_finish_renorm_kernel in place of rowbn_fwd_finish_kernel /
rowbn_bwd_finish_kernel).  Per shape it prints one JSON line with the median, fastest and slowest round of each form in
microseconds (device events around forward + backward, output allocation included, the same for both) and their
ratio; then, from one profiled round of each form (torch.profiler), a `kernels` line: the kernels of each form in
launch order with their device times, `same_but_finish` (the two lists agree once the finish kernels' names are
mapped onto each other) and the finish kernels' own times side by side.
"""
import argparse
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                       # noqa: E402

from wssdl_bus_amd.networks import _plumbing as P  # noqa: E402

EPS, MOM, RHO = 1e-3, 0.01, 0.99


def shapes(R):
    """(name, rows, C)"""
    return [("head %dx49x1024" % R, R * 49, 1024), ("head %dx16x2048" % R, R * 16, 2048),
            ("trunk 8x300x500x64", 8 * 300 * 500, 64)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def kernels_of(fn):
    """[(kernel name up to its template arguments, device microseconds)] of one call of fn, in launch order"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "rowbn" in e.name]
    evs.sort(key=lambda e: e.time_range.start)
    short = lambda n: re.search(r"rowbn_\w+", n).group(0)
    return [(short(e.name), round(e.time_range.elapsed_us(), 1)) for e in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=8512)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="substring of the shape names to run")
    ap.add_argument("--no-kernels", action="store_true", help="skip the profiled round")
    a = ap.parse_args()
    if not torch.cuda.is_available() or P.lib() is None:
        sys.exit("renorm_bench: needs a GPU and the plumbing library")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, M, C in shapes(a.R):
        if a.only not in name:
            continue
        x = torch.randn((M, C), device="cuda", generator=g)
        dy = torch.randn((M, C), device="cuda", generator=g)
        w, b = torch.rand((C,), device="cuda", generator=g) + 0.5, torch.rand((C,), device="cuda", generator=g) - 0.5
        assert P.usable(x)
        z = lambda v=0.0: torch.full((C,), v, device="cuda")
        run_p = (z(), z(1.0), MOM, torch.zeros((1,), dtype=torch.int64, device="cuda"))
        run_r = (z(), z(1.0), MOM, torch.zeros((1,), dtype=torch.int64, device="cuda"))
        ren = (z(), z(), z(), RHO)                  # a fresh layer; the state warms up over the rounds

        def plain():
            _, stats, _ = P.rowbn_forward(x, w, b, EPS, True, running=run_p)
            P.rowbn_backward(x, dy, w, stats, True)

        def renorm():
            _, stats, _ = P.rowbn_forward(x, w, b, EPS, True, running=run_r, renorm=ren)
            P.rowbn_backward(x, dy, w, stats, True)

        for _ in range(a.warmup):
            plain()
            renorm()
        torch.cuda.synchronize()
        t_p, t_r = [], []
        for _ in range(a.rounds):
            t_p.append(timed(plain))
            t_r.append(timed(renorm))
        m_p, m_r = statistics.median(t_p), statistics.median(t_r)
        print(json.dumps({"shape": name, "rounds": a.rounds, "T_bytes": M * C * 4,
                          "plain_us": [round(m_p, 1), round(min(t_p), 1), round(max(t_p), 1)],
                          "renorm_us": [round(m_r, 1), round(min(t_r), 1), round(max(t_r), 1)],
                          "renorm_over_plain": round(m_r / m_p, 4)}), flush=True)
        if not a.no_kernels:
            kp, kr = kernels_of(plain), kernels_of(renorm)
            mapped = [n.replace("_finish_renorm_kernel", "_finish_kernel") for n, _ in kr]
            fin = lambda ks: {n: t for n, t in ks if "finish" in n}
            print(json.dumps({"shape": name, "kernels": {"plain": kp, "renorm": kr},
                              "same_but_finish": mapped == [n for n, _ in kp] and len(kp) == 6,
                              "finish_us": {"plain": fin(kp), "renorm": fin(kr)}}), flush=True)
        del x, dy


if __name__ == "__main__":
    main()
