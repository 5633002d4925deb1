"""One group-norm layer (csrc/plumbing/groupnorm.hip: groupnorm_forward + groupnorm_backward, ReLU on) next to the
fused batch-norm layer (rowbn_forward + rowbn_backward) on the SAME tensor, interleaved round by round in one process,
at the shapes the train workload gives the two networks: the head's [R*49, C] and [R*16, C] (R = 8512 RoIs, a sample is
one RoI; sample-major and position-major rows) and the trunk's conv0 output [8*300*500, 64] (a sample is an image).

    python tools/groupnorm_bench.py [--R 8512] [--rounds 20] [--warmup 3]
    rocprofv3 --kernel-trace --stats ... -- python tools/groupnorm_bench.py --rounds 3        # the per-kernel split

Times are device events around one layer's forward + backward (allocation of its outputs included, the same for both
forms).  One JSON line per shape: the median, fastest and slowest round of each form in microseconds, their ratio, and
the bytes each form must move with T = one tensor (GN forward: 1 read + 1 write where the sample stays on chip, BN
forward 2 reads + 1 write; backward: GN 2 reads + 1 write at best, BN 4 reads + 1 write).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                       # noqa: E402

from wssdl_bus_amd.networks import _plumbing as P  # noqa: E402

G, EPS_GN, EPS_BN = 8, 1e-5, 1e-3


def shapes(R):
    """(name, samples, rows per sample, C, position-major)"""
    out = []
    for per, C in ((49, 1024), (49, 256), (16, 2048), (16, 512)):
        for pm in (False, True):
            out.append(("head %dx%dx%d %s" % (R, per, C, "pos-major" if pm else "sample-major"), R, per, C, pm))
    out.append(("trunk 8x150000x64 sample-major", 8, 300 * 500, 64, False))
    return out


def byte_model(S, per, C):
    """bytes each form must move per direction, T = the tensor; the small regime reads a sample once when it fits the
    registers, twice (the second time from cache) when it does not -- counted as HBM bytes only once"""
    T = S * per * C * 4
    small = P.groupnorm_plan(S, per, C)[0]
    return {"T_bytes": T, "gn_regime": "small" if small else "large",
            "gn_fwd_T": 2 if small else 3, "gn_bwd_T": 3 if small else 5, "bn_fwd_T": 3, "bn_bwd_T": 5}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=8512)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="substring of the shape names to run")
    a = ap.parse_args()
    if not torch.cuda.is_available() or P.lib() is None:
        sys.exit("groupnorm_bench: needs a GPU and the plumbing library")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, S, per, C, pm in shapes(a.R):
        if a.only not in name:
            continue
        x = torch.randn((S * per, C), device="cuda", generator=g)
        dy = torch.randn((S * per, C), device="cuda", generator=g)
        w, b = torch.rand((C,), device="cuda", generator=g) + 0.5, torch.rand((C,), device="cuda", generator=g) - 0.5
        mask = None                                 # unmasked, a batch norm does not care about the row order
        assert P.groupnorm_usable(x, per, G) and P.usable(x)

        def gn():
            _, mean, rstd = P.groupnorm_forward(x, per, w, b, EPS_GN, G, True, None, pm)
            P.groupnorm_backward(x, dy, per, w, b, mean, rstd, True, None, pm)

        def bn():
            _, stats, _ = P.rowbn_forward(x, w, b, EPS_BN, True, mask, pm)
            P.rowbn_backward(x, dy, w, stats, True, mask, pm)

        for _ in range(a.warmup):
            gn()
            bn()
        torch.cuda.synchronize()
        t_gn, t_bn = [], []
        for _ in range(a.rounds):
            t_gn.append(timed(gn))
            t_bn.append(timed(bn))
        m_gn, m_bn = statistics.median(t_gn), statistics.median(t_bn)
        line = {"shape": name, "rounds": a.rounds,
                "gn_us": [round(m_gn, 1), round(min(t_gn), 1), round(max(t_gn), 1)],
                "bn_us": [round(m_bn, 1), round(min(t_bn), 1), round(max(t_bn), 1)],
                "gn_over_bn": round(m_gn / m_bn, 3)}
        line.update(byte_model(S, per, C))
        line["gn_GBps_fwd_bwd"] = round((line["gn_fwd_T"] + line["gn_bwd_T"]) * line["T_bytes"] / m_gn / 1e3, 1)
        line["bn_GBps_fwd_bwd"] = round((line["bn_fwd_T"] + line["bn_bwd_T"]) * line["T_bytes"] / m_bn / 1e3, 1)
        print(json.dumps(line), flush=True)
        del x, dy


if __name__ == "__main__":
    main()
