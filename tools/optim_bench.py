"""One optimiser step on the ResNet-50 network's own parameter list: the three one-launch reference optimisers
(csrc/plumbing/optim.hip through fast_rcnn/optim.py), torch.optim.Adam(fused=True) -- what SolverWrapper(opt=None)
runs -- and the per-parameter chain of torch ops (WSSDL_TORCH_OPTIM=1) the kernel replaces.

    python tools/optim_bench.py [--depth 50] [--rounds 15] [--steps 20] [--warmup 3]

All forms run in one process, alternating: a round times `--steps` back-to-back steps of each form in turn (device
events around the window, a synchronise before and after), and the rounds repeat.  Per form: the median over the
rounds of the time per step, and the spread (max - min over the rounds) that a difference has to exceed.  Gradients
have their parameters' shapes and layouts and stay allocated, so the times are the update's alone.  Printed next to
each time: the bytes the form must move (Adam: p, g, m, v read and p, m, v written, 7 floats per element; AMSGrad 9;
Nesterov 5), the fraction of the HBM peak that makes, and for the chain its launches per step.  One JSON line at the
end.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                                   # noqa: E402

from wssdl_bus_amd.fast_rcnn import optim as O                  # noqa: E402
from wssdl_bus_amd.networks.factory_bus import get_network      # noqa: E402

HBM_PEAK = 8.0e12                                   # bytes / s, MI355X specification
FLOATS = {"adam": 7, "amsgrad": 9, "sgd": 5, "torch_fused_adam": 7, "chain_adam": 7}
# torch ops per parameter of ReferenceOptimizer._step_torch: sub mul add_ | mul sub mul add_ | sqrt add mul div sub_
CHAIN_OPS = {"adam": 12, "amsgrad": 13, "sgd": 7}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs a GPU"
    torch.manual_seed(0)
    net = get_network("Resnet_train", a.depth).cuda().to(memory_format=torch.channels_last)
    params = [p for p in net.parameters() if p.requires_grad]
    assert O.hip_usable(params), "the one-launch kernel does not take this parameter list"
    n = sum(p.numel() for p in params)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2          # preserve_format: the parameter's own layout
    forms = {}
    for kind in ("adam", "amsgrad", "sgd"):
        forms[kind] = O.ReferenceOptimizer(params, kind, 5e-4, eps=0.1, momentum=0.9).step
    forms["torch_fused_adam"] = torch.optim.Adam(params, lr=5e-4, eps=0.1, fused=True).step
    chain = O.ReferenceOptimizer(params, "adam", 5e-4, eps=0.1)

    def chain_step():
        os.environ["WSSDL_TORCH_OPTIM"] = "1"
        try:
            chain.step()
        finally:
            del os.environ["WSSDL_TORCH_OPTIM"]
    forms["chain_adam"] = chain_step

    def window(step, k):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(k):
            step()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3 / k      # us per step

    for name, step in forms.items():
        window(step, a.warmup)
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, step in forms.items():
            times[name].append(window(step, a.steps if name != "chain_adam" else max(1, a.steps // 10)))
    assert O.TABLE_BUILDS[0] == 3, O.TABLE_BUILDS          # one chunk table per one-launch optimiser, built once
    out = {"depth": a.depth, "params": len(params), "floats": n, "rounds": a.rounds, "steps_per_window": a.steps,
           "forms": {}}
    print("ResNet-%d: %d parameters, %d floats (%.1f MB)" % (a.depth, len(params), n, 4e-6 * n))
    for name, ts in times.items():
        med, spread = statistics.median(ts), max(ts) - min(ts)
        nbytes = 4 * n * FLOATS[name]
        row = {"us_per_step_median": round(med, 2), "us_spread": round(spread, 2), "us_min": round(min(ts), 2),
               "bytes": nbytes, "hbm_peak_fraction": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        if name == "chain_adam":
            row["launches_per_step"] = CHAIN_OPS["adam"] * len(params)
        out["forms"][name] = row
        print("%-18s %9.1f us/step  (spread %7.1f, min %9.1f)  %7.1f MB  %5.1f %% of HBM peak%s"
              % (name, med, spread, min(ts), nbytes * 1e-6, 100 * row["hbm_peak_fraction"],
                 "  %d launches" % row["launches_per_step"] if "launches_per_step" in row else ""))
    f, t = out["forms"]["adam"], out["forms"]["torch_fused_adam"]
    out["adam_minus_torch_fused_us"] = round(f["us_per_step_median"] - t["us_per_step_median"], 2)
    out["expectation_met"] = f["us_per_step_median"] <= t["us_per_step_median"] + max(f["us_spread"], t["us_spread"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
