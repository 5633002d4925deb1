#!/usr/bin/env python3
"""The image blob of a joint mini-batch: the batched device op (utils.blob.image_batch_blob, wssdl_image_batch_blob)
against the per-image path (utils.blob.image_blob_per_image: the chain of single-image launches that
_get_image_blob_joint runs) on the SAME plan.

    python tools/data_layer_bench.py [--sup 4] [--weak 4] [--rounds 9] [--seconds 1.0] [--step-ms 137] [--out FILE]
    python tools/data_layer_bench.py --kernels DIR    the per-kernel split of both paths: one `rocprofv3 --kernel-trace
                                                      --stats` run of this tool (a fresh child process) writing under DIR

Workload: speckle-like u8 planes with the five sample shapes (291x498, 535x777, 578x738, 594x738, 578x738), a 4 + 4
joint batch at the default 600 / 1000 scales with the reference-default augmentation (rotation, cropping, brightness,
contrast), one seeded plan.  The two paths alternate in one process after a warm-up of each; every round times enough
batches of one path to fill --seconds, with device events around the whole round (host packing, the uploads and the
launches of a batch are inside: this is what a training loop waits for when it asks for the blob), and the figure of
a round is ms per batch.  Reported: median [min, max] over the rounds for each path, the run-to-run spread, the
kernel count of each path at N = 2 and N = 8 (torch.profiler, device kernels only; copies are listed apart), the bytes
the op must move (planes read + blob written) and the fraction of the HBM peak that is at the measured time, and both
times as a share of --step-ms (the ResNet-50 4 + 4 step bench.py measures).  The two blobs are compared bit for bit
before anything is timed.  Prints one JSON line last."""
import argparse
import glob
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(291, 498), (535, 777), (578, 738), (594, 738), (578, 738)]
HBM_PEAK = 8.0e12            # bytes / s, MI355X


def speckle(seed, h, w):
    rs = np.random.RandomState(seed)
    low = rs.uniform(0.2, 1.0, size=(h // 32 + 2, w // 32 + 2))
    mask = np.kron(low, np.ones((32, 32)))[:h, :w]
    return np.clip(rs.rayleigh(40.0, size=(h, w)) * mask, 0, 255).astype(np.uint8)


def make_plan(n_sup, n_weak, seed=3):
    from wssdl_bus_amd.roi_data_layer import minibatch_bus as M
    mk = lambda i: dict(plane=speckle(900 + i, *SHAPES[i % len(SHAPES)]), flipped=bool(i % 2),         # noqa: E731
                        boxes=np.array([[10, 10, 200, 150]], np.uint16), gt_classes=np.array([1], np.int32), birads_diag=1)
    sup, weak = [mk(i) for i in range(n_sup)], [mk(n_sup + i) for i in range(n_weak)]
    return M.plan_minibatch_joint(sup, weak, "Resnet_train", 3, True, rng=np.random.RandomState(seed))


def kernel_count(fn):
    """Device kernels and copies of one call of fn (after one untimed call)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels, copies = {}, 0
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA"):
            if "memcpy" in ev.name.lower() or "copy" in ev.name.lower() and "kernel" not in ev.name.lower():
                copies += 1
            else:
                kernels[ev.name] = kernels.get(ev.name, 0) + 1
    return kernels, copies


def time_round(fn, seconds, per_batch_guess):
    n = max(3, int(seconds * 1e3 / max(per_batch_guess, 1e-3)))
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n, n


def kernels(a):
    out = os.path.abspath(a.kernels)
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "data_layer_bench", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--sup", str(a.sup), "--weak", str(a.weak), "--rounds", "1",
           "--seconds", "0.1", "--no-counts"]
    subprocess.check_call(cmd, timeout=280)
    for f in sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)):
        print("# " + os.path.relpath(f, out))
        with open(f) as fh:
            for line in fh:
                if "image_" in line or line.startswith('"Name"'):
                    print(line.rstrip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sup", type=int, default=4)
    ap.add_argument("--weak", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--step-ms", type=float, default=137.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-counts", action="store_true", help="skip the torch.profiler kernel counts")
    ap.add_argument("--kernels", default=None, help="directory for one rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    if a.kernels:
        return kernels(a)
    from wssdl_bus_amd.utils import blob as B
    plan = make_plan(a.sup, a.weak)
    planes = plan.planes
    batched = lambda: B.image_batch_blob(plan, planes)                  # noqa: E731
    per_image = lambda: B.image_blob_per_image(plan, planes)            # noqa: E731
    assert torch.equal(batched(), per_image()), "the two paths disagree"
    print("blob", [len(planes)] + list(plan.blob_shape) + [3], "bit-equal on both paths", flush=True)
    for f in (batched, per_image):                                      # warm-up: every shape, both paths
        for _ in range(5):
            f()
    guess = {}
    for name, f in (("batched", batched), ("per_image", per_image)):    # calibrate the batch count of a round, twice:
        guess[name], _ = time_round(f, 0.05, 5.0)                       # a handful of batches is dominated by start-up
        guess[name], _ = time_round(f, 0.3, guess[name])
    rounds = {"batched": [], "per_image": []}
    for r in range(a.rounds):
        for name, f in (("batched", batched), ("per_image", per_image)):
            ms, n = time_round(f, 1.05 * a.seconds, guess[name])
            guess[name] = ms                                            # the next round follows this one's rate
            rounds[name].append(ms)
            print("round %d %-9s %8.4f ms / batch (%d batches, %.2f s)" % (r, name, ms, n, ms * n * 1e-3), flush=True)
    counts = {}
    for n_s, n_w in (() if a.no_counts else ((1, 1), (4, 4))):
        p = make_plan(n_s, n_w)
        for name, f in (("batched", lambda: B.image_batch_blob(p, p.planes)), ("per_image", lambda: B.image_blob_per_image(p, p.planes))):
            try:
                k, c = kernel_count(f)
                counts["%s_N%d" % (name, n_s + n_w)] = dict(kernels=sum(k.values()), copies=c, by_name=k)
            except Exception as ex:                                     # the profiler is a convenience, not the product
                counts["%s_N%d" % (name, n_s + n_w)] = dict(error=repr(ex))
    plane_bytes = int(sum(p.size for p in planes))
    blob_bytes = len(planes) * plan.blob_shape[0] * plan.blob_shape[1] * 12
    res = dict(tool="data_layer_bench", n_sup=a.sup, n_weak=a.weak, blob_shape=[len(planes)] + list(plan.blob_shape) + [3],
               rounds=a.rounds, seconds_per_round=a.seconds, plane_bytes=plane_bytes, blob_bytes=blob_bytes, kernel_counts=counts)
    for name, v in rounds.items():
        med, lo, hi = float(np.median(v)), float(min(v)), float(max(v))
        res[name + "_ms"] = dict(median=med, min=lo, max=hi, spread_pct=100.0 * (hi - lo) / med)
        res[name + "_share_of_step_pct"] = 100.0 * med / a.step_ms
    res["speedup"] = res["per_image_ms"]["median"] / res["batched_ms"]["median"]
    res["batched_hbm_fraction"] = (plane_bytes + blob_bytes) / (res["batched_ms"]["median"] * 1e-3) / HBM_PEAK
    res["step_ms"] = a.step_ms
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
