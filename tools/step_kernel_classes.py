"""Kernel time by class for the timed steps of a bench.py run traced with
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 5 --warmup 3 --no-cpu-baseline`
(tools/step_breakdown.sh): the window between the last five roi_pool_bwd launches = 4 steps.

    python tools/step_kernel_classes.py DIR [TAG] [TOPN] [SUBSTRING ...]

Each SUBSTRING adds a COUNT line: calls, ms per step and mean us per launch of the kernels whose name contains it.
"""
import csv
import glob
import json
import os
import sys


def klass(name):
    if name.startswith("Cijk_") or "gemm" in name.lower() and "igemm" not in name:
        return "gemm (hipBLASLt/rocBLAS)"
    if "rowbn_" in name:
        return "rowbn"
    if "at::native" in name:
        return "torch elementwise/reduce/index"
    if "tap_" in name:
        return "tap kernels"
    return "other"


def main():
    d, tag = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""
    topn = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    f = max(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "roi_pool_bwd" in r["Kernel_Name"]]
    start, end = int(rows[idx[-5]]["Start_Timestamp"]), int(rows[idx[-1]]["Start_Timestamp"])
    sel = [r for r in rows if start <= int(r["Start_Timestamp"]) < end]
    steps = 4.0
    agg, cls = {}, {}
    for r in sel:
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        a = agg.setdefault(r["Kernel_Name"], [0.0, 0])
        a[0] += ms
        a[1] += 1
        c = cls.setdefault(klass(r["Kernel_Name"]), [0.0, 0])
        c[0] += ms
        c[1] += 1
    print(json.dumps({"tag": tag, "kernel_ms_per_step": round(sum(v[0] for v in agg.values()) / steps, 2),
                      "wall_ms_per_step": round((end - start) / 1e6 / steps, 2),
                      "launches_per_step": len(sel) / steps,
                      "classes_ms_per_step": {k: round(v[0] / steps, 2) for k, v in cls.items()},
                      "classes_launches_per_step": {k: v[1] / steps for k, v in cls.items()}}))
    fmt = "%7.3f ms/step calls/step=%6.1f avg_us=%8.1f %s"
    for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])[:topn]:
        print(fmt % (v[0] / steps, v[1] / steps, v[0] / v[1] * 1e3, k[:120]))
    for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0]):
        if "rowbn_" in k or "CUDAFunctor_add" in k:
            print("KERNEL " + fmt % (v[0] / steps, v[1] / steps, v[0] / v[1] * 1e3, k[:120]))
    for sub in sys.argv[4:]:
        ms = sum(v[0] for k, v in agg.items() if sub in k)
        n = sum(v[1] for k, v in agg.items() if sub in k)
        print("COUNT %-60s calls/step=%6.1f ms/step=%7.3f avg_us=%8.1f" % (sub[:60], n / steps, ms / steps,
                                                                           ms / n * 1e3 if n else 0.0))


if __name__ == "__main__":
    main()
