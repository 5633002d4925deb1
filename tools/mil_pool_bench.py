"""The fused MIL term (mil/core.py: mil_loss_device, forward + backward under autograd) at the weak step's shape --
2 bags x 2000 rows, K = 3 -- timed three ways:

  (a) the reference's own pairs, [mass_max, mal_max] (the alternating weak step) and [mal_max, mal_max] (the combined
      step's weak half), on this tree against the same calls on another build of the package (`--parent DIR`, a
      directory that holds a built `wssdl_bus_amd` of the parent commit);
  (b) [disc_max, mean_ben] on the fused op against the unfused route for the same pair (get_bag_logit_device, then
      torch's cross-entropy and mean: train_bus.mil_loss with cfg.FUSED_LOSS = False);
  (c) the device kernels one forward + backward of each of those launches, from torch.profiler's device activity in a
      process of its own (memory copies and sets left out).

    python tools/mil_pool_bench.py --parent DIR [--rounds 7] [--calls 3000] [--warmup 2]

Every process times its sides alternating: a round times one window of each side in turn, a window being `--calls`
back-to-back forward + backward calls between two device events, after `--warmup` windows of each.  Per side: the median
over the rounds and the spread (max - min).  With `--parent` the processes of (a) run one after another, each timing
the same two sides -- parent, this tree, parent again -- so that the difference between the two parent runs is there to judge a difference by: this tree's
median counts as no worse when it exceeds the smaller of the parent's two medians by no more than that spread.  One
JSON line at the end.  `--side-of ROOT` is what the children run: the sides of the package under ROOT, JSON only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAGS, ROWS, K = 2, 2000, 3


def sides_of(root, which, count_launches, rounds, calls, warmup):
    sys.path.insert(0, root)
    import torch
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.mil import core as M
    assert torch.cuda.is_available(), "mil_pool_bench needs a GPU"
    assert os.path.abspath(M.__file__).startswith(os.path.abspath(root)), (M.__file__, root)
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn((BAGS * ROWS, K), generator=g) * 2.0).cuda().requires_grad_(True)
    col = torch.repeat_interleave(torch.arange(BAGS), ROWS).float().cuda()
    labels = torch.tensor([1, 2], dtype=torch.int32).cuda()
    step = 4100

    def call(funcs, fused=True):
        def fn():
            cfg.FUSED_LOSS = fused
            logits.grad = None
            loss = T.mil_loss(logits, col, labels, BAGS, step, funcs)
            loss.backward()
            return loss
        return fn

    sides = {"alternating [mass_max, mal_max]": call([M.get_mass_max_logit, M.get_mal_max_logit]),
             "combined [mal_max, mal_max]": call([M.get_mal_max_logit, M.get_mal_max_logit])}
    if "b" in which and hasattr(M, "get_mean_ben_logit"):
        pair = [M.get_disc_max_logit, M.get_mean_ben_logit]
        sides["[disc_max, mean_ben] fused"] = call(pair)
        sides["[disc_max, mean_ben] unfused"] = call(pair, fused=False)
    if "a" not in which:
        sides = {k: v for k, v in sides.items() if k.startswith("[disc")}
    out = {"root": root, "sides": {}}

    if count_launches:
        from torch.profiler import ProfilerActivity, profile
        for name, fn in sides.items():
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
            names = [s for s in names if "memcpy" not in s.lower() and "memset" not in s.lower()]
            out["sides"][name] = {"device_kernels": len(names), "of_this_library": sum("mil_" in s for s in names)}
        return out

    def window(fn, k):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(k):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3 / k                  # us per forward + backward

    for fn in sides.values():
        for _ in range(warmup):
            window(fn, calls)
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(window(fn, calls))
    for name, ts in times.items():
        out["sides"][name] = {"unit": "us per forward + backward", "median": round(statistics.median(ts), 3),
                              "spread": round(max(ts) - min(ts), 3), "min": round(min(ts), 3)}
    return out


def child(root, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--side-of", root] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("a child of mil_pool_bench ended with status %d: %s" % (r.returncode, " ".join(cmd)))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory holding a built wssdl_bus_amd of the parent commit")
    ap.add_argument("--side-of", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--which", default="ab", help=argparse.SUPPRESS)
    ap.add_argument("--count-launches", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.side_of:
        print(json.dumps(sides_of(a.side_of, a.which, a.count_launches, a.rounds, a.calls, a.warmup)))
        return
    knobs = ["--which", "a", "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup", str(a.warmup)]
    runs = []
    if a.parent:
        runs.append(("parent, first run", child(os.path.abspath(a.parent), knobs)))
    runs.append(("this tree", child(HERE, knobs)))
    if a.parent:
        runs.append(("parent, second run", child(os.path.abspath(a.parent), knobs)))
    new_pair = child(HERE, ["--which", "b"] + knobs[2:])
    runs.append(("this tree, the new pair", new_pair))
    counts = [("this tree", child(HERE, ["--count-launches"]))]
    if a.parent:
        counts.append(("parent", child(os.path.abspath(a.parent), ["--count-launches"])))

    print("fused MIL term, forward + backward, %d bags x %d rows, K = %d; %d rounds of %d calls after %d warm-up windows"
          % (BAGS, ROWS, K, a.rounds, a.calls, a.warmup))
    for title, r in runs:
        print(title)
        for name, s in r["sides"].items():
            print("  %-36s %9.3f us  (spread %7.3f, min %9.3f)" % (name, s["median"], s["spread"], s["min"]))
    out = {"bags": BAGS, "rows_per_bag": ROWS, "K": K, "rounds": a.rounds, "calls_per_window": a.calls,
           "runs": {t: r["sides"] for t, r in runs}, "launches": {t: r["sides"] for t, r in counts}}
    if a.parent:
        first, mine, second = runs[0][1]["sides"], runs[1][1]["sides"], runs[2][1]["sides"]
        out["a"] = {}
        print("(a) this tree against the parent; allowed: the smaller of the parent's two medians + |first - second|")
        for name in first:
            between = abs(first[name]["median"] - second[name]["median"])
            worse = mine[name]["median"] - min(first[name]["median"], second[name]["median"])
            ok = worse <= between
            out["a"][name] = {"parent_first": first[name]["median"], "parent_second": second[name]["median"],
                              "spread_between_parent_runs": round(between, 3), "this_tree": mine[name]["median"],
                              "this_tree_minus_parent_best": round(worse, 3), "no_worse": ok}
            print("  %-36s parent %9.3f / %9.3f (between runs %7.3f), this tree %9.3f (%+.3f): %s"
                  % (name, first[name]["median"], second[name]["median"], between, mine[name]["median"], worse,
                     "no worse" if ok else "WORSE than the spread allows"))
    mine = new_pair["sides"]
    if "[disc_max, mean_ben] fused" in mine:
        f, u = mine["[disc_max, mean_ben] fused"]["median"], mine["[disc_max, mean_ben] unfused"]["median"]
        out["b"] = {"fused": f, "unfused": u, "unfused_over_fused": round(u / f, 3)}
        print("(b) [disc_max, mean_ben]: fused %.3f us, unfused %.3f us: unfused / fused = %.3f" % (f, u, u / f))
    print("(c) device kernels of one forward + backward (torch.profiler, a process of its own)")
    for title, r in counts:
        for name, s in r["sides"].items():
            print("  %-10s %-36s %3d kernels, %d of them this library's" % (title, name, s["device_kernels"], s["of_this_library"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
