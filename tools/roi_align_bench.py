"""RoIAlign against RoI max pooling at the training size: feature map [8,38,63,1024], the committed 8512-RoI set
(profiles/roofline_rois_r8512.npy), 7 x 7 bins, S = 2, aligned.

    python tools/roi_align_bench.py [--rounds 9] [--calls 5] [--warmup 2] [--no-step] [--only align_backward]

Every form runs in one process, alternating: a round times `--calls` back-to-back calls of each form in turn (device
events around the window, a synchronise before and after), and the rounds repeat.  Per form: the median over the rounds
of the time per call, the spread (max - min over the rounds), the bytes the form must move and the fraction of the 8 TB/s
HBM peak that makes.  The forms:

    align_tables / align_forward / align_prepare / align_backward     csrc/roi_align.hip (prepare = the backward's lists)
    max_forward / max_prepare / max_backward                          the training path of RoI max pooling as it stands
                                                                      (1-byte arg-max pair; forward = window table + pooling)

Must-move bytes: the forwards read the feature map once and write top (max: and one arg-max byte per element); the
backwards read top_diff (max: and the arg-max bytes) and write bottom_diff; tables and lists are counted with the steps
that write them.  The yardstick of the align pair is the max pair of the same run.

Then the align forward against a chunked torch einsum of the dense form top_r = Ay . F_n . Ax^T / S^2 on the first 256
RoIs (Ay, Ax built from the device tables; the gather of F_n is part of what torch has to do), with the largest
difference between the two; and, unless --no-step, the ResNet-50 4 + 4 step of tools/step_probe.py under both modes,
alternating.  --only NAME runs that one form alone (for a counter pass).  One JSON line at the end.
"""
import argparse
import contextlib
import io
import json
import os
import re
import runpy
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402

from wssdl_bus_amd.fast_rcnn.config import cfg                  # noqa: E402
from wssdl_bus_amd.roi_pooling_layer import roi_align_op as A   # noqa: E402
from wssdl_bus_amd.roi_pooling_layer import roi_pooling_op as M  # noqa: E402

HBM_PEAK = 8.0e12                                   # bytes / s, MI355X specification
SHAPE, PH, PW, SCALE, S, ALIGNED = (8, 38, 63, 1024), 7, 7, 1.0 / 16, 2, True


def window(fn, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(k):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / k          # us per call


def dense_axes(t, g, rows, L, axis):
    """Ay [rows,P,L] (axis 'y') or Ax from the device tables: every entry's two weights scattered onto its two cells."""
    P = g.ph if axis == 'y' else g.pw
    A_ = torch.zeros((rows, P, L), dtype=torch.float32, device=t[axis + 'lo'].device)
    for idx, w in ((axis + 'lo', axis + 'h'), (axis + 'hi', axis + 'l')):
        for i in range(g.S):
            A_.scatter_add_(2, t[idx][:rows, :, i:i + 1].long(), t[w][:rows, :, i:i + 1])
    return A_


def device_tables(buf, g):
    words, out, at = buf.view(torch.int32), {}, 0
    for name in A.TABLE_NAMES:
        shp = (g.R, 5) if name == 'win' else (g.R, g.ph if name[0] == 'y' else g.pw, g.S)
        n = int(np.prod(shp))
        a = words[at:at + n].view(shp)
        out[name] = a.view(torch.float32) if name[1:] in ('h', 'l') else a
        at += n
    return out


def step_probe(mode):
    """tools/step_probe.py 4 4 50 under cfg.ROI_POOL_MODE = mode: (forward, backward) ms of its last iteration."""
    old, argv = cfg.ROI_POOL_MODE, sys.argv
    cfg.ROI_POOL_MODE, sys.argv = mode, ["step_probe.py", "4", "4", "50"]
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            runpy.run_path(os.path.join(ROOT, "tools", "step_probe.py"), run_name="__main__")
    finally:
        cfg.ROI_POOL_MODE, sys.argv = old, argv
    rows = re.findall(r"iter \d+ R (\d+) fwd ([\d.]+) loss ([\d.]+) bwd ([\d.]+) opt ([\d.]+) ms", out.getvalue())
    r, fwd, loss, bwd, opt = rows[-1]
    return dict(R=int(r), fwd_ms=float(fwd), loss_ms=float(loss), bwd_ms=float(bwd), opt_ms=float(opt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "roi_align_bench needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    rois = torch.from_numpy(np.load(os.path.join(ROOT, "profiles", "roofline_rois_r8512.npy"))).to(dev)
    data = torch.randn(SHAPE, device=dev)
    R = rois.shape[0]
    grad = torch.randn((R, PH, PW, SHAPE[3]), device=dev)
    g = A._Geom(SHAPE, rois, PH, PW, SCALE, S, ALIGNED)
    cfg.ROI_POOL_ANNOUNCE_BWD_FORM = False

    tables, nb = A._tables(g, rois)
    ws, nws = A._prepare(g, tables, nb)
    plan = M.prepare_backward(SHAPE, rois, PH, PW, SCALE)
    _, arg8 = M.roi_pool_compact(data, rois, PH, PW, SCALE)
    forms = {
        "align_tables": lambda: A._tables(g, rois),
        "align_forward": lambda: A._forward(g, data, tables, nb),
        "align_prepare": lambda: A._prepare(g, tables, nb),
        "align_backward": lambda: A._backward(g, grad, tables, nb, ws, nws),
        "max_forward": lambda: M.roi_pool_compact(data, rois, PH, PW, SCALE),
        "max_prepare": lambda: M.prepare_backward(SHAPE, rois, PH, PW, SCALE),
        "max_backward": lambda: M.roi_pool_grad_compact(SHAPE, rois, arg8, grad, PH, PW, SCALE, plan=plan),
    }
    if a.only:
        for _ in range(a.warmup + a.calls):
            forms[a.only]()
        torch.cuda.synchronize()
        print("ran %s %d times" % (a.only, a.warmup + a.calls))
        return
    fmap, top = 4 * int(np.prod(SHAPE)), 4 * grad.numel()
    nbytes = {"align_tables": 20 * R + nb, "align_forward": fmap + top + nb, "align_prepare": nb + nws,
              "align_backward": top + fmap + nb + nws, "max_forward": fmap + top + top // 4, "max_prepare": 20 * R + plan.nbytes,
              "max_backward": top + top // 4 + fmap + plan.nbytes}
    for fn in forms.values():
        window(fn, a.warmup)
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            times[name].append(window(fn, a.calls))
    M.check_flags()
    out = {"shape": list(SHAPE), "R": R, "pooled": [PH, PW], "sampling": S, "aligned": ALIGNED, "rounds": a.rounds,
           "calls_per_window": a.calls, "max_backward_form": plan.variant, "forms": {}}
    print("feature map %s, %d RoIs, %d x %d bins, S = %d: top is %.2f GB" % (SHAPE, R, PH, PW, S, top * 1e-9))
    print("max backward: " + plan.variant)
    for name, ts in times.items():
        med, spread = statistics.median(ts), max(ts) - min(ts)
        row = {"us_median": round(med, 1), "us_spread": round(spread, 1), "us_min": round(min(ts), 1), "bytes": nbytes[name],
               "hbm_peak_fraction": round(nbytes[name] / (med * 1e-6) / HBM_PEAK, 4)}
        out["forms"][name] = row
        print("%-15s %9.1f us/call  (spread %7.1f, min %9.1f)  %8.1f MB  %5.1f %% of HBM peak"
              % (name, med, spread, min(ts), nbytes[name] * 1e-6, 100 * row["hbm_peak_fraction"]))
    f = out["forms"]
    pair = lambda k: f[k + "_forward"]["us_median"] + f[k + "_backward"]["us_median"]
    out["align_pair_us"], out["max_pair_us"] = round(pair("align"), 1), round(pair("max"), 1)
    out["align_over_max"] = round(pair("align") / pair("max"), 3)
    print("pair (forward + backward): align %.1f us, max %.1f us, ratio %.2f" % (pair("align"), pair("max"), out["align_over_max"]))

    # the dense separable form in torch on the first 256 RoIs
    rows, chunk = 256, 64
    sub = rois[:rows].contiguous()
    gs = A._Geom(SHAPE, sub, PH, PW, SCALE, S, ALIGNED)
    tb, nbs = A._tables(gs, sub)
    t = device_tables(tb[:nbs], gs)
    Ay, Ax = dense_axes(t, gs, rows, SHAPE[1], 'y'), dense_axes(t, gs, rows, SHAPE[2], 'x')
    img = t['win'][:, 0].long().clamp(min=0)

    def einsum_form():
        parts = [torch.einsum('rph,rhwc,rqw->rpqc', Ay[k:k + chunk], data[img[k:k + chunk]], Ax[k:k + chunk])
                 for k in range(0, rows, chunk)]
        return torch.cat(parts) / (S * S)

    kernel_form = lambda: A._forward(gs, data, tb, nbs)
    diff = float((einsum_form() - kernel_form()).abs().max())
    pairs = {"einsum": einsum_form, "kernel": kernel_form}
    for fn in pairs.values():
        window(fn, a.warmup)
    et = {k: [] for k in pairs}
    for _ in range(a.rounds):
        for k, fn in pairs.items():
            et[k].append(window(fn, a.calls))
    out["first_256"] = {"einsum_us_median": round(statistics.median(et["einsum"]), 1),
                        "kernel_us_median": round(statistics.median(et["kernel"]), 1), "max_abs_difference": diff}
    print("first %d RoIs: torch einsum (chunks of %d) %.1f us, align forward %.1f us, largest difference %.2e"
          % (rows, chunk, out["first_256"]["einsum_us_median"], out["first_256"]["kernel_us_median"], diff))
    del Ay, Ax, grad, arg8, data
    torch.cuda.empty_cache()

    if not a.no_step:
        steps = {"max": [], "align": []}
        for mode in ("max", "align", "max", "align"):
            steps[mode].append(step_probe(mode))
            print("ResNet-50 4 + 4 step, ROI_POOL_MODE = %-5s: R %d, forward %.1f ms, backward %.1f ms, optimiser %.1f ms"
                  % (mode, steps[mode][-1]["R"], steps[mode][-1]["fwd_ms"], steps[mode][-1]["bwd_ms"], steps[mode][-1]["opt_ms"]))
        out["resnet50_4_4_step"] = steps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
