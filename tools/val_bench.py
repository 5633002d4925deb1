"""The validation pass (SolverWrapper.validate, fast_rcnn/train_bus.py) against what a user had to write before it,
on ResNet-50 with the combined wiring and 8 synthetic 600 x 1000 validation images (wssdl_bus_amd/synthetic.py):

  (a) validation pass   validate() on one blob of 8 images -- one eval forward, one per-image loss launch, one MIL
                        call, one read-back -- against the same 8 images as 8 single-image eval forwards, each
                        followed by supervised_loss and a .cpu() read-back of its four terms;
  (b) loss op alone     loss_op.multi_task_loss_per_image for N = 8 on the layers of that forward against 8 calls of
                        loss_op.multi_task_loss on per-image slices (sliced once, outside the timed window).

    python tools/val_bench.py [--images 8] [--rounds 7] [--passes 10] [--calls 5000] [--warmup 2]

Both sides of a comparison run in one process, alternating: a round times one window of each side in turn and the
rounds repeat.  A window of (a) is `--passes` passes timed with the host clock between two device synchronises (a
pass ends in its own read-back); a window of (b) is `--calls` back-to-back calls between device events.  Every side
is warmed up with `--warmup` windows first.  Per side: the median over the rounds and the spread (max - min) that a
difference has to exceed.  The switches are the benchmark's (device sampler, fused RPN softmax).  One JSON line at the
end.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                                   # noqa: E402

from wssdl_bus_amd import synthetic                            # noqa: E402
from wssdl_bus_amd.fast_rcnn import train_bus as T              # noqa: E402
from wssdl_bus_amd.fast_rcnn.config import cfg                  # noqa: E402
from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss, multi_task_loss_per_image   # noqa: E402
from wssdl_bus_amd.networks.factory_bus import get_network      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "val_bench needs a GPU"
    n = a.images
    cfg.SAMPLING_RNG = "device"
    cfg.FUSED_RPN_SOFTMAX = True
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = n, 0
    torch.manual_seed(0)
    net = get_network("Resnet_train", a.depth).cuda().to(memory_format=torch.channels_last)
    net.train()
    solver = T.SolverWrapper(net)
    blobs = synthetic.make_batch(n, 0, a.height, a.width, seed=7)
    singles = [{k: v[i:i + 1].contiguous() for k, v in blobs.items()} for i in range(n)]

    def batched_pass():
        return solver.validate([blobs], feed_schedule=False)

    def single_image_pass():
        rows = []
        was, ims = net.training, cfg.TRAIN.IMS_PER_BATCH
        net.eval()
        cfg.TRAIN.IMS_PER_BATCH = 1
        try:
            with torch.no_grad():
                for b in singles:
                    layers = net(b["data"], b["im_info"], b["gt_boxes"], b["num_gt_boxes"], is_training=False, is_ws=False)
                    l = T.supervised_loss(layers, [], 1)
                    rows.append(torch.stack([l[k] for k in T.VAL_TERMS[1:5]]).cpu())
        finally:
            cfg.TRAIN.IMS_PER_BATCH = ims
            net.train(was)
        return torch.stack(rows)

    def host_window(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k               # ms per pass

    # the layers of one 8-image eval forward, for (b)
    net.eval()
    with torch.no_grad():
        layers = dict(net(blobs["data"], blobs["im_info"], blobs["gt_boxes"], blobs["num_gt_boxes"], is_training=False,
                          is_ws=False))
    net.train()
    args8 = (layers["rpn_cls_score"], layers["rpn_bbox_pred"], layers["cls_score"], layers["bbox_pred"], layers["rpn-data"],
             layers["roi-data"])
    rois = layers["roi-data"][0]
    sliced = []
    for i in range(n):
        r = (rois[:, 0] == i).nonzero().squeeze(1)
        sliced.append((layers["rpn_cls_score"][i:i + 1].contiguous(), layers["rpn_bbox_pred"][i:i + 1].contiguous(),
                       layers["cls_score"][r].contiguous(), layers["bbox_pred"][r].contiguous(),
                       tuple(t[i:i + 1].contiguous() for t in layers["rpn-data"]),
                       tuple(t[r].contiguous() for t in layers["roi-data"])))
    N, H, W, A2 = layers["rpn_cls_score"].shape
    K = layers["cls_score"].shape[1]
    n_rows = int(layers["roi-data"][1].numel())

    def per_image_op():
        with torch.no_grad():
            return multi_task_loss_per_image(*args8, n)

    def sliced_ops():
        with torch.no_grad():
            return [multi_task_loss(*s, 1) for s in sliced]

    def event_window(fn, k):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(k):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3 / k                  # us per call (of all images)

    # same numbers on both sides before anything is timed
    got = per_image_op()[0]
    want = torch.stack(sliced_ops())
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-7, equal_nan=True), (got, want)

    sides_a = {"validate_%d_per_forward" % n: batched_pass, "%d_single_image_forwards" % n: single_image_pass}
    sides_b = {"per_image_op_N%d" % n: per_image_op, "%d_sliced_batch_ops" % n: sliced_ops}
    for name, fn in sides_a.items():
        host_window(fn, a.warmup)
    for name, fn in sides_b.items():
        event_window(fn, a.warmup * 50)
    times = {name: [] for name in list(sides_a) + list(sides_b)}
    for _ in range(a.rounds):
        for name, fn in sides_a.items():
            times[name].append(host_window(fn, a.passes))
        for name, fn in sides_b.items():
            times[name].append(event_window(fn, a.calls))

    # bytes the per-image op reads: scores 2A, labels A, box pred + 3 target tensors 16A floats per cell; per row K
    # scores, 1 label, 16K box floats, and the image column once per image's workgroup
    op_bytes = 4 * (N * H * W * (A2 // 2) * 19 + n_rows * (17 * K + 1) + n * n_rows)
    out = {"depth": a.depth, "images": n, "image_size": [a.height, a.width], "score_map": [N, H, W, A2 // 2],
           "roi_rows": n_rows, "rounds": a.rounds, "passes_per_window": a.passes, "calls_per_window": a.calls,
           "per_image_op_bytes": op_bytes, "sides": {}}
    print("ResNet-%d combined wiring, %d images of %d x %d: score map %d x %d x %d anchors, %d RoI rows"
          % (a.depth, n, a.height, a.width, H, W, A2 // 2, n_rows))
    for group, unit in ((sides_a, "ms/pass"), (sides_b, "us/call")):
        for name in group:
            ts = times[name]
            med, spread = statistics.median(ts), max(ts) - min(ts)
            out["sides"][name] = {"unit": unit, "median": round(med, 3), "spread": round(spread, 3), "min": round(min(ts), 3)}
            print("%-28s %10.3f %s  (spread %8.3f, min %10.3f)" % (name, med, unit, spread, min(ts)))
    names_a, names_b = list(sides_a), list(sides_b)
    out["a_speedup"] = round(out["sides"][names_a[1]]["median"] / out["sides"][names_a[0]]["median"], 3)
    out["b_speedup"] = round(out["sides"][names_b[1]]["median"] / out["sides"][names_b[0]]["median"], 3)
    print("(a) single-image forwards / validate = %.3f;  (b) sliced batch ops / per-image op = %.3f"
          % (out["a_speedup"], out["b_speedup"]))
    print("per-image op reads %.2f MB per call" % (op_bytes * 1e-6))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
