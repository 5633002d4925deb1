"""The detection half of the validation pass (fast_rcnn/val_detect.py, SolverWrapper.validate(..., gt_roidb=...)) next
to what it replaces, on ResNet-50 with the combined wiring, 8 images of 600 x 1000 and 128 sampled RoIs each, K = 3:

  (a) decode step      wssdl_decode_detections (one launch) against the chain of torch ops im_detect_batch runs for the
                       same step (restated here on the same tensors: the sampled RoIs, bbox_pred and im_info of one
                       eval forward), with the number of device kernels each side launches;
  (b) validation pass  validate([blob], gt_roidb=gt) -- one forward, losses, detections and their scores -- against
                       validate([blob]) followed by eval_batch.evaluate_images over the same 8 images, which runs a
                       second forward through the test wiring.  The images are prepared once, outside the timed
                       windows, for both sides (evaluate_images' get_test_blobs is handed the prepared blob), and the
                       forwards of one pass are counted on each side.

    python tools/val_detect_bench.py [--images 8] [--rounds 7] [--passes 10] [--calls 2000] [--warmup 2]

Both sides of a comparison run in one process, alternating; per side the median over the rounds and the spread
(max - min).  A window of (a) is `--calls` back-to-back calls between device events, a window of (b) `--passes` passes
under the host clock between two device synchronises.  Kernel counts come from torch.profiler's device activity where
this build has it; the count of tensor-writing ATen calls (a lower bound of the launches) is printed either way.  There
is no speed claim in this tool's purpose: what it documents is one forward instead of two and one launch instead of a
chain.  One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                              # noqa: E402
import torch                                                   # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode     # noqa: E402

from wssdl_bus_amd import _lib, synthetic                       # noqa: E402
from wssdl_bus_amd.fast_rcnn import eval_batch, train_bus as T   # noqa: E402
from wssdl_bus_amd.fast_rcnn.bbox_transform import bbox_transform_inv   # noqa: E402
from wssdl_bus_amd.fast_rcnn.config import cfg                  # noqa: E402
from wssdl_bus_amd.fast_rcnn.val_detect import decode_detections_device   # noqa: E402
from wssdl_bus_amd.networks.factory_bus import get_network      # noqa: E402


def torch_chain(rois, deltas, im_info, n):
    """im_detect_batch's decode / clip (fast_rcnn/detect_batch.py) on given tensors"""
    info = _lib.to_device(im_info, torch.float64, rois.device)
    img = rois[:, 0].to(torch.int64).clamp_(0, n - 1)
    scale = info[:, 2].to(torch.float32)
    boxes = rois[:, 1:5] * torch.reciprocal(scale)[img].unsqueeze(1)
    pred = bbox_transform_inv(boxes, deltas)
    xmax = (info[:, 1] / info[:, 2] - 1.0).to(torch.float32)[img].unsqueeze(1)
    ymax = (info[:, 0] / info[:, 2] - 1.0).to(torch.float32)[img].unsqueeze(1)
    pred[:, 0::4] = pred[:, 0::4].clamp_min(0)
    pred[:, 1::4] = pred[:, 1::4].clamp_min(0)
    pred[:, 2::4] = torch.minimum(pred[:, 2::4], xmax)
    pred[:, 3::4] = torch.minimum(pred[:, 3::4], ymax)
    return pred


class _WritingOps(TorchDispatchMode):
    """counts the ATen calls that write a tensor: everything but views and allocations"""

    def __init__(self):
        super().__init__()
        self.count = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        view = any(r.alias_info is not None and not r.alias_info.is_write for r in func._schema.returns)
        if not view and ".empty" not in name and "detach" not in name:
            self.count += 1
        return func(*args, **(kwargs or {}))


def writing_ops(fn):
    with _WritingOps() as m:
        fn()
    return m.count


def device_kernels(fn):
    """device kernels of one call from torch.profiler (memory copies and sets left out), or None and the reason"""
    try:
        from torch.profiler import ProfilerActivity, profile, supported_activities
        if ProfilerActivity.CUDA not in supported_activities():
            return None, "this build's profiler has no device activity"
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        names = [s for s in names if "memcpy" not in s.lower() and "memset" not in s.lower()]
        return len(names), sorted(set(names))
    except Exception as e:                                        # noqa: BLE001 (a count that is not taken is reported as such)
        return None, "%s: %s" % (type(e).__name__, e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "val_detect_bench needs a GPU"
    n = a.images
    cfg.SAMPLING_RNG = "device"
    cfg.FUSED_RPN_SOFTMAX = True
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = n, 0
    torch.manual_seed(0)
    net = get_network("Resnet_train", a.depth).cuda().to(memory_format=torch.channels_last)
    net.train()
    solver = T.SolverWrapper(net)
    blobs = synthetic.make_batch(n, 0, a.height, a.width, seed=7)
    gtb, ng, info_h = blobs["gt_boxes"].cpu().numpy(), blobs["num_gt_boxes"].cpu().numpy(), blobs["im_info"].cpu().numpy()
    gt = [{"boxes": gtb[i, :ng[i], :4] / info_h[i, 2], "gt_classes": gtb[i, :ng[i], 4].astype(np.int32)} for i in range(n)]
    forwards = [0]
    net.register_forward_pre_hook(lambda m, args: forwards.__setitem__(0, forwards[0] + 1))

    # ---- (a): the tensors of one eval forward
    net.eval()
    with torch.no_grad():
        layers = dict(net(blobs["data"], blobs["im_info"], blobs["gt_boxes"], blobs["num_gt_boxes"], is_training=False,
                          is_ws=False))
    net.train()
    rois = layers["roi-data"][0].contiguous()
    R = int(rois.shape[0])
    deltas = layers["bbox_pred"][:R].contiguous()
    info = blobs["im_info"]
    K = int(deltas.shape[1]) // 4

    def decode_op():
        return decode_detections_device(rois, deltas, info, n)

    def chain():
        with torch.no_grad():
            return torch_chain(rois, deltas, info, n)
    live = (rois[:, 0] >= 0) & (rois[:, 0] < n)
    got, want = decode_op()[live], chain()[live]
    worst = float((got - want).abs().max())
    assert worst <= 1e-2, worst                                   # the chain multiplies by a reciprocal: last-bit differences
    counts = {}
    for name, fn in (("decode_op", decode_op), ("torch_chain", chain)):
        k, detail = device_kernels(fn)
        counts[name] = {"device_kernels": k, "writing_aten_calls": writing_ops(fn)}
        if k is None:
            counts[name]["device_kernels_not_counted"] = detail
    counts["decode_op"]["library_launches"] = 1                  # one hipLaunchKernelGGL per call (csrc/decode_detect.hip)

    def event_window(fn, k):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(k):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3 / k                  # us per call

    # ---- (b): the two validation passes; the test wiring's blob prepared once
    test_data, test_info = blobs["data"], blobs["im_info"][:, :3].contiguous()
    eval_batch.get_test_blobs = lambda planes, net_name: (test_data, test_info)
    planes = [None] * n

    def one_forward_pass():
        return solver.validate([blobs], feed_schedule=False, gt_roidb=gt)

    def two_forward_pass():
        out = solver.validate([blobs], feed_schedule=False)
        out.update(eval_batch.evaluate_images(net, planes, gt, "Resnet", batch_size=n))
        return out

    def host_window(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k               # ms per pass

    sides_a = {"decode_op": decode_op, "torch_chain": chain}
    sides_b = {"validate_with_gt_roidb": one_forward_pass, "validate_plus_evaluate_images": two_forward_pass}
    per_pass = {}
    for name, fn in sides_b.items():
        forwards[0] = 0
        res = fn()
        per_pass[name] = forwards[0]
        assert len(res["corloc_list"]) == K and len(res["aps"]) == K - 1
    for name, fn in sides_a.items():
        event_window(fn, a.warmup * 50)
    for name, fn in sides_b.items():
        host_window(fn, a.warmup)
    times = {name: [] for name in list(sides_a) + list(sides_b)}
    for _ in range(a.rounds):
        for name, fn in sides_a.items():
            times[name].append(event_window(fn, a.calls))
        for name, fn in sides_b.items():
            times[name].append(host_window(fn, a.passes))

    out = {"depth": a.depth, "images": n, "image_size": [a.height, a.width], "roi_rows": R, "classes": K,
           "rounds": a.rounds, "calls_per_window": a.calls, "passes_per_window": a.passes, "launches": counts,
           "forwards_per_pass": per_pass, "decode_vs_chain_max_abs_diff": worst, "sides": {}}
    print("ResNet-%d combined wiring, %d images of %d x %d, %d RoI rows, K = %d" % (a.depth, n, a.height, a.width, R, K))
    for group, unit in ((sides_a, "us/call"), (sides_b, "ms/pass")):
        for name in group:
            ts = times[name]
            med, spread = statistics.median(ts), max(ts) - min(ts)
            out["sides"][name] = {"unit": unit, "median": round(med, 3), "spread": round(spread, 3), "min": round(min(ts), 3)}
            extra = ""
            if name in counts:
                c = counts[name]
                extra = "  device kernels %s, tensor-writing ATen calls %d" % (
                    c["device_kernels"] if c["device_kernels"] is not None else "not counted", c["writing_aten_calls"])
            if name in per_pass:
                extra = "  forwards per pass %d" % per_pass[name]
            print("%-30s %10.3f %s  (spread %8.3f, min %10.3f)%s" % (name, med, unit, spread, min(ts), extra))
    print("decode op against the chain on the live rows: largest absolute difference %.3g px" % worst)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
