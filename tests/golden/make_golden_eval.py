#!/usr/bin/env python3
"""Generate tests/golden/eval_detections.npz: the reference's own datasets/voc_eval_bus.py on result, annotation and
image-set files written here.

Run in the build container only:  python tests/golden/make_golden_eval.py
The reference module is Python 2: it is copied to a temporary directory OUTSIDE the repository, converted there by
lib2to3 and imported from there; its text-mode pickle cache is the one obstacle under Python 3, so `open` is
shadowed in the staged module's namespace to open that one file in binary mode.  Data only goes into the .npz:
the inputs (detections, ground truth, thresholds) and the values the reference returned.  Re-running reproduces
the file bit for bit.

Case `small`: 12 images, 2 classes, at most 8 detections per image and class; the 3-decimal scores of each class
are pairwise distinct (asserted), so the reference's unstable argsort cannot matter.  It holds an image without
boxes, an image with boxes and no detections, a difficult box that is hit, two detections on one box, a detection
whose best box is difficult while it overlaps another, scores on rounding ties (0.0625, 0.1875, 0.3125),
coordinates on rounding ties (x + 1 = 10.25, 10.75) and scores that are thresholds (0.5, 1.0).
Case `runs`: 40 images x 64 detections per class (more than one 2048-key sort run); score ties are unavoidable,
so only what does not depend on the order among ties is stored, and that is asserted by evaluating the result
file's lines in two orders.
"""
import builtins
import importlib.util
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("WSSDL_REFERENCE", "/root/reference")
REF_MODULE = os.path.join(REFERENCE, "code", "lib", "datasets", "voc_eval_bus.py")
OUT = os.path.join(HERE, "eval_detections.npz")
CLASSES = ("__background__", "benign", "malignant")
THRESHOLDS = np.arange(1.0, -0.01, -0.05)


def available():
    return os.path.exists(REF_MODULE)


def stage_reference(tmp):
    """The reference's module, converted to Python 3 in `tmp` and imported from there."""
    from lib2to3.main import main as lib2to3_main
    dst = os.path.join(tmp, "ref_voc_eval_bus.py")
    shutil.copyfile(REF_MODULE, dst)
    saved = sys.stdout, sys.stderr
    try:
        with open(os.devnull, "w") as null:
            sys.stdout = sys.stderr = null
            rc = lib2to3_main("lib2to3.fixes", ["-w", "-n", dst])
    finally:
        sys.stdout, sys.stderr = saved
    assert rc == 0
    spec = importlib.util.spec_from_file_location("ref_voc_eval_bus", dst)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def binary_open_for_the_cache(path, mode="r", *a, **k):
        if str(path).endswith(".pkl") and "b" not in mode:
            mode += "b"
        return builtins.open(path, mode, *a, **k)
    mod.open = binary_open_for_the_cache
    return mod


def image_name(i):
    return "im%04d" % i


def write_annotations(tmp, gt):
    ann = os.path.join(tmp, "Annotations")
    os.makedirs(ann)
    for i, (boxes, cls, dif) in enumerate(gt):
        objs = "".join(
            "<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
            "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
            % (CLASSES[c], d, b[0], b[1], b[2], b[3]) for b, c, d in zip(boxes, cls, dif))
        with open(os.path.join(ann, image_name(i) + ".xml"), "w") as f:
            f.write("<annotation>%s</annotation>" % objs)
    with open(os.path.join(tmp, "set.txt"), "w") as f:
        f.write("".join(image_name(i) + "\n" for i in range(len(gt))))
    return os.path.join(ann, "{:s}.xml"), os.path.join(tmp, "set.txt")


def result_lines(dets, image, cls, c):
    """The result file's lines of class c in its order (image index, then rank): score to 3 decimals, the f32
    coordinates + 1 to one."""
    lines = []
    for k in np.nonzero(cls == c)[0]:
        d = dets[k]
        one = np.float32(1)
        lines.append("%s %s %s %s %s %s\n" % (image_name(image[k]), format(d[4], ".3f"), format(d[0] + one, ".1f"),
                                              format(d[1] + one, ".1f"), format(d[2] + one, ".1f"), format(d[3] + one, ".1f")))
    return lines


def run_reference(mod, tmp, tag, lines_by_class, annopath, setfile, n_images):
    """voc_eval_bus for both classes and all thresholds (11-point AP), once more for the area AP."""
    out = {}
    for c in (1, 2):
        path = os.path.join(tmp, "det_%s_{:s}.txt" % tag)
        with open(path.format(CLASSES[c]), "w") as f:
            f.write("".join(lines_by_class[c]))
        cache = os.path.join(tmp, "cache_%s" % tag)
        rows = []
        for t in THRESHOLDS:
            rows.append(mod.voc_eval_bus(path, annopath, setfile, CLASSES[c], cache, ovthresh=0.5, use_07_metric=True, score_thresh=t))
        area = mod.voc_eval_bus(path, annopath, setfile, CLASSES[c], cache, ovthresh=0.5, use_07_metric=False, score_thresh=0.5)
        rec, prec, ap = rows[0][0], rows[0][1], rows[0][2]
        for r in rows:
            assert np.array_equal(r[0], rec) and np.array_equal(r[1], prec) and r[2] == ap and r[3] == rows[0][3]
        assert np.array_equal(area[0], rec) and np.array_equal(area[1], prec)
        out[c] = dict(rec=np.asarray(rec, np.float64), prec=np.asarray(prec, np.float64), ap07=np.float64(ap), ap_area=np.float64(area[2]),
                      ni=np.int64(rows[0][3]), nok=np.array([r[4] for r in rows], np.int64),
                      arr_ok=np.array([r[5] for r in rows], np.float64),
                      num_all_fps=np.array([r[6] for r in rows], np.int64),
                      num_fp_per_img=np.array([r[7] for r in rows], np.int64).reshape(len(rows), n_images))
    return out


def flat_gt(gt):
    boxes = np.array([b for g in gt for b in g[0]], np.int64).reshape(-1, 4)
    cls = np.array([c for g in gt for c in g[1]], np.int32)
    dif = np.array([d for g in gt for d in g[2]], np.uint8)
    off = np.cumsum([0] + [len(g[1]) for g in gt]).astype(np.int32)
    return boxes, cls, dif, off


def distinct_scores(rs, n, taken):
    """n f32 scores whose 3-decimal forms are pairwise distinct and avoid `taken`; a jitter below the quantum keeps
    the quantisation from being the identity."""
    pool = np.array([k for k in rs.permutation(np.arange(1, 1000)) if k not in taken][:n])
    return (pool / 1000.0 + rs.uniform(-0.0004, 0.0004, n)).astype(np.float32)


def jitter(rs, box, amount):
    b = np.asarray(box, np.float64) - 1.0                     # detections are 0-based
    w, h = b[2] - b[0], b[3] - b[1]
    return (b + rs.uniform(-amount, amount, 4) * np.array([w, h, w, h])).astype(np.float32)


def case_small():
    rs = np.random.RandomState(20)
    gt = [([], [], []) for _ in range(12)]
    gt[1] = ([[50, 50, 150, 150]], [1], [0])                                       # boxes, no detections
    gt[2] = ([[20, 20, 120, 120], [200, 200, 300, 300]], [1, 1], [1, 0])           # a difficult box that is hit
    gt[3] = ([[30, 30, 130, 130], [31, 200, 131, 300]], [1, 2], [0, 0])            # two detections on one box
    gt[4] = ([[40, 40, 140, 140], [60, 60, 160, 160]], [1, 1], [1, 0])             # best box difficult, overlaps another
    for i in range(5, 12):
        n = rs.randint(1, 4)
        boxes = []
        for _ in range(n):
            x, y = rs.randint(1, 300, 2)
            boxes.append([x, y, x + rs.randint(30, 200), y + rs.randint(30, 200)])
        gt[i] = (boxes, list(rs.randint(1, 3, n)), list((rs.rand(n) < 0.25).astype(int)))
    dets, image, cls = [], [], []

    def add(i, c, box, score):
        dets.append(list(np.asarray(box, np.float32)) + [np.float32(score)])
        image.append(i), cls.append(c)
    # hand-made rows: (image, class, box 0-based f32, score)
    add(0, 1, [10, 10, 80, 80], 0.0625)                       # image without boxes; '0.062'
    add(2, 1, [19, 19, 119, 119], 1.0)                        # hits the difficult box; a threshold
    add(2, 1, [201, 203, 297, 301], 0.5)                      # a threshold
    add(3, 1, [29, 29, 129, 129], 0.1875)                     # '0.188'
    add(3, 1, [33, 27, 131, 133], 0.3125)                     # the same box, the better score: '0.312'
    add(3, 2, [9.25, 199, 130, 299], 0.75)                    # x + 1 = 10.25 -> '10.2'
    add(3, 2, [9.75, 150, 130.75, 299.25], 0.875)             # x + 1 = 10.75 -> '10.8'
    add(4, 1, [41, 41, 141, 141], 0.625)                      # best: the difficult box; overlaps the other one
    add(4, 1, [62, 61, 158, 162], 0.25)
    taken = {62, 188, 312, 500, 1000, 750, 875, 625, 250}
    for c in (1, 2):
        rows = []
        for i in range(5, 12):
            boxes = [b for b, k in zip(gt[i][0], gt[i][1])]
            for _ in range(rs.randint(0, 8)):
                if boxes and rs.rand() < 0.7:
                    rows.append((i, jitter(rs, boxes[rs.randint(len(boxes))], rs.choice([0.05, 0.2, 0.5]))))
                else:
                    x, y = rs.uniform(0, 300, 2)
                    rows.append((i, np.array([x, y, x + rs.uniform(20, 150), y + rs.uniform(20, 150)], np.float32)))
        for (i, b), s in zip(rows, distinct_scores(rs, len(rows), taken)):
            add(i, c, b, s)
    dets, image, cls = np.array(dets, np.float32), np.array(image, np.int32), np.array(cls, np.int32)
    order = np.lexsort((np.arange(len(cls)), image, cls))     # result-file order: class, image, rank
    dets, image, cls = dets[order], image[order], cls[order]
    for c in (1, 2):
        q = np.rint(dets[cls == c, 4].astype(np.float64) * 1000.0)
        assert len(np.unique(q)) == len(q), "3-decimal scores of a class must be pairwise distinct"
        assert max(np.bincount(image[cls == c])) <= 8
    return gt, dets, image, cls


def case_runs():
    rs = np.random.RandomState(21)
    gt = []
    for i in range(40):
        boxes, cl, dif = [], [], []
        for c in (1, 2):
            for _ in range(rs.randint(0, 4)):
                x, y = rs.randint(1, 400, 2)
                boxes.append([x, y, x + rs.randint(30, 200), y + rs.randint(30, 200)])
                cl.append(c), dif.append(int(rs.rand() < 0.2))
        gt.append((boxes, cl, dif))
    dets, image, cls = [], [], []
    for c in (1, 2):
        for i in range(40):
            boxes = [b for b, k in zip(gt[i][0], gt[i][1]) if k == c]
            scores = np.sort(rs.randint(0, 1001, 64))[::-1] / 1000.0          # best first, like the post-detection op
            for s in scores:
                if boxes and rs.rand() < 0.3:
                    b = jitter(rs, boxes[rs.randint(len(boxes))], rs.choice([0.05, 0.2, 0.5]))
                else:
                    x, y = rs.uniform(0, 400, 2)
                    b = np.array([x, y, x + rs.uniform(20, 150), y + rs.uniform(20, 150)], np.float32)
                dets.append(list(b) + [np.float32(s)]), image.append(i), cls.append(c)
    return gt, np.array(dets, np.float32), np.array(image, np.int32), np.array(cls, np.int32)


def totals(r, npos):
    """final tp and fp of a class from the reference's curves"""
    tp = int(np.rint(r["rec"][-1] * npos))
    assert tp > 0
    return tp, int(np.rint(tp / r["prec"][-1])) - tp


def generate():
    """{name: array} of the committed file."""
    tmp = tempfile.mkdtemp(prefix="wssdl_golden_eval_")
    assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE)) + os.sep)
    try:
        mod = stage_reference(tmp)
        out = {"thresholds": THRESHOLDS}
        # small: everything
        gt, dets, image, cls = case_small()
        d = os.path.join(tmp, "small")
        os.makedirs(d)
        annopath, setfile = write_annotations(d, gt)
        ref = run_reference(mod, d, "a", {c: result_lines(dets, image, cls, c) for c in (1, 2)}, annopath, setfile, len(gt))
        gb, gc, gd, goff = flat_gt(gt)
        out.update(small_dets=dets, small_image=image, small_class=cls, small_gt_boxes=gb, small_gt_class=gc, small_gt_difficult=gd,
                   small_gt_offsets=goff)
        for c in (1, 2):
            for k, v in ref[c].items():
                out["small_c%d_%s" % (c, k)] = v
        # runs: what does not depend on the order among equal scores
        gt, dets, image, cls = case_runs()
        d = os.path.join(tmp, "runs")
        os.makedirs(d)
        annopath, setfile = write_annotations(d, gt)
        lines = {c: result_lines(dets, image, cls, c) for c in (1, 2)}
        ref_a = run_reference(mod, d, "a", lines, annopath, setfile, len(gt))
        ref_b = run_reference(mod, d, "b", {c: lines[c][::-1] for c in (1, 2)}, annopath, setfile, len(gt))
        gb, gc, gd, goff = flat_gt(gt)
        out.update(runs_dets=dets, runs_image=image, runs_class=cls, runs_gt_boxes=gb, runs_gt_class=gc, runs_gt_difficult=gd,
                   runs_gt_offsets=goff)
        for c in (1, 2):
            npos = int(np.sum((gc == c) & (gd == 0)))
            for k in ("ni", "nok", "arr_ok", "num_all_fps", "num_fp_per_img"):
                assert np.array_equal(ref_a[c][k], ref_b[c][k]), k
                out["runs_c%d_%s" % (c, k)] = ref_a[c][k]
            assert totals(ref_a[c], npos) == totals(ref_b[c], npos)
            out["runs_c%d_npos" % c] = np.int64(npos)
            out["runs_c%d_tp_fp_total" % c] = np.array(totals(ref_a[c], npos), np.int64)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if not available():
        sys.exit("the reference is not on this machine: %s" % REF_MODULE)
    np.savez_compressed(OUT, **generate())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
