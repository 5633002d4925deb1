"""GPU: wssdl_draw_detections bit for bit against the NumPy painter of tests/vis_reference.py (written from the header
comment; Python's '{:.3f}' for the text).  The output arena is pre-filled with 0xA5 and has gaps between the images:
bytes outside the images must stay as they were."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CLASSES = ['__background__', 'benign', 'malignant']
FILL = 0xA5
HUGE = 3.0e38


def run_case(planes, strides, gt, dets, counts, style=None, classes=CLASSES, gap=37):
    """planes: [h, w] u8 arrays; strides: row stride per plane (>= w); gt: per image (boxes [g,4], classes [g]);
    dets [N,K-1,P,5], counts [N,K-1].  Returns (pictures from the op, pictures from the painter, whole arena, spans)."""
    import torch
    from wssdl_bus_amd.fast_rcnn import vis
    N, K = len(planes), len(classes)
    offsets, out_offsets, parts, pos, opos = [], [], [], 5, 3              # odd offsets: nothing is aligned by luck
    for p, rs in zip(planes, strides):
        h, w = p.shape
        buf = np.full((h, rs), 0x3C, np.uint8)
        buf[:, :w] = p
        offsets.append(pos), out_offsets.append(opos)
        parts.append((pos, buf.reshape(-1)[:(h - 1) * rs + w]))
        pos += (h - 1) * rs + w + 3
        opos += h * w * 3 + gap
    arena = np.full(pos, 0x3C, np.uint8)
    for o, b in parts:
        arena[o:o + len(b)] = b
    out0 = np.full(opos, FILL, np.uint8)
    items = vis._item_table([p.shape for p in planes], strides, offsets, out_offsets)
    gb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b, _ in gt], 0)
    gc = np.concatenate([np.asarray(c, np.int32).reshape(-1) for _, c in gt])
    goff = np.cumsum([0] + [len(np.asarray(c).reshape(-1)) for _, c in gt]).astype(np.int32)
    st = vis.DrawStyle(**(style or {}))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    colours, glyphs = vis.colour_table(classes), vis.glyph_table()
    out = t(out0)
    vis.draw_raw(t(arena), items, t(gb) if len(gb) else torch.zeros((0, 4), device="cuda"), t(gc) if len(gc) else
                 torch.zeros((0,), dtype=torch.int32, device="cuda"), goff, t(np.asarray(dets, np.float32)),
                 t(np.asarray(counts, np.int32)), t(colours), t(glyphs), t(vis.label_table(classes)), st, out)
    flat = out.cpu().numpy()
    got, want, spans = [], [], []
    for i, p in enumerate(planes):
        h, w = p.shape
        got.append(flat[out_offsets[i]:out_offsets[i] + h * w * 3].reshape(h, w, 3))
        spans.append((out_offsets[i], out_offsets[i] + h * w * 3))
        want.append(ref.paint_image(p, gt[i][0], gt[i][1], np.asarray(dets, np.float32)[i], np.asarray(counts)[i], colours, glyphs,
                                    [c[:24] for c in classes], style))
    return got, want, flat, spans


def assert_gaps_intact(flat, spans):
    keep = np.ones(len(flat), bool)
    for a, b in spans:
        keep[a:b] = False
    assert keep.any() and np.all(flat[keep] == FILL)


def assert_same(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(np.any(g != w, axis=2))
        assert len(bad) == 0, "image %d: %d pixels differ, first (y, x) = %s: got %s, want %s" % (
            i, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def planes_of(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, s).astype(np.uint8) for s in shapes]


def test_one_small_image_ground_truth_partly_outside():
    planes = planes_of([(8, 8)], 1)
    gt = [([[-2.0, 3.0, 5.0, 11.0]], [2])]
    got, want, flat, spans = run_case(planes, [8], gt, np.zeros((1, 2, 1, 5), np.float32), np.zeros((1, 2), np.int32))
    assert_same(got, want)
    assert_gaps_intact(flat, spans)
    assert (got[0][3, 0] == (255, 0, 0)).all() and (got[0][0, 0] == planes[0][0, 0]).all()


def two_image_case():
    """37x53 (h x w) and 64x40, K = 3, P = 16: counts 1 and 12 in image 0, 0 and 12 in image 1."""
    planes = planes_of([(37, 53), (64, 40)], 2)
    P = 16
    dets = np.empty((2, 2, P, 5), np.float32)
    dets[...] = np.nan
    dets[:, :, 1::2] = HUGE                                                 # rows beyond counts: NaN and huge values
    counts = np.asarray([[1, 12], [0, 12]], np.int32)
    up = np.nextafter(np.float32(0.5), np.float32(1))
    dets[0, 0, 0] = (2.5, 3.5, 30.5, 20.5, up)                              # half-pixel corners: 2, 4, 30, 20
    dets[0, 1, :12] = [
        (10, 8, 45, 30, 0.9995),                                            # '0.999'; overlaps the class-1 box and its tag
        (12, 10, 40, 28, 0.99951172),                                       # '1.000'; over the box before
        (30, 5, 20, 25, 0.9),                                               # inverted
        (7, 7, 7, 7, 0.5625),                                               # degenerate: one point; '0.562'
        (np.nan, 1, 5, 5, 0.9), (1, 1, np.inf, 5, 0.9),                     # non-finite
        (200, 300, 260, 340, 0.9),                                          # wholly off the image
        (20, 2, 50, 12, 0.5),                                               # exactly 0.5: not drawn
        (44, 22, 52, 35, 0.6875),                                           # tag clipped at the right and the bottom; '0.688'
        (-30, -30, 3, 3, np.nan),                                           # NaN score: not drawn
        (1, 1, 50, 35, 0.99), (3, 3, 48, 33, 0.98),                         # rows 10 and 11: beyond the cap of 10
    ]
    dets[1, 1, :12] = [(2 + 3 * k, 1 + 5 * k, 14 + 3 * k, 9 + 5 * k, 0.51 + 0.04 * k) for k in range(12)]
    dets[1, 1, 3, :4] = (-1.0e30, 0, 5, 5)                                  # |v| >= 2^24
    dets[1, 1, 4, :4] = (-20.5, 50.5, 8.5, 70.5)                            # partly off: left and bottom
    gt = [([[5, 5, 25, 25], [30.5, 10.5, 51.5, 36.0]], [1, 2]), ([[0, 0, 39, 63]], [1])]
    return planes, [53, 47], gt, dets, counts


STYLES = [None, dict(line_width=1, glyph_scale=1), dict(line_width=5, glyph_scale=3),
          dict(vis_thresh=0.0, max_draw=12, dash_on=3, dash_off=0, tag_pad=0, tag_dy=0)]


@pytest.mark.parametrize("style", STYLES, ids=["default", "lw1_gs1", "lw5_gs3", "thresh0_draw12"])
def test_two_images_every_rule(style):
    planes, strides, gt, dets, counts = two_image_case()
    got, want, flat, spans = run_case(planes, strides, gt, dets, counts, style)
    assert_same(got, want)
    assert_gaps_intact(flat, spans)
    if style is None:
        # the painter drew something of every kind (the comparison is not empty on both sides)
        assert (want[0] == 255).all(axis=2).any() and (want[0] == (255, 0, 0)).all(axis=2).any() and (want[0] == (0, 0, 255)).all(axis=2).any()
        again, _, flat2, _ = run_case(planes, strides, gt, dets, counts, style)
        assert np.array_equal(flat, flat2)                                  # two runs, the same bits


def test_low_scores_and_ties_below_the_default_threshold():
    planes = planes_of([(40, 200)], 5)
    scores = [0.0625, 0.0005, 0.0015, 2.0 ** -13, 1e-45, 0.125]
    dets = np.zeros((1, 2, 6, 5), np.float32)
    for k, s in enumerate(scores):
        dets[0, k % 2, k // 2] = (3 + 60 * (k // 2), 2 + 18 * (k % 2), 50 + 60 * (k // 2), 16 + 18 * (k % 2), s)
    counts = np.asarray([[3, 3]], np.int32)
    got, want, flat, spans = run_case(planes, [203], [(np.zeros((0, 4)), [])], dets, counts, dict(vis_thresh=0.0, glyph_scale=1))
    assert_same(got, want)
    assert_gaps_intact(flat, spans)


def test_overflow_flag_draws_no_detection():
    planes, strides, gt, dets, counts = two_image_case()
    counts = counts.copy()
    counts[0, 0] = -1
    got, want, flat, spans = run_case(planes, strides, gt, dets, counts)
    assert_same(got, want)
    from wssdl_bus_amd.fast_rcnn import vis
    only_gt = ref.paint_image(planes[0], gt[0][0], gt[0][1], dets[0], [0, 0], vis.colour_table(CLASSES), vis.glyph_table(), CLASSES)
    assert np.array_equal(got[0], only_gt)
    assert_gaps_intact(flat, spans)


def test_wide_image_many_tiles():
    # more than one tile in x and y (tiles are 256 x 16), 3 * w not a multiple of 4, a box across the tile borders
    planes = planes_of([(35, 601), (17, 257)], 7)
    dets = np.zeros((2, 2, 2, 5), np.float32)
    dets[0, 0, 0] = (250, 10, 520, 30, 0.75)
    dets[0, 1, 0] = (500, 14, 600, 34, 0.8125)
    dets[1, 1, 0] = (240, 5, 300, 20, 0.9375)
    counts = np.asarray([[1, 1], [0, 1]], np.int32)
    gt = [([[100, 3, 400, 33]], [2]), ([[254, 0, 256, 16]], [1])]
    got, want, flat, spans = run_case(planes, [601, 300], gt, dets, counts, gap=1)
    assert_same(got, want)
    assert_gaps_intact(flat, spans)


def test_wrapper_on_a_real_accumulator():
    import torch
    from wssdl_bus_amd.datasets.voc_eval_bus import DetectionAccumulator
    from wssdl_bus_amd.fast_rcnn import vis
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device
    rng = np.random.RandomState(11)
    K, N, R = 3, 3, 90
    planes = planes_of([(60, 80), (45, 70), (50, 50)], 12)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), R // N)
    scores = rng.rand(R, K).astype(np.float32)
    xy = rng.rand(R, K, 2) * 40
    wh = 5 + rng.rand(R, K, 2) * 30
    boxes = np.concatenate([xy, xy + wh], 2).reshape(R, 4 * K).astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()                                # noqa: E731
    acc = DetectionAccumulator(K)
    d01, c01 = post_detections_batched_device(t(scores[:60]), t(boxes[:60]), t(rois[:60]), 2, K, 0.05, 300, max_rows_per_image=30)
    r2 = rois[60:].copy()
    r2[:, 0] = 0
    d2, c2 = post_detections_batched_device(t(scores[60:]), t(boxes[60:]), t(r2), 1, K, 0.05, 300, max_rows_per_image=30)
    acc.add(d01, c01, 0)
    acc.add(d2, c2, 2)
    gt_roidb = [dict(boxes=np.asarray([[4, 4, 30, 30]]), gt_classes=np.asarray([1])),
                dict(boxes=np.zeros((0, 4)), gt_classes=np.zeros(0, np.int32)),
                dict(boxes=np.asarray([[10, 10, 45, 45], [0, 0, 9, 9]]), gt_classes=np.asarray([2, 1]))]
    pics = vis.draw_detections(planes, gt_roidb, acc, CLASSES)
    dets, counts = acc.gathered(N)
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    assert counts.sum() > 10
    colours, glyphs = vis.colour_table(CLASSES), vis.glyph_table()
    for i in range(N):
        want = ref.paint_image(planes[i], gt_roidb[i]['boxes'], gt_roidb[i]['gt_classes'], dets[i], counts[i], colours, glyphs, CLASSES)
        assert pics[i].shape == planes[i].shape + (3,) and pics[i].dtype == np.uint8
        assert_same([pics[i]], [want])
    # a later slice of the pass: first_image
    tail = vis.draw_detections(planes[1:], gt_roidb[1:], acc, CLASSES, first_image=1)
    assert np.array_equal(tail[0], pics[1]) and np.array_equal(tail[1], pics[2])
    # (dets, counts) instead of the accumulator
    pair = vis.draw_detections(planes, gt_roidb, acc.gathered(N), CLASSES)
    assert all(np.array_equal(a, b) for a, b in zip(pair, pics))


def test_the_op_is_capturable_and_reads_nothing_back():
    """With its device-side tables made beforehand the call enqueues two kernels and nothing else: it runs under
    torch's sync-debug 'error' mode, and a captured graph of it replays to the eager bits on fresh inputs."""
    import torch
    from wssdl_bus_amd.fast_rcnn import vis
    planes, strides, gt, dets, counts = two_image_case()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    sizes = [p.size for p in planes]
    items = vis._item_table([p.shape for p in planes], [p.shape[1] for p in planes], [0, sizes[0]], [0, 3 * sizes[0]])
    arena = t(np.concatenate([p.reshape(-1) for p in planes]))
    gb = t(np.concatenate([np.asarray(b, np.float32) for b, _ in gt]))
    gc = t(np.concatenate([np.asarray(c, np.int32) for _, c in gt]))
    goff = np.asarray([0, 2, 3], np.int32)
    d, c = t(dets), t(counts)
    consts = (t(vis.colour_table(CLASSES)), t(vis.glyph_table()), t(vis.label_table(CLASSES)), vis.DrawStyle())
    prepared = vis.prepare_draw(items, goff, arena.device)
    eager = torch.full((3 * sum(sizes),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        vis.draw_raw(arena, items, gb, gc, goff, d, c, *consts, eager, prepared=prepared)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = torch.full_like(eager, FILL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vis.draw_raw(arena, items, gb, gc, goff, d, c, *consts, out, prepared=prepared)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vis.draw_raw(arena, items, gb, gc, goff, d, c, *consts, out, prepared=prepared)
    out.fill_(0)
    graph.replay()
    assert torch.equal(out, eager)
    # new detections in the same buffers: the replay draws them
    c.copy_(t(np.asarray([[0, 3], [1, 0]], np.int32)))
    vis.draw_raw(arena, items, gb, gc, goff, d, c, *consts, eager, prepared=prepared)
    graph.replay()
    assert torch.equal(out, eager)
    want = ref.paint_image(planes[0], gt[0][0], gt[0][1], dets[0], [0, 3], vis.colour_table(CLASSES), vis.glyph_table(), CLASSES)
    assert np.array_equal(out.cpu().numpy()[:3 * sizes[0]].reshape(want.shape), want)
