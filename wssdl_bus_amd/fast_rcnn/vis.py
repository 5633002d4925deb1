"""Qualitative results: ground truth and detections drawn over the grey planes of a whole pass in ONE device op
(wssdl_draw_detections, csrc/draw_detect.hip), PNG files written with the standard library.

The reference draws every validation / test image with matplotlib (fast_rcnn/test_bus.py:337-390,
fast_rcnn/train_bus.py:824-870: grey image, ground truth as solid rectangles, the first detections above 0.5 as dashed
rectangles with a '<class> <score>' tag, red for 'malignant' and blue otherwise).  Here the detections already lie on
the device; the overlay of all images is two launches and only finished RGB bytes come back.  The drawing rules are this
project's own and exact (include/wssdl_bus_hip.h states them); matplotlib's anti-aliased rendering, fonts and figure
margins are NOT reproduced -- parity with the reference's pictures is UNPINNED.
"""
import ctypes
import os
import struct
import zlib

import numpy as np
import torch

from .. import _lib

# 5x7 bitmaps, rows from the top, '#' = set.  The order is the op's fixed glyph order: space . - _ 0-9, then a-z.
_GLYPH_ROWS = {
    ' ': ".....|.....|.....|.....|.....|.....|.....",
    '.': ".....|.....|.....|.....|.....|.##..|.##..",
    '-': ".....|.....|.....|#####|.....|.....|.....",
    '_': ".....|.....|.....|.....|.....|.....|#####",
    '0': ".###.|#...#|#..##|#.#.#|##..#|#...#|.###.",
    '1': "..#..|.##..|..#..|..#..|..#..|..#..|.###.",
    '2': ".###.|#...#|....#|...#.|..#..|.#...|#####",
    '3': "#####|...#.|..#..|...#.|....#|#...#|.###.",
    '4': "...#.|..##.|.#.#.|#..#.|#####|...#.|...#.",
    '5': "#####|#....|####.|....#|....#|#...#|.###.",
    '6': "..##.|.#...|#....|####.|#...#|#...#|.###.",
    '7': "#####|....#|...#.|..#..|.#...|.#...|.#...",
    '8': ".###.|#...#|#...#|.###.|#...#|#...#|.###.",
    '9': ".###.|#...#|#...#|.####|....#|...#.|.##..",
    'a': ".....|.....|.###.|....#|.####|#...#|.####",
    'b': "#....|#....|#.##.|##..#|#...#|#...#|####.",
    'c': ".....|.....|.###.|#....|#....|#...#|.###.",
    'd': "....#|....#|.##.#|#..##|#...#|#...#|.####",
    'e': ".....|.....|.###.|#...#|#####|#....|.###.",
    'f': "..##.|.#..#|.#...|###..|.#...|.#...|.#...",
    'g': ".....|.####|#...#|#...#|.####|....#|.###.",
    'h': "#....|#....|#.##.|##..#|#...#|#...#|#...#",
    'i': "..#..|.....|.##..|..#..|..#..|..#..|.###.",
    'j': "...#.|.....|..##.|...#.|...#.|#..#.|.##..",
    'k': "#....|#....|#..#.|#.#..|##...|#.#..|#..#.",
    'l': ".##..|..#..|..#..|..#..|..#..|..#..|.###.",
    'm': ".....|.....|##.#.|#.#.#|#.#.#|#...#|#...#",
    'n': ".....|.....|#.##.|##..#|#...#|#...#|#...#",
    'o': ".....|.....|.###.|#...#|#...#|#...#|.###.",
    'p': ".....|####.|#...#|#...#|####.|#....|#....",
    'q': ".....|.####|#...#|#...#|.####|....#|....#",
    'r': ".....|.....|#.##.|##..#|#....|#....|#....",
    's': ".....|.....|.###.|#....|.###.|....#|####.",
    't': ".#...|.#...|###..|.#...|.#...|.#..#|..##.",
    'u': ".....|.....|#...#|#...#|#...#|#..##|.##.#",
    'v': ".....|.....|#...#|#...#|#...#|.#.#.|..#..",
    'w': ".....|.....|#...#|#...#|#.#.#|#.#.#|.#.#.",
    'x': ".....|.....|#...#|.#.#.|..#..|.#.#.|#...#",
    'y': ".....|#...#|#...#|#...#|.####|....#|.###.",
    'z': ".....|.....|#####|...#.|..#..|.#...|#####",
}
GLYPH_CHARS = " .-_0123456789abcdefghijklmnopqrstuvwxyz"
LABEL_LEN = _lib.DRAW_LABEL_LEN
BLANK = 0                                   # any character outside GLYPH_CHARS paints nothing, like the space


def glyph_table():
    """[n_glyphs, 7] u8: one byte per row from the top, bit 4 the left column."""
    out = np.zeros((len(GLYPH_CHARS), 7), np.uint8)
    for i, ch in enumerate(GLYPH_CHARS):
        rows = _GLYPH_ROWS[ch].split('|')
        for r, bits in enumerate(rows):
            out[i, r] = sum(1 << (4 - c) for c in range(5) if bits[c] == '#')
    return out


def glyph_indices(text):
    """Glyph indices of `text`: upper case folds to lower, any other character is blank."""
    return [GLYPH_CHARS.index(ch) if ch in GLYPH_CHARS else BLANK for ch in str(text).lower()]


def label_table(classes):
    """[K, 24] u8 glyph indices of the class names, terminated by 255 (a longer name is cut)."""
    out = np.full((len(classes), LABEL_LEN), 255, np.uint8)
    for k, name in enumerate(classes):
        idx = glyph_indices(name)[:LABEL_LEN]
        out[k, :len(idx)] = idx
    return out


def colour_table(classes):
    """[K, 3] u8: red for the class named 'malignant', blue otherwise (the reference's two colours)."""
    out = np.zeros((len(classes), 3), np.uint8)
    for k, name in enumerate(classes):
        out[k] = (255, 0, 0) if name == 'malignant' else (0, 0, 255)
    return out


def score_millis(score):
    """The op's integer rule for the three decimals of an f32 score: n = round-half-even(score * 1000) computed from
    the bits (score = m * 2^-s), n = 0 once s > 40.  Equal to int('{:.3f}' without the point) on [0, 1]."""
    u = int(np.asarray(score, np.float32).view(np.uint32))
    e = (u >> 23) & 0xff
    m = (0x800000 | (u & 0x7fffff)) if e else (u & 0x7fffff)
    s = 150 - e if e else 149
    prod = m * 1000
    if s > 40:
        return 0
    if s <= 0:
        return prod
    q, rem, half = prod >> s, prod & ((1 << s) - 1), 1 << (s - 1)
    return q + (1 if (rem > half or (rem == half and (q & 1))) else 0)


def score_text(score):
    n = score_millis(score)
    return "%d.%03d" % ((n // 1000) % 10, n % 1000)


class _DrawItem(ctypes.Structure):
    """wssdl_draw_item (include/wssdl_bus_hip.h)."""
    _fields_ = [("offset", ctypes.c_int64), ("out_offset", ctypes.c_int64), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("row_stride", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DrawStyle(ctypes.Structure):
    """wssdl_draw_style with the defaults of the header."""
    _fields_ = [(k, ctypes.c_int32) for k in ("line_width", "dash_on", "dash_off", "glyph_scale", "tag_pad", "tag_dy",
                                              "max_draw")] + [("vis_thresh", ctypes.c_float)]

    def __init__(self, line_width=3, dash_on=11, dash_off=5, glyph_scale=2, tag_pad=3, tag_dy=4, max_draw=10,
                 vis_thresh=0.5):
        super(DrawStyle, self).__init__(line_width, dash_on, dash_off, glyph_scale, tag_pad, tag_dy, max_draw, vis_thresh)


def _item_table(shapes, strides, offsets, out_offsets):
    items = (_DrawItem * len(shapes))()
    for it, (h, w), rs, o, oo in zip(items, shapes, strides, offsets, out_offsets):
        it.offset, it.out_offset, it.h, it.w, it.row_stride = int(o), int(oo), int(h), int(w), int(rs)
    return items


def prepare_draw(items, gt_offsets, device):
    """The device-side copies and the workspace one call needs: (device item table, device offsets, workspace).  Made
    outside a graph capture; draw_raw(..., prepared=...) then enqueues nothing but the op's two kernels."""
    L = _lib.lib()
    nb = ctypes.sizeof(items)
    table = torch.empty((nb,), dtype=torch.uint8, pin_memory=True)
    ctypes.memmove(table.data_ptr(), ctypes.addressof(items), nb)
    off_h = np.ascontiguousarray(gt_offsets, np.int32)
    with torch.cuda.device(device):
        n = L.wssdl_draw_workspace_bytes(len(items))
        return (table.to(device), torch.from_numpy(off_h).to(device), torch.empty((max(n, 1),), dtype=torch.uint8, device=device))


def draw_raw(arena, items, gt_boxes, gt_classes, gt_offsets, dets, counts, colours, glyphs, labels, style, out, prepared=None):
    """One wssdl_draw_detections call on device tensors (arena u8, gt_boxes [G,4] f32, gt_classes [G] i32, dets
    [N,K-1,P,5] f32, counts [N,K-1] i32, colours [K,3] u8, glyphs [n,7] u8, labels [K,24] u8, out u8); `items` is the
    ctypes table and gt_offsets the host i32 array [N+1].  Writes into `out`; no read-back, no synchronise.
    prepared: prepare_draw's tuple for the same items and offsets (default: made here)."""
    _lib.require_cuda(arena, gt_boxes, gt_classes, dets, counts, colours, glyphs, labels, out)
    L = _lib.lib()
    N, K, P = len(items), int(colours.shape[0]), int(dets.shape[2])
    off_h = np.ascontiguousarray(gt_offsets, np.int32)
    table_d, off_d, ws = prepared if prepared is not None else prepare_draw(items, off_h, out.device)
    with torch.cuda.device(out.device):
        _lib.check(L.wssdl_draw_detections(
            _lib.ptr(arena), arena.numel(), ctypes.cast(items, ctypes.c_void_p), _lib.ptr(table_d), N, _lib.ptr(gt_boxes),
            _lib.ptr(gt_classes), _lib.host_ptr(off_h), _lib.ptr(off_d), int(gt_boxes.shape[0]), _lib.ptr(dets), _lib.ptr(counts),
            K, P, _lib.ptr(colours), _lib.ptr(glyphs), int(glyphs.shape[0]), _lib.ptr(labels),
            ctypes.cast(ctypes.pointer(style), ctypes.c_void_p), _lib.ptr(out), out.numel(), _lib.ptr(ws), ws.numel(), _lib.stream()),
            "wssdl_draw_detections")
    return out


def draw_detections(planes, gt_roidb, acc_or_dets, classes, first_image=0, style=None, colours=None, device=None):
    """The pictures of `planes` (N grey planes [h, w] u8, numpy) with their ground truth (gt_roidb: one entry per plane,
    as for datasets.voc_eval_bus.pack_gt) and detections: a DetectionAccumulator whose images first_image ..
    first_image + N - 1 these are, or (dets [N, K-1, P, 5], counts [N, K-1]) device tensors for exactly these planes.
    classes: the class names, '__background__' first.  Returns a list of [h, w, 3] u8 arrays.  The planes go up in one
    copy, the op runs once for all N images, and the output arena comes back in one copy."""
    from ..datasets.voc_eval_bus import pack_gt
    N, K = len(planes), len(classes)
    if N < 1 or len(gt_roidb) != N:
        raise ValueError("expected at least one plane and one gt_roidb entry per plane")
    if hasattr(acc_or_dets, "gathered"):
        if acc_or_dets.num_classes != K:
            raise ValueError("the accumulator holds %d classes, `classes` names %d" % (acc_or_dets.num_classes, K))
        dets, counts = acc_or_dets.gathered(int(first_image) + N)
        dets, counts = dets[int(first_image):], counts[int(first_image):]
    else:
        dets, counts = acc_or_dets
    dev = torch.device(device) if device is not None else (
        dets.device if isinstance(dets, torch.Tensor) and dets.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    dets = _lib.to_device(dets, torch.float32, dev)
    counts = _lib.to_device(counts, torch.int32, dev)
    if dets.dim() != 4 or tuple(dets.shape[:2]) != (N, K - 1) or dets.shape[3] != 5 or tuple(counts.shape) != (N, K - 1):
        raise ValueError("expected dets [N, K-1, P, 5] and counts [N, K-1] for N = %d planes and K = %d classes" % (N, K))
    planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
    if any(p.ndim != 2 for p in planes):
        raise ValueError("expected grey planes [h, w]")
    sizes = [p.size for p in planes]
    offsets = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    out_offsets = offsets * 3
    total = int(sum(sizes))
    host = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for p, o in zip(planes, offsets):
        hv[int(o):int(o) + p.size] = p.reshape(-1)
    items = _item_table([p.shape for p in planes], [p.shape[1] for p in planes], offsets, out_offsets)
    gb, gc, _, goff = pack_gt(gt_roidb)
    style = style if style is not None else DrawStyle()
    colours = colour_table(classes) if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(K, 3)
    with torch.cuda.device(dev):
        arena = host.to(dev, non_blocking=True)
        out = torch.empty((total * 3,), dtype=torch.uint8, device=dev)
        draw_raw(arena, items, _lib.to_device(gb.astype(np.float32).reshape(-1, 4), torch.float32, dev),
                 _lib.to_device(gc, torch.int32, dev), goff, dets, counts, _lib.to_device(colours, torch.uint8, dev),
                 _lib.to_device(glyph_table(), torch.uint8, dev), _lib.to_device(label_table(classes), torch.uint8, dev), style, out)
        flat = out.cpu().numpy()                                # the one read-back
    return [flat[int(oo):int(oo) + p.size * 3].reshape(p.shape[0], p.shape[1], 3) for p, oo in zip(planes, out_offsets)]


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def png_bytes(image):
    """An [h, w, 3] u8 array as a PNG file (8-bit RGB, filter 0 on every row, zlib): standard library only."""
    im = np.ascontiguousarray(image, np.uint8)
    if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError("expected an [h, w, 3] u8 image")
    h, w = im.shape[:2]
    raw = np.zeros((h, 1 + w * 3), np.uint8)
    raw[:, 1:] = im.reshape(h, w * 3)
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            _png_chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def qualitative_paths(save_dir, image_paths):
    """<save_dir>/<image basename>.png for every image path (the reference's test_save_path file names)."""
    return [os.path.join(save_dir, os.path.splitext(os.path.basename(str(p)))[0] + ".png") for p in image_paths]


def save_qualitative(images, paths):
    """Writes every image to its path as a PNG (the directories are created; a file appears under its name only whole)."""
    if len(images) != len(paths):
        raise ValueError("one path per image")
    for im, path in zip(images, paths):
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "wb") as f:
            f.write(png_bytes(im))
        os.replace(tmp, path)
    return list(paths)
