"""A NumPy restatement of wssdl_draw_detections, written from the comment in include/wssdl_bus_hip.h alone: plain
loops and slices, Python's own '{:.3f}' for the score's text (so the op's integer rule is checked independently),
and a small PNG decoder for the round trip of the writer.  Not imported by the package."""
import struct
import zlib

import numpy as np

GLYPH_ORDER = " .-_0123456789abcdefghijklmnopqrstuvwxyz"

DEFAULT_STYLE = dict(line_width=3, dash_on=11, dash_off=5, glyph_scale=2, tag_pad=3, tag_dy=4, max_draw=10, vis_thresh=0.5)


def rounded_box(box):
    """(X1, Y1, X2, Y2) as Python ints, or None for a box the op skips."""
    b = np.asarray(box, np.float32)
    if not np.all(np.isfinite(b)) or np.any(np.abs(b) >= np.float32(2.0 ** 24)):
        return None
    X1, Y1, X2, Y2 = (int(v) for v in np.rint(b))
    if X2 < X1 or Y2 < Y1:
        return None
    return X1, Y1, X2, Y2


def paint_outline(img, corners, colour, style, dashed):
    h, w = img.shape[:2]
    X1, Y1, X2, Y2 = corners
    hw = (style['line_width'] - 1) // 2
    period = style['dash_on'] + style['dash_off']
    for y in range(max(Y1 - hw, 0), min(Y2 + hw, h - 1) + 1):
        for x in range(max(X1 - hw, 0), min(X2 + hw, w - 1) + 1):
            if X1 + hw < x < X2 - hw and Y1 + hw < y < Y2 - hw:
                continue
            if dashed:
                if abs(y - Y1) <= hw or abs(y - Y2) <= hw:
                    on = (x - (X1 - hw)) % period < style['dash_on']
                else:
                    on = (y - (Y1 - hw)) % period < style['dash_on']
                if not on:
                    continue
            img[y, x] = colour


def text_glyphs(text):
    return [GLYPH_ORDER.index(ch) if ch in GLYPH_ORDER else 0 for ch in text.lower()]


def paint_tag(img, corners, colour, text, glyphs, style):
    h, w = img.shape[:2]
    X1, Y1 = corners[0], corners[1]
    gs, pad = style['glyph_scale'], style['tag_pad']
    idx = text_glyphs(text)
    Wt, Ht = len(idx) * 6 * gs - gs, 7 * gs
    tx0, ty0 = X1, Y1 + style['tag_dy']
    tx1, ty1 = tx0 + Wt + 2 * pad, ty0 + Ht + 2 * pad
    ys, xs = slice(max(ty0, 0), max(min(ty1, h), 0)), slice(max(tx0, 0), max(min(tx1, w), 0))
    region = img[ys, xs].astype(np.int64)
    img[ys, xs] = ((region + np.asarray(colour, np.int64) + 1) >> 1).astype(np.uint8)
    ox, oy = tx0 + pad, ty0 + pad
    for ci, g in enumerate(idx):
        for row in range(7):
            for col in range(5):
                if not (int(glyphs[g, row]) >> (4 - col)) & 1:
                    continue
                for sy in range(gs):
                    for sx in range(gs):
                        x, y = ox + ci * 6 * gs + col * gs + sx, oy + row * gs + sy
                        if 0 <= x < w and 0 <= y < h:
                            img[y, x] = (255, 255, 255)


def paint_image(plane, gt_boxes, gt_classes, dets, counts, colours, glyphs, class_names, style=None):
    """plane [h, w] u8; gt_boxes [g, 4] f32, gt_classes [g]; dets [K-1, P, 5] f32, counts [K-1] of ONE image;
    class_names [K] as they are drawn (already cut to 24 characters).  Returns [h, w, 3] u8."""
    st = dict(DEFAULT_STYLE)
    st.update(style or {})
    plane = np.asarray(plane, np.uint8)
    img = np.dstack([plane, plane, plane]).copy()
    K = len(colours)
    for box, c in zip(np.asarray(gt_boxes, np.float32).reshape(-1, 4), np.asarray(gt_classes).reshape(-1)):
        corners = rounded_box(box)
        if corners is None or not 0 <= int(c) < K:
            continue
        paint_outline(img, corners, colours[int(c)], st, dashed=False)
    dets, counts = np.asarray(dets, np.float32), np.asarray(counts).reshape(-1)
    if len(counts) and int(counts[0]) == -1:
        return img
    thresh = np.float32(st['vis_thresh'])
    for j in range(1, K):
        for p in range(max(min(st['max_draw'], int(counts[j - 1]), dets.shape[1]), 0)):
            score = np.float32(dets[j - 1, p, 4])
            if not score > thresh:
                continue
            corners = rounded_box(dets[j - 1, p, :4])
            if corners is None:
                continue
            paint_outline(img, corners, colours[j], st, dashed=True)
            paint_tag(img, corners, colours[j], '{:s} {:.3f}'.format(class_names[j], float(score)), glyphs, st)
    return img


def decode_png(data):
    """An 8-bit RGB, non-interlaced PNG whose rows all use filter 0 -> [h, w, 3] u8.  Checks signature and CRCs."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, shape = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b"IHDR":
            w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
            shape = (h, w)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            break
        pos += 12 + n
    h, w = shape
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3).copy()
