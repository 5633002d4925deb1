"""CPU: the drawing rules of wssdl_draw_detections as tests/vis_reference.py restates them, on hand-written pixel
sets; the integer score rule and the glyph table of fast_rcnn/vis.py; the PNG writer's round trip; and every
argument error of the export, which returns its status before anything is launched (no GPU needed)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_reference as ref  # noqa: E402

TIES = [0.0625, 0.9995, 0.99951172, 0.5, 0.0005, 0.0015, 0.0025, 0.125, 0.1875, 0.3125, 1.0, 0.0, 2.0 ** -13, 3 * 2.0 ** -13,
        2.0 ** -30, 2.0 ** -41, 2.0 ** -60, 1e-45, 0.9994999, 0.4995, 0.49950001]


def style(**kv):
    s = dict(ref.DEFAULT_STYLE)
    s.update(kv)
    return s


def test_solid_outline_pixel_by_pixel():
    img = np.zeros((16, 16, 3), np.uint8)
    ref.paint_outline(img, (4, 5, 10, 9), (255, 0, 0), style(), dashed=False)
    expect = set()
    for x in range(3, 12):                                      # line width 3: one pixel either side of the edge
        for y in (4, 5, 6, 8, 9, 10):
            expect.add((x, y))
    for y in range(4, 11):
        for x in (3, 4, 5, 9, 10, 11):
            expect.add((x, y))
    got = {(int(x), int(y)) for y, x in zip(*np.nonzero(img[:, :, 0]))}
    assert got == expect
    assert (6, 7) not in got and (8, 7) not in got and len(got) == 9 * 7 - 3 * 1
    assert not img[:, :, 1].any() and not img[:, :, 2].any()


def test_outline_is_clipped_and_line_width_one():
    img = np.zeros((8, 8, 3), np.uint8)
    ref.paint_outline(img, (-3, 2, 4, 20), (0, 0, 255), style(line_width=1), dashed=False)
    got = {(int(x), int(y)) for y, x in zip(*np.nonzero(img[:, :, 2]))}
    assert got == {(x, 2) for x in range(0, 5)} | {(4, y) for y in range(2, 8)}


def test_dash_phase_along_a_40_pixel_side():
    img = np.zeros((60, 60, 3), np.uint8)
    ref.paint_outline(img, (10, 10, 49, 49), (0, 0, 255), style(), dashed=True)
    # the top band starts at x = X1 - hw = 9: 11 on, 5 off
    on = [x for x in range(60) if img[10, x, 2]]
    assert on == [x for x in range(9, 51) if (x - 9) % 16 < 11]
    assert on[:11] == list(range(9, 20)) and 20 not in on and 25 in on
    # the band is hw rows either side, all with the phase of x; the corners count as horizontal
    assert np.array_equal(img[9], img[10]) and np.array_equal(img[11], img[10]) and np.array_equal(img[48], img[10])
    # the left side below the band: phase of y from Y1 - hw = 9
    on_y = [y for y in range(12, 48) if img[y, 10, 2]]
    assert on_y == [y for y in range(12, 48) if (y - 9) % 16 < 11]
    assert np.array_equal(img[12:48, 9], img[12:48, 10]) and np.array_equal(img[12:48, 50], img[12:48, 10])
    assert not img[12:48, 12:48].any()


def test_tag_blend_and_one_glyph_at_scale_2():
    from wssdl_bus_amd.fast_rcnn import vis
    glyphs = vis.glyph_table()
    img = np.full((40, 40, 3), 100, np.uint8)
    img[:, :, 1] = 7
    ref.paint_tag(img, (5, 6, 30, 30), (255, 0, 0), "1", glyphs, style())
    # one character at scale 2: Wt = 10, Ht = 14; the tag is [5, 21) x [10, 30)
    tag = np.zeros((40, 40), bool)
    tag[10:30, 5:21] = True
    assert np.all(img[~tag] == (100, 7, 100))
    # the '1' glyph: ..#.. / .##.. / ..#.. x4 / .###. , every bit a 2x2 block from (8, 13)
    bits = ["..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."]
    white = np.zeros((40, 40), bool)
    for r, row in enumerate(bits):
        for c, ch in enumerate(row):
            if ch == '#':
                white[13 + 2 * r:15 + 2 * r, 8 + 2 * c:10 + 2 * c] = True
    assert np.all(img[white] == 255)
    assert np.all(img[tag & ~white] == ((100 + 255 + 1) >> 1, (7 + 0 + 1) >> 1, (100 + 0 + 1) >> 1))
    assert (img[tag & ~white][0] == (178, 4, 50)).all()


def test_rounding_and_skipped_boxes():
    assert ref.rounded_box([2.5, 3.5, 4.5, 5.5]) == (2, 4, 4, 6)
    assert ref.rounded_box([-0.5, -1.5, 0.5, 1.5]) == (0, -2, 0, 2)
    assert ref.rounded_box([5, 5, 4.4, 9]) is None and ref.rounded_box([5, 5, 9, 4]) is None
    assert ref.rounded_box([5, 5, 5, 5]) == (5, 5, 5, 5)
    assert ref.rounded_box([np.nan, 0, 1, 1]) is None and ref.rounded_box([0, 0, np.inf, 1]) is None
    assert ref.rounded_box([0, 0, 2.0 ** 24, 1]) is None and ref.rounded_box([0, 0, 2.0 ** 24 - 1, 1]) is not None


def test_integer_score_rule_equals_python_format():
    from wssdl_bus_amd.fast_rcnn import vis
    rng = np.random.RandomState(20)
    sample = np.concatenate([np.asarray(TIES, np.float32), rng.rand(20000).astype(np.float32),
                             (np.arange(1, 2000, 2) / 2000.0).astype(np.float32),          # every thousandth midpoint
                             np.nextafter((np.arange(1, 2000, 2) / 2000.0).astype(np.float32), np.float32(0)),
                             np.nextafter((np.arange(1, 2000, 2) / 2000.0).astype(np.float32), np.float32(1)),
                             (np.arange(0, 8193) * 2.0 ** -13).astype(np.float32)])
    for s in sample:
        assert vis.score_text(s) == '{:.3f}'.format(float(s)), repr(s)
    assert vis.score_text(np.float32(0.0625)) == '0.062'
    assert vis.score_text(np.float32(0.9995)) == '0.999'
    assert vis.score_text(np.float32(0.99951172)) == '1.000'


def test_glyph_table():
    from wssdl_bus_amd.fast_rcnn import vis
    g = vis.glyph_table()
    assert g.shape == (40, 7) and g.dtype == np.uint8 and g.max() < 32
    assert vis.GLYPH_CHARS == ref.GLYPH_ORDER
    assert not g[0].any()                                                   # the space
    digits = [tuple(g[4 + d]) for d in range(10)]
    assert len(set(digits)) == 10
    assert len({tuple(r) for r in g}) == 40                                 # every glyph differs from every other
    assert vis.glyph_indices("Mal-1_x.?") == [26, 14, 25, 2, 5, 3, 37, 1, 0]
    lab = vis.label_table(['__background__', 'benign', 'a' * 30])
    assert lab.shape == (3, 24) and lab[1, 6] == 255 and list(lab[1, :6]) == vis.glyph_indices('benign') and (lab[2] == 14).all()
    assert vis.colour_table(['__background__', 'benign', 'malignant']).tolist() == [[0, 0, 255], [0, 0, 255], [255, 0, 0]]


def test_png_round_trip(tmp_path):
    from wssdl_bus_amd.fast_rcnn import vis
    rng = np.random.RandomState(3)
    for shape in ((1, 1, 3), (7, 13, 3), (64, 40, 3)):
        im = rng.randint(0, 256, shape).astype(np.uint8)
        assert np.array_equal(ref.decode_png(vis.png_bytes(im)), im)
    im = rng.randint(0, 256, (5, 9, 3)).astype(np.uint8)
    paths = vis.qualitative_paths(str(tmp_path / "test"), ["/data/a/img_001.jpg", "b.png"])
    assert [os.path.basename(p) for p in paths] == ["img_001.png", "b.png"]
    vis.save_qualitative([im, im[:2]], paths)
    assert np.array_equal(ref.decode_png(open(paths[0], "rb").read()), im)
    assert sorted(os.listdir(str(tmp_path / "test"))) == ["b.png", "img_001.png"]
    with pytest.raises(ValueError):
        vis.png_bytes(im[:, :, 0])


# ---- argument errors of the export: host checks only, nothing is launched --------------------------------------------
@pytest.fixture(scope="module")
def L():
    from wssdl_bus_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


class Args(object):
    """A valid call on host arrays that stand for device memory (a rejected call never touches them)."""

    def __init__(self):
        from wssdl_bus_amd.fast_rcnn import vis
        self.vis = vis
        self.N, self.K, self.P, self.G = 2, 3, 4, 3
        self.arena = np.zeros(8 * 10 + 5 * 6 + 5, np.uint8)
        self.items = vis._item_table([(8, 10), (6, 5)], [10, 6], [0, 80], [0, 300])
        self.out = np.zeros(300 + 90 + 7, np.uint8)
        self.gt_boxes, self.gt_classes = np.zeros((3, 4), np.float32), np.ones(3, np.int32)
        self.off = np.asarray([0, 2, 3], np.int32)
        self.dets, self.counts = np.zeros((2, 2, 4, 5), np.float32), np.zeros((2, 2), np.int32)
        self.colours, self.glyphs, self.labels = np.zeros((3, 3), np.uint8), vis.glyph_table(), np.full((3, 24), 255, np.uint8)
        self.style = vis.DrawStyle()
        self.ws = np.zeros(1, np.uint8)
        self.ws_bytes = None
        self.n_glyphs = 40
        self.arena_bytes, self.out_bytes = self.arena.size, self.out.size
        self.null = set()

    def call(self, L):
        need = L.wssdl_draw_workspace_bytes(self.N) if self.ws_bytes is None else self.ws_bytes

        def p(name):
            if name in self.null:
                return None
            a = getattr(self, name)
            return ctypes.cast(a, ctypes.c_void_p) if name == "items" else ctypes.c_void_p(a.ctypes.data)
        st = None if "style" in self.null else ctypes.cast(ctypes.pointer(self.style), ctypes.c_void_p)
        return L.wssdl_draw_detections(p("arena"), self.arena_bytes, p("items"), p("items"), self.N, p("gt_boxes"), p("gt_classes"),
                                       p("off"), p("off"), self.G, p("dets"), p("counts"), self.K, self.P, p("colours"), p("glyphs"),
                                       self.n_glyphs, p("labels"), st, p("out"), self.out_bytes, p("ws"), need, None)


def _set(a, **kv):
    for k, v in kv.items():
        setattr(a, k, v)


def _item(a, i, **kv):
    for k, v in kv.items():
        setattr(a.items[i], k, v)


def _style(a, **kv):
    for k, v in kv.items():
        setattr(a.style, k, v)


INVALID = {
    "N = 0": lambda a: _set(a, N=0),
    "N = 65536": lambda a: _set(a, N=65536),
    "K = 1": lambda a: _set(a, K=1),
    "K = 66": lambda a: _set(a, K=66),
    "negative G": lambda a: _set(a, G=-1),
    "negative P": lambda a: _set(a, P=-1),
    "too few glyphs": lambda a: _set(a, n_glyphs=13),
    "too many glyphs": lambda a: _set(a, n_glyphs=255),
    "null arena": lambda a: a.null.add("arena"),
    "null items": lambda a: a.null.add("items"),
    "null gt boxes": lambda a: a.null.add("gt_boxes"),
    "null gt classes": lambda a: a.null.add("gt_classes"),
    "null offsets": lambda a: a.null.add("off"),
    "null dets": lambda a: a.null.add("dets"),
    "null counts": lambda a: a.null.add("counts"),
    "null colours": lambda a: a.null.add("colours"),
    "null glyphs": lambda a: a.null.add("glyphs"),
    "null labels": lambda a: a.null.add("labels"),
    "null style": lambda a: a.null.add("style"),
    "null out": lambda a: a.null.add("out"),
    "h = 0": lambda a: _item(a, 0, h=0),
    "w = 0": lambda a: _item(a, 1, w=0),
    "row_stride < w": lambda a: _item(a, 0, row_stride=9),
    "a plane that leaves its arena": lambda a: _item(a, 1, offset=81),
    "a negative plane offset": lambda a: _item(a, 0, offset=-1),
    "an arena one byte short": lambda a: _set(a, arena_bytes=a.arena.size - 1),
    "an output image that leaves its arena": lambda a: _item(a, 1, out_offset=308),
    "a negative output offset": lambda a: _item(a, 1, out_offset=-1),
    "output images that overlap": lambda a: _item(a, 1, out_offset=239),
    "output images that coincide": lambda a: _item(a, 1, out_offset=0),
    "65 ground-truth boxes in one image": lambda a: _set(a, G=66, off=np.asarray([0, 65, 66], np.int32), gt_boxes=np.zeros((66, 4), np.float32),
                                                        gt_classes=np.zeros(66, np.int32)),
    "(K-1) * max_draw > 192": lambda a: _style(a, max_draw=97),
    "even line width": lambda a: _style(a, line_width=2),
    "line width 0": lambda a: _style(a, line_width=0),
    "line width 17": lambda a: _style(a, line_width=17),
    "dash_on 0": lambda a: _style(a, dash_on=0),
    "negative dash_off": lambda a: _style(a, dash_off=-1),
    "glyph_scale 0": lambda a: _style(a, glyph_scale=0),
    "glyph_scale 5": lambda a: _style(a, glyph_scale=5),
    "negative tag_pad": lambda a: _style(a, tag_pad=-1),
    "negative tag_dy": lambda a: _style(a, tag_dy=-1),
    "negative max_draw": lambda a: _style(a, max_draw=-1),
    "NaN vis_thresh": lambda a: _style(a, vis_thresh=float("nan")),
    "offsets that do not start at 0": lambda a: _set(a, off=np.asarray([1, 2, 3], np.int32)),
    "offsets that decrease": lambda a: _set(a, off=np.asarray([0, 4, 3], np.int32)),
    "offsets that do not end at G": lambda a: _set(a, off=np.asarray([0, 2, 2], np.int32)),
}


def test_a_valid_table_passes_every_host_check(L):
    # the same arguments with a workspace that is too small get past every argument check and stop at the workspace
    # check, which is the last one before the launches
    from wssdl_bus_amd import _lib
    a = Args()
    a.ws_bytes = 0
    assert a.call(L) == _lib.ERR_WORKSPACE
    a.ws_bytes = L.wssdl_draw_workspace_bytes(2) - 1
    assert a.call(L) == _lib.ERR_WORKSPACE
    a = Args()
    a.null.add("ws")
    assert a.call(L) == _lib.ERR_WORKSPACE
    # images that touch without overlapping, and an image that ends exactly at the arena's end, are fine
    a = Args()
    a.ws_bytes = 0
    _item(a, 1, out_offset=240)
    assert a.call(L) == _lib.ERR_WORKSPACE
    _item(a, 1, out_offset=a.out.size - 90)
    assert a.call(L) == _lib.ERR_WORKSPACE
    _style(a, max_draw=96, line_width=15, glyph_scale=4)
    assert a.call(L) == _lib.ERR_WORKSPACE


@pytest.mark.parametrize("name", sorted(INVALID))
def test_argument_errors(L, name):
    from wssdl_bus_amd import _lib
    a = Args()
    INVALID[name](a)
    assert a.call(L) == _lib.ERR_INVALID_ARGUMENT


def test_workspace_query_is_pure_host(L):
    assert L.wssdl_draw_workspace_bytes(0) == 0 and L.wssdl_draw_workspace_bytes(65536) == 0
    assert L.wssdl_draw_workspace_bytes(1) >= 256 * 56 and L.wssdl_draw_workspace_bytes(3) >= 3 * 256 * 56
