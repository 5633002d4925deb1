// Host-side check of wssdl_draw_detections' argument validation (csrc/draw_detect.hip): every rejected call must return
// its status before anything is launched, so this runs without a GPU, under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       wssdl_bus_amd/csrc/draw_detect.hip wssdl_bus_amd/csrc/api_common.hip tools/draw_host_check.cpp \
//       -o draw_host_check && ./draw_host_check
//
// The pointers that stand for device memory are never dereferenced on the host: they point at small host arrays so
// that a validation that did read them would be seen by the sanitizer rather than fault.  No call here gets past the
// checks: the valid table is sent with a workspace that is too small, which is the last check before the launches.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <vector>

#include "../include/wssdl_bus_hip.h"

namespace {

struct Call {
    std::vector<uint8_t> arena, out, colours, glyphs, labels, ws;
    std::vector<wssdl_draw_item> items;
    std::vector<float> gt_boxes, dets;
    std::vector<int32_t> gt_classes, off, counts;
    wssdl_draw_style style;
    int N = 2, K = 3, P = 4, G = 3, n_glyphs = 40;
    size_t arena_bytes, out_bytes, ws_bytes;
    bool null_arena = false, null_items_host = false, null_items_dev = false, null_gt_boxes = false, null_gt_classes = false,
         null_off_host = false, null_off_dev = false, null_dets = false, null_counts = false, null_colours = false, null_glyphs = false,
         null_labels = false, null_style = false, null_out = false, null_ws = false;

    Call()
        : arena(8 * 10 + 5 * 6 + 5, 0), out(397, 0), colours(9, 0), glyphs(40 * 7, 0), labels(3 * WSSDL_DRAW_LABEL_LEN, 255), ws(1, 0),
          items(2), gt_boxes(3 * 4, 0.f), dets(2 * 2 * 4 * 5, 0.f), gt_classes(3, 1), off{0, 2, 3}, counts(4, 0) {
        items[0] = wssdl_draw_item{0, 0, 8, 10, 10, 0};
        items[1] = wssdl_draw_item{80, 300, 6, 5, 6, 0};
        style = wssdl_draw_style{3, 11, 5, 2, 3, 4, 10, 0.5f};
        arena_bytes = arena.size();
        out_bytes = out.size();
        ws_bytes = 0;                                          // too small: a call that passes every check stops here
    }

    int run() {
        return wssdl_draw_detections(null_arena ? nullptr : arena.data(), arena_bytes, null_items_host ? nullptr : items.data(),
                                     null_items_dev ? nullptr : items.data(), N, null_gt_boxes ? nullptr : gt_boxes.data(),
                                     null_gt_classes ? nullptr : gt_classes.data(), null_off_host ? nullptr : off.data(),
                                     null_off_dev ? nullptr : off.data(), G, null_dets ? nullptr : dets.data(),
                                     null_counts ? nullptr : counts.data(), K, P, null_colours ? nullptr : colours.data(),
                                     null_glyphs ? nullptr : glyphs.data(), n_glyphs, null_labels ? nullptr : labels.data(),
                                     null_style ? nullptr : &style, null_out ? nullptr : out.data(), out_bytes,
                                     null_ws ? nullptr : ws.data(), ws_bytes, nullptr);
    }
};

int n_checks = 0, n_bad = 0;

void expect(const char *what, int got, int want) {
    ++n_checks;
    if (got != want) {
        ++n_bad;
        std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    }
}

template <typename F>
void invalid(const char *what, F change) {
    Call c;
    change(c);
    expect(what, c.run(), WSSDL_ERR_INVALID_ARGUMENT);
}

template <typename F>
void passes(const char *what, F change) {
    Call c;
    change(c);
    expect(what, c.run(), WSSDL_ERR_WORKSPACE);
}

}  // namespace

int main() {
    expect("workspace query rejects N = 0", wssdl_draw_workspace_bytes(0) == 0, 1);
    expect("workspace query rejects N = 65536", wssdl_draw_workspace_bytes(65536) == 0, 1);
    expect("workspace query", wssdl_draw_workspace_bytes(2) >= 2 * 256 * 56, 1);

    passes("the valid table stops at the workspace check", [](Call &) {});
    passes("workspace one byte short", [](Call &c) { c.ws_bytes = wssdl_draw_workspace_bytes(2) - 1; });
    passes("null workspace", [](Call &c) { c.null_ws = true;  c.ws_bytes = (size_t)1 << 30; });
    passes("output images that touch", [](Call &c) { c.items[1].out_offset = 240; });
    passes("an output image that ends with the arena", [](Call &c) { c.items[1].out_offset = 307; });
    passes("the style's upper ends", [](Call &c) { c.style = wssdl_draw_style{15, 255, 255, 4, 15, 64, 96, 0.f}; });
    passes("no ground truth and no detection rows", [](Call &c) {
        c.G = 0;  c.off = {0, 0, 0};  c.null_gt_boxes = c.null_gt_classes = true;  c.P = 0;  c.null_dets = true;
    });

    invalid("N = 0", [](Call &c) { c.N = 0; });
    invalid("N = -1", [](Call &c) { c.N = -1; });
    invalid("N = 65536", [](Call &c) { c.N = 65536; });
    invalid("K = 1", [](Call &c) { c.K = 1; });
    invalid("K = 66", [](Call &c) { c.K = 66; });
    invalid("G = -1", [](Call &c) { c.G = -1; });
    invalid("P = -1", [](Call &c) { c.P = -1; });
    invalid("13 glyphs", [](Call &c) { c.n_glyphs = 13; });
    invalid("255 glyphs", [](Call &c) { c.n_glyphs = 255; });
    invalid("null arena", [](Call &c) { c.null_arena = true; });
    invalid("null host items", [](Call &c) { c.null_items_host = true; });
    invalid("null device items", [](Call &c) { c.null_items_dev = true; });
    invalid("null gt boxes", [](Call &c) { c.null_gt_boxes = true; });
    invalid("null gt classes", [](Call &c) { c.null_gt_classes = true; });
    invalid("null host offsets", [](Call &c) { c.null_off_host = true; });
    invalid("null device offsets", [](Call &c) { c.null_off_dev = true; });
    invalid("null dets", [](Call &c) { c.null_dets = true; });
    invalid("null counts", [](Call &c) { c.null_counts = true; });
    invalid("null colours", [](Call &c) { c.null_colours = true; });
    invalid("null glyphs", [](Call &c) { c.null_glyphs = true; });
    invalid("null labels", [](Call &c) { c.null_labels = true; });
    invalid("null style", [](Call &c) { c.null_style = true; });
    invalid("null out", [](Call &c) { c.null_out = true; });
    invalid("h = 0", [](Call &c) { c.items[0].h = 0; });
    invalid("w = -3", [](Call &c) { c.items[1].w = -3; });
    invalid("row_stride < w", [](Call &c) { c.items[0].row_stride = 9; });
    invalid("a plane that leaves its arena", [](Call &c) { c.items[1].offset = 81; });
    invalid("a plane offset beyond the arena", [](Call &c) { c.items[1].offset = 1 << 20; });
    invalid("a negative plane offset", [](Call &c) { c.items[0].offset = -1; });
    invalid("an arena one byte short", [](Call &c) { c.arena_bytes -= 1; });
    invalid("an output image that leaves its arena", [](Call &c) { c.items[1].out_offset = 308; });
    invalid("a negative output offset", [](Call &c) { c.items[1].out_offset = -1; });
    invalid("an output one byte short", [](Call &c) { c.out_bytes = 389; });
    invalid("output images that overlap by a byte", [](Call &c) { c.items[1].out_offset = 239; });
    invalid("output images that coincide", [](Call &c) { c.items[1].out_offset = 0; });
    invalid("a huge plane whose size overflows 32 bits", [](Call &c) { c.items[0].h = 0x7fffffff;  c.items[0].w = c.items[0].row_stride = 0x7fffffff; });
    invalid("65 ground-truth boxes in one image", [](Call &c) {
        c.G = 66;  c.off = {0, 65, 66};  c.gt_boxes.assign(66 * 4, 0.f);  c.gt_classes.assign(66, 1);
    });
    invalid("(K-1) * max_draw = 194", [](Call &c) { c.style.max_draw = 97; });
    invalid("max_draw 193", [](Call &c) { c.K = 2;  c.style.max_draw = 193; });
    invalid("even line width", [](Call &c) { c.style.line_width = 4; });
    invalid("line width 0", [](Call &c) { c.style.line_width = 0; });
    invalid("line width 17", [](Call &c) { c.style.line_width = 17; });
    invalid("dash_on 0", [](Call &c) { c.style.dash_on = 0; });
    invalid("dash_on 256", [](Call &c) { c.style.dash_on = 256; });
    invalid("dash_off -1", [](Call &c) { c.style.dash_off = -1; });
    invalid("glyph_scale 0", [](Call &c) { c.style.glyph_scale = 0; });
    invalid("glyph_scale 5", [](Call &c) { c.style.glyph_scale = 5; });
    invalid("tag_pad -1", [](Call &c) { c.style.tag_pad = -1; });
    invalid("tag_pad 16", [](Call &c) { c.style.tag_pad = 16; });
    invalid("tag_dy -1", [](Call &c) { c.style.tag_dy = -1; });
    invalid("tag_dy 65", [](Call &c) { c.style.tag_dy = 65; });
    invalid("max_draw -1", [](Call &c) { c.style.max_draw = -1; });
    invalid("NaN vis_thresh", [](Call &c) { c.style.vis_thresh = std::nanf(""); });
    invalid("offsets that do not start at 0", [](Call &c) { c.off = {1, 2, 3}; });
    invalid("offsets that decrease", [](Call &c) { c.off = {0, 4, 3}; });
    invalid("offsets that do not end at G", [](Call &c) { c.off = {0, 2, 2}; });
    std::printf("%d checks, %d failures\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}
