// Qualitative results on the device: the ground truth and the detections of all N images of a pass drawn over their
// grey planes in one op (what fast_rcnn/test_bus.py:337-390 and fast_rcnn/train_bus.py:824-870 of the reference do
// image by image with matplotlib), gfx950.  The semantics are this project's own and exact (include/wssdl_bus_hip.h);
// matplotlib's anti-aliased rendering is not reproduced.
//
//   LAUNCHES PER CALL: 2, whatever N is
//     1. draw_build_kernel   grid N x 256 threads: thread t owns one candidate slot of its image (64 ground-truth
//                            slots, then (K-1) * max_draw detection slots in class-then-row order), decides whether it
//                            is drawn, and the drawn ones are written as item records in slot order (an ordered
//                            compaction through LDS flags): rounded corners, colour, dash flag, the glyph indices of
//                            the tag's text with the score's three decimals taken from the f32's bits.
//     2. draw_paint_kernel   grid (tiles, N): a workgroup owns a 256 x 16 pixel tile.  It stages the records whose
//                            extent touches the tile in LDS (in order), then every lane owns 4 adjacent pixels of a
//                            row: one pass over the staged records per pixel, later items over earlier ones.  The 768
//                            bytes a wave produces for its row go through LDS and out as whole dwords where the
//                            address is 4-aligned (head and tail bytes singly): 3 * w need not be a multiple of 4.
// A pure gather: no atomics, every output byte has one writer, the same bits on every run.  Bytes of the output arena
// outside the images are not written.  Every read of the detections is bounded by min(max_draw, counts, P); rows at
// and beyond counts are never read.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.hip.h"

namespace wssdl {
namespace {

constexpr int MAX_GT = WSSDL_DRAW_MAX_GT, MAX_DETS = WSSDL_DRAW_MAX_DETS, MAX_ITEMS = MAX_GT + MAX_DETS;   // 256
constexpr int LABEL_LEN = WSSDL_DRAW_LABEL_LEN, TEXT_LEN = LABEL_LEN + 6;      // label, ' ', 'd.ddd'
constexpr int TILE_W = 256, TILE_H = 16, PX = 4;                                // a lane owns PX adjacent pixels
constexpr int G_SPACE = 0, G_DOT = 1, G_ZERO = 4;                               // the glyph table's fixed layout
static_assert(MAX_ITEMS == 256, "one build thread per candidate slot");

typedef wssdl_draw_item Item;
typedef wssdl_draw_style Style;

struct Rec {
    int x1, y1, x2, y2;                 // rounded corners
    unsigned char r, g, b, kind;        // kind 0: solid outline; 1: dashed outline, tag and text
    unsigned char nchars, pad[3];
    unsigned char text[32];             // glyph indices (TEXT_LEN <= 32)
};
static_assert(sizeof(Rec) == 56 && TEXT_LEN <= 32, "record layout");

__device__ __forceinline__ bool usable(float v) { return fabsf(v) < 16777216.0f; }      // false for NaN and inf

// n = round-half-even(score * 1000) from the f32's bits: score = m * 2^-s
__device__ __forceinline__ unsigned long long score_millis(float score) {
    const unsigned int u = __float_as_uint(score);
    const int e = (int)((u >> 23) & 0xffu);
    const unsigned long long m = e ? (0x800000ull | (u & 0x7fffffu)) : (unsigned long long)(u & 0x7fffffu);
    const int s = e ? 150 - e : 149;
    const unsigned long long prod = m * 1000ull;                                          // < 2^34
    if (s > 40) return 0ull;
    if (s <= 0) return prod;                                                              // >= 2^24: unspecified text
    const unsigned long long q = prod >> s, rem = prod & ((1ull << s) - 1ull), half = 1ull << (s - 1);
    return q + ((rem > half || (rem == half && (q & 1ull))) ? 1ull : 0ull);
}

__global__ __launch_bounds__(MAX_ITEMS) void draw_build_kernel(const Item *__restrict__ items, const float *__restrict__ gt_boxes,
                                                               const int *__restrict__ gt_classes, const int *__restrict__ gt_off, int G,
                                                               const float *__restrict__ dets, const int *__restrict__ counts, int K,
                                                               int P, const unsigned char *__restrict__ colours,
                                                               const unsigned char *__restrict__ labels, Style st,
                                                               int *__restrict__ n_recs, Rec *__restrict__ recs) {
    __shared__ unsigned char s_flag[MAX_ITEMS];
    const int i = blockIdx.x, t = threadIdx.x;
    Rec rec;
    bool on = false;
    int cls = 0;
    const float *box = nullptr;
    rec.kind = 0;
    rec.nchars = 0;
    rec.pad[0] = rec.pad[1] = rec.pad[2] = 0;
    for (int k = 0; k < 32; ++k) rec.text[k] = 255;
    if (t < MAX_GT) {
        int g0 = gt_off[i], g1 = gt_off[i + 1];
        g0 = min(max(g0, 0), G);
        g1 = min(max(g1, g0), G);
        if (t < g1 - g0 && t < MAX_GT) {
            cls = gt_classes[g0 + t];
            box = gt_boxes + (size_t)(g0 + t) * 4;
            on = cls >= 0 && cls < K;
        }
    } else if (st.max_draw > 0 && P > 0) {
        const int d = t - MAX_GT, j1 = d / st.max_draw, p = d - j1 * st.max_draw;
        if (j1 < K - 1 && counts[(size_t)i * (K - 1)] != -1) {
            const int c = min(min(counts[(size_t)i * (K - 1) + j1], st.max_draw), P);
            if (p < c) {
                box = dets + (((size_t)i * (K - 1) + j1) * P + p) * 5;
                cls = j1 + 1;
                rec.kind = 1;
                on = box[4] > st.vis_thresh;                            // strict, false for NaN
            }
        }
    }
    if (on) {
        const float a = box[0], b = box[1], c = box[2], d = box[3];
        on = usable(a) && usable(b) && usable(c) && usable(d);
        if (on) {
            rec.x1 = (int)rintf(a);  rec.y1 = (int)rintf(b);  rec.x2 = (int)rintf(c);  rec.y2 = (int)rintf(d);
            on = rec.x2 >= rec.x1 && rec.y2 >= rec.y1;
        }
    }
    if (on) {
        rec.r = colours[cls * 3];  rec.g = colours[cls * 3 + 1];  rec.b = colours[cls * 3 + 2];
        if (rec.kind) {
            int n = 0;
            for (; n < LABEL_LEN; ++n) {
                const unsigned char ch = labels[cls * LABEL_LEN + n];
                if (ch == 255) break;
                rec.text[n] = ch;
            }
            const unsigned long long m = score_millis(box[4]);
            const unsigned int frac = (unsigned int)(m % 1000ull);
            rec.text[n++] = G_SPACE;
            rec.text[n++] = (unsigned char)(G_ZERO + (int)((m / 1000ull) % 10ull));
            rec.text[n++] = G_DOT;
            rec.text[n++] = (unsigned char)(G_ZERO + frac / 100);
            rec.text[n++] = (unsigned char)(G_ZERO + (frac / 10) % 10);
            rec.text[n++] = (unsigned char)(G_ZERO + frac % 10);
            rec.nchars = (unsigned char)n;
        }
    }
    s_flag[t] = on ? 1 : 0;
    __syncthreads();
    int pos = 0, total = 0;
    for (int k = 0; k < MAX_ITEMS; ++k) {
        const int f = s_flag[k];
        total += f;
        if (k < t) pos += f;
    }
    if (on) recs[(size_t)i * MAX_ITEMS + pos] = rec;
    if (t == 0) n_recs[i] = total;
}

// the tag rectangle of a detection record: [tx0, tx1) x [ty0, ty1)
__device__ __forceinline__ void tag_rect(const Rec &r, const Style &st, int &tx0, int &ty0, int &tx1, int &ty1) {
    const int wt = (int)r.nchars * 6 * st.glyph_scale - st.glyph_scale, ht = 7 * st.glyph_scale;
    tx0 = r.x1;
    ty0 = r.y1 + st.tag_dy;
    tx1 = tx0 + wt + 2 * st.tag_pad;
    ty1 = ty0 + ht + 2 * st.tag_pad;
}

__global__ __launch_bounds__(256) void draw_paint_kernel(const unsigned char *__restrict__ arena, const Item *__restrict__ items,
                                                         const int *__restrict__ n_recs, const Rec *__restrict__ recs,
                                                         const unsigned char *__restrict__ glyphs, int n_glyphs, Style st,
                                                         unsigned char *__restrict__ out) {
    __shared__ Rec s_rec[MAX_ITEMS];
    __shared__ unsigned char s_flag[MAX_ITEMS];
    __shared__ unsigned char s_glyph[256 * 7];
    __shared__ unsigned int s_row[4][TILE_W * 3 / 4];
    __shared__ int s_n;
    const Item it = items[blockIdx.y];
    const int h = it.h, w = it.w;
    const int tiles_x = (w + TILE_W - 1) / TILE_W, tiles_y = (h + TILE_H - 1) / TILE_H;
    if ((long long)blockIdx.x >= (long long)tiles_x * tiles_y) return;                   // (uniform over the workgroup)
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * TILE_W, y0 = tile_y * TILE_H;
    const int xe = min(x0 + TILE_W, w), ye = min(y0 + TILE_H, h);                       // the tile: [x0, xe) x [y0, ye)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int hw = (st.line_width - 1) / 2, period = st.dash_on + st.dash_off;

    // stage the records that touch the tile, in order
    const int count = min(max(n_recs[blockIdx.y], 0), MAX_ITEMS);
    Rec mine;
    bool keep = false;
    if (t < count) {
        mine = recs[(size_t)blockIdx.y * MAX_ITEMS + t];
        int ex0 = mine.x1 - hw, ey0 = mine.y1 - hw, ex1 = mine.x2 + hw + 1, ey1 = mine.y2 + hw + 1;
        if (mine.kind) {
            int tx0, ty0, tx1, ty1;
            tag_rect(mine, st, tx0, ty0, tx1, ty1);
            ex0 = min(ex0, tx0);  ey0 = min(ey0, ty0);  ex1 = max(ex1, tx1);  ey1 = max(ey1, ty1);
        }
        keep = ex0 < xe && ex1 > x0 && ey0 < ye && ey1 > y0;
    }
    s_flag[t] = keep ? 1 : 0;
    for (int k = t; k < n_glyphs * 7; k += 256) s_glyph[k] = glyphs[k];
    __syncthreads();
    {
        int pos = 0, total = 0;
        for (int k = 0; k < count; ++k) {
            const int f = s_flag[k];
            total += f;
            if (k < t) pos += f;
        }
        if (keep) s_rec[pos] = mine;
        if (t == 0) s_n = total;
    }
    __syncthreads();
    const int n = s_n;

    const unsigned char *plane = arena + it.offset;
    unsigned char *img = out + it.out_offset;
    const int xl = x0 + lane * PX;
    for (int rr = 0; rr < TILE_H / 4; ++rr) {
        const int y = y0 + rr * 4 + wave;
        const bool row_on = y < ye;
        unsigned int px[PX];                                                             // r | g << 8 | b << 16
        if (row_on) {
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const int x = xl + k;
                const unsigned int g = x < xe ? plane[(size_t)y * it.row_stride + x] : 0u;
                px[k] = g | (g << 8) | (g << 16);
            }
            for (int q = 0; q < n; ++q) {
                const Rec &r = s_rec[q];
                const int ox0 = r.x1 - hw, ox1 = r.x2 + hw, oy0 = r.y1 - hw, oy1 = r.y2 + hw;
                const unsigned int col = (unsigned int)r.r | ((unsigned int)r.g << 8) | ((unsigned int)r.b << 16);
                if (y >= oy0 && y <= oy1 && xl + PX > ox0 && xl <= ox1) {
                    const bool inner_y = y > r.y1 + hw && y < r.y2 - hw;
                    const bool horiz = abs(y - r.y1) <= hw || abs(y - r.y2) <= hw;
                    // dash phases as unsigned residues: of this lane's first pixel along x (xl may lie left of the
                    // outline: brought into 0 .. period-1 first), of the row along y (y >= oy0 here)
                    const unsigned int up = (unsigned int)period;
                    const unsigned int phx = (unsigned int)(((xl - ox0) % period + period) % period);
                    const bool y_lit = (unsigned int)(y - oy0) % up < (unsigned int)st.dash_on;
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const int x = xl + k;
                        const bool outside = x < ox0 || x > ox1;
                        const bool inside = inner_y && x > r.x1 + hw && x < r.x2 - hw;
                        const bool x_lit = (phx + (unsigned int)k) % up < (unsigned int)st.dash_on;
                        const bool lit = !r.kind || (horiz ? x_lit : y_lit);
                        if (!outside && !inside && lit) px[k] = col;
                    }
                }
                if (r.kind) {
                    int tx0, ty0, tx1, ty1;
                    tag_rect(r, st, tx0, ty0, tx1, ty1);
                    if (y >= ty0 && y < ty1 && xl + PX > tx0 && xl < tx1) {
                        const int gs = st.glyph_scale, dy = y - (ty0 + st.tag_pad);
                        const int wt = (int)r.nchars * 6 * gs - gs;
                        const bool text_row = dy >= 0 && dy < 7 * gs;
                        const int grow = text_row ? dy / gs : 0;
#pragma unroll
                        for (int k = 0; k < PX; ++k) {
                            const int x = xl + k;
                            if (x < tx0 || x >= tx1) continue;
                            const unsigned int o = px[k];
                            unsigned int v = 0;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const unsigned int oc = (o >> (8 * c)) & 0xffu, cc = (col >> (8 * c)) & 0xffu;
                                v |= ((oc + cc + 1u) >> 1) << (8 * c);
                            }
                            const int dx = x - (tx0 + st.tag_pad);
                            if (text_row && dx >= 0 && dx < wt) {
                                const int ci = dx / (6 * gs), cx = (dx - ci * 6 * gs) / gs;
                                const int gi = r.text[ci];
                                if (cx < 5 && gi < n_glyphs && ((s_glyph[gi * 7 + grow] >> (4 - cx)) & 1)) v = 0xffffffu;
                            }
                            px[k] = v;
                        }
                    }
                }
            }
            // 12 bytes of this lane -> 3 dwords of the wave's row buffer
            s_row[wave][lane * 3] = (px[0] & 0xffffffu) | (px[1] << 24);
            s_row[wave][lane * 3 + 1] = ((px[1] >> 8) & 0xffffu) | (px[2] << 16);
            s_row[wave][lane * 3 + 2] = ((px[2] >> 16) & 0xffu) | (px[3] << 8);
        }
        __syncthreads();
        if (row_on) {
            const unsigned char *src = reinterpret_cast<const unsigned char *>(s_row[wave]);
            unsigned char *dst = img + ((size_t)y * w + x0) * 3;
            const int nbytes = (xe - x0) * 3;
            const int head = min(nbytes, (int)((4u - (unsigned int)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
            const int nd = (nbytes - head) >> 2, tail0 = head + nd * 4;
            if (lane < head) dst[lane] = src[lane];
            unsigned int *dst4 = reinterpret_cast<unsigned int *>(dst + head);           // 4-aligned by construction
            for (int d = lane; d < nd; d += 64) {
                const unsigned char *s = src + head + d * 4;
                dst4[d] = (unsigned int)s[0] | ((unsigned int)s[1] << 8) | ((unsigned int)s[2] << 16) | ((unsigned int)s[3] << 24);
            }
            if (lane < nbytes - tail0) dst[tail0 + lane] = src[tail0 + lane];
        }
        __syncthreads();
    }
}

struct Workspace {
    int *n_recs;
    Rec *recs;
    size_t bytes;
};

Workspace carve(void *p, int N) {
    Carver c(p);
    Workspace w;
    w.n_recs = c.take<int>((size_t)N);
    w.recs = c.take<Rec>((size_t)N * MAX_ITEMS);
    w.bytes = c.off;
    return w;
}

bool style_ok(const Style &s) {
    return s.line_width >= 1 && s.line_width <= 15 && (s.line_width & 1) && s.dash_on >= 1 && s.dash_on <= 255 && s.dash_off >= 0 &&
           s.dash_off <= 255 && s.glyph_scale >= 1 && s.glyph_scale <= 4 && s.tag_pad >= 0 && s.tag_pad <= 15 && s.tag_dy >= 0 &&
           s.tag_dy <= 64 && s.max_draw >= 0 && s.max_draw <= MAX_DETS && s.vis_thresh == s.vis_thresh;
}

}  // namespace
}  // namespace wssdl

using namespace wssdl;

extern "C" size_t wssdl_draw_workspace_bytes(int N) {
    if (N < 1 || N > 65535) return 0;
    return carve(nullptr, N).bytes;
}

extern "C" int wssdl_draw_detections(const uint8_t *arena, size_t arena_bytes, const wssdl_draw_item *items_host,
                                     const wssdl_draw_item *items_dev, int N, const float *gt_boxes, const int32_t *gt_classes,
                                     const int32_t *gt_image_offsets_host, const int32_t *gt_image_offsets_dev, int G,
                                     const float *dets, const int32_t *counts, int K, int P, const uint8_t *colours,
                                     const uint8_t *glyphs, int n_glyphs, const uint8_t *labels, const wssdl_draw_style *style,
                                     uint8_t *out, size_t out_bytes, void *workspace, size_t workspace_bytes,
                                     wssdl_stream_t stream) {
    // host arithmetic on the arguments and the two host tables only: a rejected call has launched nothing
    if (N < 1 || N > 65535 || K < 2 || K > 65 || G < 0 || P < 0) return WSSDL_ERR_INVALID_ARGUMENT;
    if (n_glyphs < WSSDL_DRAW_MIN_GLYPHS || n_glyphs > 254) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!arena || !items_host || !items_dev || !gt_image_offsets_host || !gt_image_offsets_dev || !counts || !colours || !glyphs ||
        !labels || !style || !out)
        return WSSDL_ERR_INVALID_ARGUMENT;
    if ((G > 0 && (!gt_boxes || !gt_classes)) || (P > 0 && !dets)) return WSSDL_ERR_INVALID_ARGUMENT;
    const Style st = *style;
    if (!style_ok(st) || (long long)(K - 1) * st.max_draw > MAX_DETS) return WSSDL_ERR_INVALID_ARGUMENT;
    if (gt_image_offsets_host[0] != 0 || gt_image_offsets_host[N] != G) return WSSDL_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < N; ++i) {
        const long long g = (long long)gt_image_offsets_host[i + 1] - gt_image_offsets_host[i];
        if (g < 0 || g > MAX_GT) return WSSDL_ERR_INVALID_ARGUMENT;
    }
    long long max_tiles = 0;
    std::vector<std::pair<uint64_t, uint64_t>> spans((size_t)N);                         // (first byte, one past the last) of every output image
    for (int i = 0; i < N; ++i) {
        const Item &it = items_host[i];
        if (it.h < 1 || it.w < 1 || it.row_stride < it.w) return WSSDL_ERR_INVALID_ARGUMENT;
        if (it.offset < 0 || (uint64_t)it.offset > arena_bytes) return WSSDL_ERR_INVALID_ARGUMENT;
        const uint64_t extent = (uint64_t)(it.h - 1) * (uint64_t)it.row_stride + (uint64_t)it.w;
        if (extent > arena_bytes - (uint64_t)it.offset) return WSSDL_ERR_INVALID_ARGUMENT;
        if (it.out_offset < 0 || (uint64_t)it.out_offset > out_bytes) return WSSDL_ERR_INVALID_ARGUMENT;
        const uint64_t obytes = (uint64_t)it.h * (uint64_t)it.w * 3u;
        if (obytes > out_bytes - (uint64_t)it.out_offset) return WSSDL_ERR_INVALID_ARGUMENT;
        spans[i] = std::make_pair((uint64_t)it.out_offset, (uint64_t)it.out_offset + obytes);
        const long long tiles = (long long)cdiv(it.w, TILE_W) * cdiv(it.h, TILE_H);
        if (tiles > 0x7fffffffLL) return WSSDL_ERR_INVALID_ARGUMENT;
        max_tiles = std::max(max_tiles, tiles);
    }
    std::sort(spans.begin(), spans.end());
    for (int i = 1; i < N; ++i)
        if (spans[i].first < spans[i - 1].second) return WSSDL_ERR_INVALID_ARGUMENT;     // output images overlap
    const Workspace ws = carve(workspace, N);
    if (!workspace || workspace_bytes < ws.bytes) return WSSDL_ERR_WORKSPACE;

    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(draw_build_kernel, dim3(N), dim3(MAX_ITEMS), 0, s, items_dev, gt_boxes, gt_classes, gt_image_offsets_dev, G, dets,
                       counts, K, P, colours, labels, st, ws.n_recs, ws.recs);
    hipLaunchKernelGGL(draw_paint_kernel, dim3((unsigned)max_tiles, N), dim3(256), 0, s, arena, items_dev, ws.n_recs, ws.recs, glyphs,
                       n_glyphs, st, out);
    return check_launch();
}
