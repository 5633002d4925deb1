// RoIAlign (cfg.ROI_POOL_MODE = 'align'): axis tables, forward, owner-cell backward.  include/wssdl_bus_hip.h states
// the semantics; DESIGN.md "RoIAlign" the structure, the summation order and the bytes.
//
// RoIAlign is separable: top_r = Ay . F_n . Ax^T / S^2 with at most 2 S non-zeros per bin and axis, so all of a RoI's
// geometry is two small tables (wssdl_roi_align_tables) and neither the forward nor the backward does any coordinate
// arithmetic.  The backward is the transpose as a GATHER -- float atomics would move ~27 GB at the training size and
// are not reproducible -- one wave owns a row of four cells of the map and 64 channel vectors, walks the RoIs that touch
// its 4 x 4 tile in ascending order and stores each cell once.
#include "common.hip.h"
#include "roi_pool.hip.h"

namespace wssdl {
namespace {

constexpr int ALIGN_MAX_POOLED = 16, ALIGN_MAX_SAMPLING = 4;
constexpr int TILE_H = 4, TILE_W = 4;          // cells per list tile; one workgroup owns it, one wave per row of 4 cells

// the nine arrays of the tables buffer (header: layout)
struct AlignTables {
    const int32_t *ylo, *yhi;
    const float *yh, *yl;
    const int32_t *xlo, *xhi;
    const float *xh, *xl;
    const int32_t *win;
};

inline size_t tables_elems(int R, int PH, int PW, int S) {
    return (size_t)R * ((size_t)4 * PH * S + (size_t)4 * PW * S + 5);
}

__host__ __device__ inline AlignTables carve_tables(const void *p, int R, int PH, int PW, int S) {
    const int32_t *b = static_cast<const int32_t *>(p);
    const size_t ny = (size_t)R * PH * S, nx = (size_t)R * PW * S;
    AlignTables t;
    t.ylo = b;
    t.yhi = b + ny;
    t.yh = reinterpret_cast<const float *>(b + 2 * ny);
    t.yl = reinterpret_cast<const float *>(b + 3 * ny);
    b += 4 * ny;
    t.xlo = b;
    t.xhi = b + nx;
    t.xh = reinterpret_cast<const float *>(b + 2 * nx);
    t.xl = reinterpret_cast<const float *>(b + 3 * nx);
    t.win = b + 4 * nx;
    return t;
}

// One thread per (RoI, axis): the P * S entries of that axis in order, and the range of cells they read.
__global__ __launch_bounds__(256) void roi_align_tables_kernel(const float *__restrict__ rois, int R, int N, int H, int W,
                                                               int PH, int PW, float scale, int S, int aligned,
                                                               int32_t *__restrict__ tables) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= 2 * R) return;
    const int r = id >> 1, axis = id & 1;                     // 0: y, 1: x
    const AlignTables t = carve_tables(tables, R, PH, PW, S);
    const float *roi = rois + (size_t)r * 5;
    const float b = roi[0];
    bool live = b >= 0.0f && b < (float)N;
    for (int k = 0; k < 5; ++k) live = live && isfinite(roi[k]);
    const int P = axis ? PW : PH, L = axis ? W : H;
    const size_t base = (size_t)r * P * S;
    int32_t *lo_out = const_cast<int32_t *>(axis ? t.xlo : t.ylo) + base;
    int32_t *hi_out = const_cast<int32_t *>(axis ? t.xhi : t.yhi) + base;
    float *h_out = const_cast<float *>(axis ? t.xh : t.yh) + base;
    float *l_out = const_cast<float *>(axis ? t.xl : t.yl) + base;
    const float off = aligned ? 0.5f : 0.0f;
    const float s = roi[axis ? 1 : 2] * scale - off;
    const float e = roi[axis ? 3 : 4] * scale - off;
    float len = e - s;
    if (!aligned) len = fmaxf(len, 1.0f);
    const float bin = len / (float)P;
    int first = L, last = -1;
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < S; ++i) {
            float y = (s + (float)p * bin) + (((float)i + 0.5f) * bin) / (float)S;
            int lo = 0, hi = 0;
            float wh = 0.0f, wl = 0.0f;
            if (live && y >= -1.0f && y <= (float)L) {          // (a NaN is void as well: nothing is read for it)
                if (y <= 0.0f) y = 0.0f;
                lo = (int)y;
                if (lo >= L - 1) {
                    lo = hi = L - 1;
                    y = (float)lo;
                } else {
                    hi = lo + 1;
                }
                wl = y - (float)lo;
                wh = 1.0f - wl;
                first = min(first, lo);
                last = max(last, hi);
            }
            lo_out[p * S + i] = lo;
            hi_out[p * S + i] = hi;
            h_out[p * S + i] = wh;
            l_out[p * S + i] = wl;
        }
    int32_t *win = const_cast<int32_t *>(t.win) + (size_t)r * 5;
    if (axis == 0) win[0] = live ? (int)b : -1;
    win[1 + 2 * axis] = first;
    win[2 + 2 * axis] = last;
}

template <typename V>
__device__ __forceinline__ V load_vec(const float *p) { return *reinterpret_cast<const V *>(p); }

// One wave per (RoI, bin row) and slice of 64 channel vectors; a lane owns one channel vector and walks the bins of the
// row, so the wave lies along C: 64 lanes x 16 bytes of one cell per load.  All table entries are uniform over the
// wave.  The slices are the slow index of the grid: what is in flight reads one image's 256-channel slice (2.4 MB at the
// training size, against 4 MB of L2 per chiplet) instead of the whole image.  Per output:
// acc += (wy*wx)*v over the samples (i, j) in order and the cells (lo,lo) (lo,hi) (hi,lo) (hi,hi); then acc / (S*S).
// Neighbouring samples of a row read overlapping columns (a bin is seldom wider than two cells): per sample row i the
// lane keeps the last two columns it loaded -- both map rows of that sample -- and loads a column only when it is
// neither.  The values and their order are those of the plain loop: the same bits, well under half the loads.
template <typename V, int S>
__global__ __launch_bounds__(256) void roi_align_forward_kernel(const float *__restrict__ bottom, int H, int W, int C, int R,
                                                                int PH, int PW, AlignTables t, float *__restrict__ top) {
    constexpr int VEC = sizeof(V) / sizeof(float);
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= R * PH) return;
    const int r = row / PH, ph = row % PH;
    const int CV = C / VEC;
    const int n = t.win[(size_t)r * 5];
    const size_t ybase = ((size_t)r * PH + ph) * S;
    const float samples = (float)(S * S);
    float *out_row = top + ((size_t)r * PH + ph) * PW * C;
    float yh[S], yl[S];
    size_t row_lo[S], row_hi[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        yh[i] = t.yh[ybase + i];
        yl[i] = t.yl[ybase + i];
        row_lo[i] = (size_t)t.ylo[ybase + i] * W * C;
        row_hi[i] = (size_t)t.yhi[ybase + i] * W * C;
    }
    const int cv = blockIdx.y * 64 + (threadIdx.x & 63);
    if (cv < CV) {
        const float *img = bottom + (size_t)(n < 0 ? 0 : n) * H * W * C + (size_t)cv * VEC;
        int col[S][2];                                    // the two columns held for sample row i, -1: none
        V held_lo[S][2], held_hi[S][2];                   // their values on the sample's two map rows
#pragma unroll
        for (int i = 0; i < S; ++i) col[i][0] = col[i][1] = -1;
        for (int pw = 0; pw < PW; ++pw) {
            V acc = (V)(0.0f);
            if (n >= 0) {
                const size_t xbase = ((size_t)r * PW + pw) * S;
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    if (yh[i] == 0.0f && yl[i] == 0.0f) continue;             // void along y
#pragma unroll
                    for (int j = 0; j < S; ++j) {
                        const float xh = t.xh[xbase + j], xl = t.xl[xbase + j];
                        if (xh == 0.0f && xl == 0.0f) continue;               // void along x
                        const int xlo = t.xlo[xbase + j], xhi = t.xhi[xbase + j];
                        V v00, v10, v01, v11;
                        if (xlo == col[i][0]) {
                            v00 = held_lo[i][0];
                            v10 = held_hi[i][0];
                        } else if (xlo == col[i][1]) {
                            v00 = held_lo[i][1];
                            v10 = held_hi[i][1];
                        } else {
                            v00 = load_vec<V>(img + row_lo[i] + (size_t)xlo * C);
                            v10 = load_vec<V>(img + row_hi[i] + (size_t)xlo * C);
                        }
                        if (xhi == xlo) {
                            v01 = v00;
                            v11 = v10;
                        } else if (xhi == col[i][1]) {
                            v01 = held_lo[i][1];
                            v11 = held_hi[i][1];
                        } else if (xhi == col[i][0]) {
                            v01 = held_lo[i][0];
                            v11 = held_hi[i][0];
                        } else {
                            v01 = load_vec<V>(img + row_lo[i] + (size_t)xhi * C);
                            v11 = load_vec<V>(img + row_hi[i] + (size_t)xhi * C);
                        }
                        col[i][0] = xlo;
                        held_lo[i][0] = v00;
                        held_hi[i][0] = v10;
                        col[i][1] = xhi;
                        held_lo[i][1] = v01;
                        held_hi[i][1] = v11;
                        acc += (yh[i] * xh) * v00;
                        acc += (yh[i] * xl) * v01;
                        acc += (yl[i] * xh) * v10;
                        acc += (yl[i] * xl) * v11;
                    }
                }
                acc = acc / samples;
            }
            // top is written once and never read again here: keep it out of the caches the feature map lives in
            __builtin_nontemporal_store(acc, reinterpret_cast<V *>(out_row + (size_t)pw * C + (size_t)cv * VEC));
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward lists ---
// workspace: offs i32 [N * tiles + 1] (256-byte slice), list i32 [R * tiles per image].  One wave per (image, tile)
// tests the RoIs 64 at a time in ascending order, so a tile's list is ascending by construction.
__device__ __forceinline__ bool touches(const int32_t *win, int r, int n, int h0, int h1, int w0, int w1) {
    const int32_t *q = win + (size_t)r * 5;
    return q[0] == n && q[1] <= h1 && q[2] >= h0 && q[3] <= w1 && q[4] >= w0;      // (an empty range fails one side)
}

template <bool FILL>
__global__ __launch_bounds__(256) void roi_align_lists_kernel(const int32_t *__restrict__ win, int R, int H, int W,
                                                              int tiles_h, int tiles_w, int total_tiles,
                                                              int32_t *__restrict__ offs, int32_t *__restrict__ list) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= total_tiles) return;
    const int tx = tile % tiles_w, ty = (tile / tiles_w) % tiles_h, n = tile / (tiles_w * tiles_h);
    const int h0 = ty * TILE_H, h1 = min(h0 + TILE_H, H) - 1, w0 = tx * TILE_W, w1 = min(w0 + TILE_W, W) - 1;
    int count = 0;
    const int base = FILL ? offs[tile] : 0;
    for (int r0 = 0; r0 < R; r0 += 64) {
        const int r = r0 + lane;
        const bool hit = r < R && touches(win, r, n, h0, h1, w0, w1);
        const unsigned long long m = __ballot(hit);
        if (FILL && hit) list[base + count + __popcll(m & ((1ull << lane) - 1ull))] = r;
        count += __popcll(m);
    }
    if (!FILL && lane == 0) offs[tile + 1] = count;        // counts, shifted by one: the scan below makes them offsets
}

// exclusive scan of the counts in place (one workgroup; integer sums: the same offsets on every run)
__global__ __launch_bounds__(256) void roi_align_scan_kernel(int32_t *__restrict__ offs, int total_tiles) {
    __shared__ int part[256];
    const int per = (total_tiles + 255) / 256;
    const int b = threadIdx.x * per, e = min(b + per, total_tiles);
    int s = 0;
    for (int i = b; i < e; ++i) s += offs[i + 1];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = part[i];
            part[i] = run;
            run += v;
        }
        offs[0] = 0;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = b; i < e; ++i) {
        run += offs[i + 1];
        offs[i + 1] = run;
    }
}

// ---------------------------------------------------------------------------------------------------- backward ---
struct AxisEntry {
    int lo, hi;
    float h, l;
};

__device__ __forceinline__ AxisEntry load_entry(const int32_t *lo, const int32_t *hi, const float *h, const float *l,
                                                size_t base, int lane, int count) {
    AxisEntry a = {0, 0, 0.0f, 0.0f};
    if (lane < count) {
        a.lo = lo[base + lane];
        a.hi = hi[base + lane];
        a.h = h[base + lane];
        a.l = l[base + lane];
    }
    return a;
}

// weight of cell `c` in the bin `lane` (lanes >= P: 0): the S entries of the bin in order, each (lo == c ? h : 0) +
// (hi == c ? l : 0).  Lane k holds entry k of the RoI's axis.
__device__ __forceinline__ float bin_weight(const AxisEntry &a, int c, int lane, int P, int S) {
    const float mine = (a.lo == c ? a.h : 0.0f) + (a.hi == c ? a.l : 0.0f);
    float wsum = 0.0f;
    for (int i = 0; i < S; ++i) wsum += __shfl(mine, (lane * S + i) & 63);
    return lane < P ? wsum : 0.0f;
}

// One wave per (row of a list tile = 4 cells, 64 channel vectors); a workgroup is one tile (4 waves) and one slice of
// channels.  The wave walks its tile's list 64 entries at a time (ascending), keeps the RoIs whose window touches its
// four cells, builds their weights once -- WY[ph] for its map row, WX[pw] for each of its four columns, 64 lanes = 64
// table entries -- and turns each RoI into its terms
//     (row of top_diff (r, ph, pw), WY[ph] * WX_c[pw] for the four cells c)      ph ascending, then pw ascending,
//                                                                                 bins with a non-zero weight in any cell
// which go into a queue in LDS (they are uniform over the wave: one lane writes, all lanes read).  The queue is drained
// eight terms at a time -- eight independent 16-byte loads per lane in flight, then acc_c += g * weight_c in queue order
// -- so a row of top_diff is loaded once for the cells of the row it touches, and the order of every cell's sum is the
// order of the terms: RoI, then ph, then pw, all ascending.  (A term whose weight for a cell is zero adds an exact zero
// there: the bits of a finite sum do not see it.)  Each cell is stored once, divided by S*S.  The next RoI's entries
// are loaded before the current one's terms are made.
constexpr int QUEUE_TERMS = 320, QUEUE_DRAIN_AT = 64, QUEUE_GROUP = 8;       // a RoI makes at most 16 x 16 = 256 terms

typedef float4v CellWeights;                                                 // one weight per cell of the row

template <typename V>
__global__ __launch_bounds__(256) void roi_align_backward_kernel(const float *__restrict__ top_diff, int H, int W, int C,
                                                                 int PH, int PW, int S, AlignTables t,
                                                                 const int32_t *__restrict__ offs,
                                                                 const int32_t *__restrict__ list, int tiles_h, int tiles_w,
                                                                 float *__restrict__ bottom_diff) {
    constexpr int VEC = sizeof(V) / sizeof(float);
    static_assert(TILE_W == 4 && TILE_H == 4, "four waves, four cells each");
    __shared__ int q_row[TILE_H][QUEUE_TERMS];
    __shared__ CellWeights q_weight[TILE_H][QUEUE_TERMS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Workgroup ids are dealt round-robin to the eight chiplets, each with an L2 of its own.  The remap gives a tile and
    // the tile beside it ids of one residue mod 8, close together, so the rows of top_diff they share meet in one L2.
    // 16 ids <-> 16 tiles, a bijection; the tiles past the last multiple of 16 keep the plain order.
    const int grouped = (int)(gridDim.x / 16) * 16;
    int tile = blockIdx.x;
    if (tile < grouped) tile = tile / 16 * 16 + tile % 8 * 2 + tile % 16 / 8;
    const int tx = tile % tiles_w, ty = (tile / tiles_w) % tiles_h, n = tile / (tiles_w * tiles_h);
    const int h = ty * TILE_H + wave, w0 = tx * TILE_W, w1 = min(w0 + TILE_W, W) - 1;
    if (h >= H) return;                                         // (whole waves: no workgroup barrier below)
    const int CV = C / VEC;
    const int cv = blockIdx.y * 64 + lane;
    const bool mine = cv < CV;
    const int ny = PH * S, nx = PW * S;
    const float *g_lane = top_diff + (size_t)(mine ? cv : 0) * VEC;
    int *rows = q_row[wave];
    CellWeights *weights = q_weight[wave];
    int queued = 0;
    V acc[TILE_W];
#pragma unroll
    for (int c = 0; c < TILE_W; ++c) acc[c] = (V)(0.0f);

    auto add = [&](const V &g, const CellWeights &cw) {
#pragma unroll
        for (int c = 0; c < TILE_W; ++c) acc[c] += g * cw[c];
    };
    // drains the queue in order: whole groups of eight, and the rest too when `all`; else the rest moves to the front
    auto drain = [&](bool all) {
        __builtin_amdgcn_wave_barrier();
        int k = 0;
        for (; k + QUEUE_GROUP <= queued; k += QUEUE_GROUP) {
            V g[QUEUE_GROUP];
#pragma unroll
            for (int u = 0; u < QUEUE_GROUP; ++u)
                g[u] = mine ? load_vec<V>(g_lane + (size_t)rows[k + u] * C) : (V)(0.0f);
#pragma unroll
            for (int u = 0; u < QUEUE_GROUP; ++u) add(g[u], weights[k + u]);
        }
        if (all) {
            for (; k < queued; ++k) {
                const V g = mine ? load_vec<V>(g_lane + (size_t)rows[k] * C) : (V)(0.0f);
                add(g, weights[k]);
            }
            queued = 0;
        } else {
            const int rest = queued - k;                        // < 8
            int row = 0;
            CellWeights cw = (CellWeights)(0.0f);
            if (lane < rest) {
                row = rows[k + lane];
                cw = weights[k + lane];
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < rest) {
                rows[lane] = row;
                weights[lane] = cw;
            }
            queued = rest;
        }
        __builtin_amdgcn_wave_barrier();
    };

    const int beg = offs[tile], end = offs[tile + 1];
    for (int k0 = beg; k0 < end; k0 += 64) {
        const int entry = k0 + lane < end ? list[k0 + lane] : -1;
        bool hit = false;
        if (entry >= 0) {
            const int32_t *win = t.win + (size_t)entry * 5;
            hit = win[1] <= h && h <= win[2] && win[3] <= w1 && w0 <= win[4];
        }
        unsigned long long todo = __ballot(hit);
        if (!todo) continue;
        int r = __builtin_amdgcn_readfirstlane(__shfl(entry, __ffsll((long long)todo) - 1));
        todo &= todo - 1;
        AxisEntry ey = load_entry(t.ylo, t.yhi, t.yh, t.yl, (size_t)r * ny, lane, ny);
        AxisEntry ex = load_entry(t.xlo, t.xhi, t.xh, t.xl, (size_t)r * nx, lane, nx);
        while (r >= 0) {
            int r_next = -1;
            AxisEntry ey_next = ey, ex_next = ex;
            if (todo) {
                r_next = __builtin_amdgcn_readfirstlane(__shfl(entry, __ffsll((long long)todo) - 1));
                todo &= todo - 1;
                ey_next = load_entry(t.ylo, t.yhi, t.yh, t.yl, (size_t)r_next * ny, lane, ny);
                ex_next = load_entry(t.xlo, t.xhi, t.xh, t.xl, (size_t)r_next * nx, lane, nx);
            }
            const float wy_lane = bin_weight(ey, h, lane, PH, S);
            float wx_lane[TILE_W];
            bool any_x = false;
#pragma unroll
            for (int c = 0; c < TILE_W; ++c) {
                wx_lane[c] = bin_weight(ex, w0 + c, lane, PW, S);
                any_x = any_x || wx_lane[c] != 0.0f;
            }
            unsigned long long my = __ballot(wy_lane != 0.0f);
            const unsigned long long mx = __ballot(any_x);
            const int row0 = r * PH * PW;
            while (my) {
                const int ph = __ffsll((long long)my) - 1;
                my &= my - 1;
                const float wy = __shfl(wy_lane, ph);
                unsigned long long m = mx;
                while (m) {
                    const int pw = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    CellWeights cw;
#pragma unroll
                    for (int c = 0; c < TILE_W; ++c) cw[c] = wy * __shfl(wx_lane[c], pw);
                    if (lane == 0) {
                        rows[queued] = row0 + ph * PW + pw;
                        weights[queued] = cw;
                    }
                    ++queued;
                }
            }
            if (queued >= QUEUE_DRAIN_AT) drain(false);
            r = r_next;
            ey = ey_next;
            ex = ex_next;
        }
    }
    drain(true);
    if (mine) {
#pragma unroll
        for (int c = 0; c < TILE_W; ++c)
            if (w0 + c < W)
                *reinterpret_cast<V *>(bottom_diff + (((size_t)n * H + h) * W + w0 + c) * C + (size_t)cv * VEC) =
                    acc[c] / (float)(S * S);
    }
}

template <typename V>
void launch_forward_v(int S, dim3 grid, dim3 block, hipStream_t st, const float *bottom, int H, int W, int C, int R, int PH, int PW,
                      const AlignTables &t, float *top) {
    switch (S) {
    case 1: hipLaunchKernelGGL((roi_align_forward_kernel<V, 1>), grid, block, 0, st, bottom, H, W, C, R, PH, PW, t, top); break;
    case 2: hipLaunchKernelGGL((roi_align_forward_kernel<V, 2>), grid, block, 0, st, bottom, H, W, C, R, PH, PW, t, top); break;
    case 3: hipLaunchKernelGGL((roi_align_forward_kernel<V, 3>), grid, block, 0, st, bottom, H, W, C, R, PH, PW, t, top); break;
    default: hipLaunchKernelGGL((roi_align_forward_kernel<V, 4>), grid, block, 0, st, bottom, H, W, C, R, PH, PW, t, top); break;
    }
}

void launch_forward(bool vec, int S, dim3 grid, dim3 block, hipStream_t st, const float *bottom, int H, int W, int C, int R,
                    int PH, int PW, const AlignTables &t, float *top) {
    if (vec) launch_forward_v<float4v>(S, grid, block, st, bottom, H, W, C, R, PH, PW, t, top);
    else launch_forward_v<float>(S, grid, block, st, bottom, H, W, C, R, PH, PW, t, top);
}

int invalid() {
    set_last_error(hipErrorInvalidValue);
    return WSSDL_ERR_INVALID_ARGUMENT;
}

bool bad_pooling(int PH, int PW, int S) {
    return PH < 1 || PH > ALIGN_MAX_POOLED || PW < 1 || PW > ALIGN_MAX_POOLED || S < 1 || S > ALIGN_MAX_SAMPLING;
}

inline int tiles_of(int L, int T) { return (L + T - 1) / T; }

// 16-byte channel vectors need C % 4 == 0 and 16-byte aligned tensors; anything else takes the plain path
bool vector_ok(int C, const void *a, const void *b) {
    return C % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0;
}

}  // namespace
}  // namespace wssdl

using namespace wssdl;

extern "C" size_t wssdl_roi_align_tables_bytes(int R, int pooled_h, int pooled_w, int sampling) {
    if (R < 0 || bad_pooling(pooled_h, pooled_w, sampling)) return 0;
    return tables_elems(R, pooled_h, pooled_w, sampling) * sizeof(int32_t);
}

extern "C" int wssdl_roi_align_tables(const float *rois, int R, int N, int H, int W, int pooled_h, int pooled_w,
                                      float spatial_scale, int sampling, int aligned, void *tables, size_t tables_bytes,
                                      wssdl_stream_t stream) {
    set_last_error(hipSuccess);
    if (R < 0 || N < 1 || H < 1 || W < 1 || bad_pooling(pooled_h, pooled_w, sampling) || (aligned != 0 && aligned != 1))
        return invalid();
    if (R == 0) return WSSDL_OK;
    if (!rois || !tables || tables_bytes < wssdl_roi_align_tables_bytes(R, pooled_h, pooled_w, sampling)) return invalid();
    if ((long long)R * 2 > 0x7fffffffLL) return invalid();
    hipLaunchKernelGGL(roi_align_tables_kernel, dim3(cdiv(2LL * R, 256)), dim3(256), 0, as_stream(stream), rois, R, N, H, W,
                       pooled_h, pooled_w, spatial_scale, sampling, aligned, static_cast<int32_t *>(tables));
    return check_launch();
}

extern "C" int wssdl_roi_align_forward(const float *bottom, int N, int H, int W, int C, int R, int pooled_h, int pooled_w,
                                       int sampling, const void *tables, size_t tables_bytes, float *top,
                                       wssdl_stream_t stream) {
    set_last_error(hipSuccess);
    if (R < 0 || N < 1 || H < 1 || W < 1 || C < 1 || bad_pooling(pooled_h, pooled_w, sampling)) return invalid();
    if (R == 0) return WSSDL_OK;
    if (!bottom || !tables || !top || tables_bytes < wssdl_roi_align_tables_bytes(R, pooled_h, pooled_w, sampling))
        return invalid();
    if ((long long)R * pooled_h > 0x7fffffffLL || (long long)pooled_w * C > 0x7fffffffLL) return invalid();
    const AlignTables t = carve_tables(tables, R, pooled_h, pooled_w, sampling);
    const bool vec = vector_ok(C, bottom, top);
    const long long slices = cdiv(vec ? C / 4 : C, 64);
    if (slices > 65535) return invalid();
    launch_forward(vec, sampling, dim3(cdiv((long long)R * pooled_h, 4), (unsigned)slices), dim3(256), as_stream(stream), bottom,
                   H, W, C, R, pooled_h, pooled_w, t, top);
    return check_launch();
}

extern "C" size_t wssdl_roi_align_backward_workspace_bytes(int R, int N, int H, int W) {
    if (R < 0 || N < 1 || H < 1 || W < 1) return 0;
    const size_t tiles = (size_t)tiles_of(H, TILE_H) * tiles_of(W, TILE_W);
    Carver c(nullptr);
    c.take<int32_t>((size_t)N * tiles + 1);
    c.take<int32_t>((size_t)R * tiles);
    return c.off;
}

namespace wssdl {
namespace {
// the shape limits the two backward calls share: tile and list counts are 32-bit in the kernels
bool backward_shape_ok(int R, int N, int H, int W) {
    const long long tiles = (long long)tiles_of(H, TILE_H) * tiles_of(W, TILE_W);
    return tiles * N <= 0x7fffffffLL && tiles * R <= 0x7fffffffLL;
}
}  // namespace
}  // namespace wssdl

extern "C" int wssdl_roi_align_backward_prepare(int R, int N, int H, int W, int pooled_h, int pooled_w, int sampling,
                                                const void *tables, size_t tables_bytes, void *workspace,
                                                size_t workspace_bytes, wssdl_stream_t stream) {
    set_last_error(hipSuccess);
    if (R < 0 || N < 1 || H < 1 || W < 1 || bad_pooling(pooled_h, pooled_w, sampling) || !backward_shape_ok(R, N, H, W))
        return invalid();
    if (R == 0) return WSSDL_OK;
    if (!tables || !workspace || tables_bytes < wssdl_roi_align_tables_bytes(R, pooled_h, pooled_w, sampling) ||
        workspace_bytes < wssdl_roi_align_backward_workspace_bytes(R, N, H, W))
        return invalid();
    const AlignTables t = carve_tables(tables, R, pooled_h, pooled_w, sampling);
    const int tiles_h = tiles_of(H, TILE_H), tiles_w = tiles_of(W, TILE_W), total = N * tiles_h * tiles_w;
    Carver c(workspace);
    int32_t *offs = c.take<int32_t>((size_t)total + 1);
    int32_t *list = c.take<int32_t>((size_t)R * tiles_h * tiles_w);
    const dim3 grid(cdiv(total, 4)), block(256);
    hipLaunchKernelGGL(roi_align_lists_kernel<false>, grid, block, 0, as_stream(stream), t.win, R, H, W, tiles_h, tiles_w,
                       total, offs, list);
    hipLaunchKernelGGL(roi_align_scan_kernel, dim3(1), block, 0, as_stream(stream), offs, total);
    hipLaunchKernelGGL(roi_align_lists_kernel<true>, grid, block, 0, as_stream(stream), t.win, R, H, W, tiles_h, tiles_w,
                       total, offs, list);
    return check_launch();
}

extern "C" int wssdl_roi_align_backward(const float *top_diff, int R, int N, int H, int W, int C, int pooled_h, int pooled_w,
                                        int sampling, const void *tables, size_t tables_bytes, const void *workspace,
                                        size_t workspace_bytes, float *bottom_diff, wssdl_stream_t stream) {
    set_last_error(hipSuccess);
    if (R < 0 || N < 1 || H < 1 || W < 1 || C < 1 || bad_pooling(pooled_h, pooled_w, sampling) ||
        !backward_shape_ok(R, N, H, W) || (long long)R * pooled_h * pooled_w > 0x7fffffffLL || !bottom_diff)
        return invalid();
    if (R == 0) {
        hipError_t e = hipMemsetAsync(bottom_diff, 0, (size_t)N * H * W * C * sizeof(float), as_stream(stream));
        if (e != hipSuccess) {
            set_last_error(e);
            return WSSDL_ERR_LAUNCH;
        }
        return WSSDL_OK;
    }
    if (!top_diff || !tables || !workspace || tables_bytes < wssdl_roi_align_tables_bytes(R, pooled_h, pooled_w, sampling) ||
        workspace_bytes < wssdl_roi_align_backward_workspace_bytes(R, N, H, W))
        return invalid();
    const AlignTables t = carve_tables(tables, R, pooled_h, pooled_w, sampling);
    const int tiles_h = tiles_of(H, TILE_H), tiles_w = tiles_of(W, TILE_W), total = N * tiles_h * tiles_w;
    Carver c(const_cast<void *>(workspace));
    const int32_t *offs = c.take<int32_t>((size_t)total + 1);
    const int32_t *list = c.take<int32_t>((size_t)R * tiles_h * tiles_w);
    const bool vec = vector_ok(C, top_diff, bottom_diff);
    const long long slices = cdiv(vec ? C / 4 : C, 64);
    if (slices > 65535) return invalid();
    const dim3 grid(total, (unsigned)slices), block(TILE_H * 64);
    if (vec)
        hipLaunchKernelGGL(roi_align_backward_kernel<float4v>, grid, block, 0, as_stream(stream), top_diff, H, W, C, pooled_h,
                           pooled_w, sampling, t, offs, list, tiles_h, tiles_w, bottom_diff);
    else
        hipLaunchKernelGGL(roi_align_backward_kernel<float>, grid, block, 0, as_stream(stream), top_diff, H, W, C, pooled_h,
                           pooled_w, sampling, t, offs, list, tiles_h, tiles_w, bottom_diff);
    return check_launch();
}
