// RPN proposal recall on the device: the greedy proposal-to-ground-truth matching of the reference's
// imdb.evaluate_recall (code/lib/datasets/imdb.py:151-213) for every (area range, limit) cell of the recall table
// in one call.
//
// The reference, per image, per area range and per limit: take the ground-truth boxes whose area lies in the range,
// the first `limit` candidate boxes, the f64 IoU matrix of the two, and G_valid rounds of
//   column maximum per gt over the boxes (argmax(axis=0): lowest box index among equal maxima),
//   the gt with the largest column maximum (argmax(): lowest gt index among equal maxima),
//   record that overlap, set the box's row and the gt's column to -1.
// It recomputes the matrix for every cell.  Here
//   recall_iou_kernel     writes the [G_i, count_i] f64 IoU matrix of every image ONCE into the workspace (gt-major:
//                         a column of the reference's matrix is contiguous, lanes walk it coalesced); the area range
//                         masks its columns and the limit cuts its rows, so every cell reads the same values;
//   recall_match_kernel   one workgroup per (image, area range, limit): the column maxima (value, lowest box index)
//                         are found once by wave-64 reductions and kept in LDS; a round picks the best unused gt
//                         (wave 0), marks gt and box used, and recomputes ONLY the columns whose maximum sat on the box
//                         that was just taken -- a column's (max, first argmax) over the unused boxes does not change
//                         when another box leaves.  Records go out in round order; `overlap >= threshold` counts,
//                         the cell's num_pos and its flag are integer atomics whose result does not depend on the
//                         order of arrival, so two runs give the same bits.
// An image with fewer usable boxes than valid gts (the reference's assert(gt_ovr >= 0)) runs out of boxes: the rounds
// that find none record box -1 / overlap -1 and raise the cell's flag; nothing is read or written out of range.
// Latency-bound at test sizes (300 boxes x 1-3 gts per image): see DESIGN.md.
#include <math.h>

#include "box_iou.hip.h"

namespace wssdl {
namespace {

constexpr int MATCH_THREADS = 256, MATCH_WAVES = MATCH_THREADS / WSSDL_WAVE;
constexpr int MAX_GT = WSSDL_RECALL_MAX_GT, MAX_BOXES = WSSDL_RECALL_MAX_BOXES;

struct Candidates {
    const float *f32;           // first coordinate of row 0 of image 0, or null
    const float *scale;         // [N] or null
    const double *f64;          // or null
    int row_stride;             // elements between rows; an image is P rows
};

__device__ __forceinline__ void load_box(const Candidates &c, int i, int p, int P, double b[4]) {
    const size_t row = ((size_t)i * P + p) * c.row_stride;
    if (c.f32) {
        const float *r = c.f32 + row;
        if (c.scale) {
            const float s = c.scale[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = (double)__fdiv_rn(r[k], s);   // f32 IEEE division, then widened
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = (double)r[k];
        }
    } else {
        const double *r = c.f64 + row;
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = r[k];
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ov[(g0 + g) * P + p] for p < count_i: grid (N, cdiv(P, 256))
__global__ __launch_bounds__(256) void recall_iou_kernel(Candidates cand, const int *__restrict__ counts, int P,
                                                         const double *__restrict__ gt_boxes, const int *__restrict__ gt_off,
                                                         int Gtot, double *__restrict__ ov) {
    const int i = blockIdx.x, p = blockIdx.y * blockDim.x + threadIdx.x;
    if (p >= clampi(counts[i], 0, P)) return;
    const int g0 = clampi(gt_off[i], 0, Gtot), g1 = clampi(gt_off[i + 1], g0, Gtot);
    double b[4];
    load_box(cand, i, p, P, b);
    for (int g = g0; g < g1; ++g) {
        const double *q = gt_boxes + (size_t)g * 4;
        const double qarea = box_area_f64(q[0], q[1], q[2], q[3]);
        ov[(size_t)g * P + p] = iou_pair(b[0], b[1], b[2], b[3], q[0], q[1], q[2], q[3], qarea);
    }
}

// (max, lowest index among equal maxima) of one column over the unused boxes 0 .. n-1, by one wave; the result is
// valid in lane 0.  No unused box: (-1, -1).
__device__ __forceinline__ void column_max(const double *__restrict__ col, int n, const unsigned int *s_box_used, int lane,
                                           double *val, int *idx) {
    double best = -1.0;
    int bi = -1;
    for (int p = lane; p < n; p += WSSDL_WAVE) {
        if ((s_box_used[p >> 5] >> (p & 31)) & 1u) continue;
        const double v = col[p];
        if (v > best || bi < 0) { best = v;  bi = p; }      // ascending p: the first maximum stays
    }
#pragma unroll
    for (int off = WSSDL_WAVE / 2; off; off >>= 1) {
        const double ov = __shfl_down(best, off, WSSDL_WAVE);
        const int oi = __shfl_down(bi, off, WSSDL_WAVE);
        if (oi >= 0 && (bi < 0 || ov > best || (ov == best && oi < bi))) { best = ov;  bi = oi; }
    }
    *val = bi >= 0 ? best : -1.0;
    *idx = bi;
}

__global__ __launch_bounds__(MATCH_THREADS) void recall_match_kernel(
    const double *__restrict__ ov, const int *__restrict__ counts, int P, const double *__restrict__ gt_areas,
    const int *__restrict__ gt_off, int Gtot, const double *__restrict__ area_ranges, int A, const int *__restrict__ limits, int L,
    const double *__restrict__ thresholds, int T, int *__restrict__ hits, int *__restrict__ num_pos, int *__restrict__ flags,
    int *__restrict__ match_gt, int *__restrict__ match_box, double *__restrict__ match_ov) {
    __shared__ int s_vg[MAX_GT];                    // valid gts of the cell, ascending (index within the image)
    __shared__ double s_cm_val[MAX_GT];             // column maximum over the unused boxes
    __shared__ int s_cm_idx[MAX_GT];                // its box (lowest index), -1: no unused box
    __shared__ double s_rec[MAX_GT];                // recorded overlaps, round order
    __shared__ unsigned char s_gt_used[MAX_GT];
    __shared__ unsigned int s_box_used[MAX_BOXES / 32];
    __shared__ int s_nv, s_sel_box;

    const int cell = blockIdx.x % (A * L), i = blockIdx.x / (A * L);
    const int a = cell / L, l = cell - a * L;
    const int tid = threadIdx.x, lane = tid & (WSSDL_WAVE - 1), wave = tid / WSSDL_WAVE;
    const int g0 = clampi(gt_off[i], 0, Gtot), g1 = clampi(gt_off[i + 1], g0, Gtot);
    const int G = min(g1 - g0, MAX_GT);
    const double lo = area_ranges[a * 2], hi = area_ranges[a * 2 + 1];
    const int count = clampi(counts[i], 0, min(P, MAX_BOXES)), limit = limits[l];
    const int n = (limit > 0 && count > limit) ? limit : count;          // imdb.py:173-176
    const size_t out0 = (size_t)cell * Gtot + g0;

    if (tid == 0) {                                                       // imdb.py:161-164 (G <= 1024: one thread, in order)
        int nv = 0;
        for (int g = 0; g < G; ++g) {
            const double ar = gt_areas[g0 + g];
            if (ar >= lo && ar <= hi) s_vg[nv++] = g;
        }
        s_nv = nv;
        if (nv) atomicAdd(&num_pos[cell], nv);
    }
    for (int w = tid; w < (n + 31) / 32; w += MATCH_THREADS) s_box_used[w] = 0u;
    __syncthreads();
    const int nv = s_nv, rounds = n > 0 ? nv : 0;                         // no boxes: counted in num_pos only
    for (int k = tid; k < nv; k += MATCH_THREADS) s_gt_used[k] = 0;
    // slots of this image the rounds do not fill
    for (int g = rounds + tid; g < g1 - g0; g += MATCH_THREADS) {
        if (match_gt) match_gt[out0 + g] = -1;
        if (match_box) match_box[out0 + g] = -1;
        if (match_ov) match_ov[out0 + g] = -1.0;
    }
    if (rounds == 0) return;

    for (int k = wave; k < nv; k += MATCH_WAVES) {
        double v;
        int b;
        column_max(ov + (size_t)(g0 + s_vg[k]) * P, n, s_box_used, lane, &v, &b);
        if (lane == 0) { s_cm_val[k] = v;  s_cm_idx[k] = b; }
    }
    __syncthreads();

    for (int r = 0; r < rounds; ++r) {
        if (wave == 0) {
            // max_overlaps.argmax(): the best unused gt, lowest index among equal maxima (every unused gt is a
            // candidate, also at -1 when the boxes have run out)
            double best = -2.0;
            int bk = -1;
            for (int k = lane; k < nv; k += WSSDL_WAVE) {
                if (s_gt_used[k]) continue;
                const double v = s_cm_val[k];
                if (bk < 0 || v > best) { best = v;  bk = k; }
            }
#pragma unroll
            for (int off = WSSDL_WAVE / 2; off; off >>= 1) {
                const double ovv = __shfl_down(best, off, WSSDL_WAVE);
                const int ok = __shfl_down(bk, off, WSSDL_WAVE);
                if (ok >= 0 && (bk < 0 || ovv > best || (ovv == best && ok < bk))) { best = ovv;  bk = ok; }
            }
            if (lane == 0) {                                              // bk >= 0: r < nv unused gts remain
                const int b = s_cm_idx[bk];
                s_gt_used[bk] = 1;
                s_rec[r] = best;
                s_sel_box = b;
                if (b >= 0) s_box_used[b >> 5] |= 1u << (b & 31);
                else atomicAdd(&flags[cell], 1);                          // the reference's assert(gt_ovr >= 0)
                if (match_gt) match_gt[out0 + r] = s_vg[bk];
                if (match_box) match_box[out0 + r] = b;
                if (match_ov) match_ov[out0 + r] = best;
            }
        }
        __syncthreads();
        const int b = s_sel_box;
        if (b >= 0) {
            for (int k = wave; k < nv; k += MATCH_WAVES) {
                if (s_gt_used[k] || s_cm_idx[k] != b) continue;           // (uniform over the wave)
                double v;
                int nb;
                column_max(ov + (size_t)(g0 + s_vg[k]) * P, n, s_box_used, lane, &v, &nb);
                if (lane == 0) { s_cm_val[k] = v;  s_cm_idx[k] = nb; }
            }
        }
        __syncthreads();
    }
    for (int t = tid; t < T; t += MATCH_THREADS) {                        // imdb.py:208-209
        const double thr = thresholds[t];
        int c = 0;
        for (int r = 0; r < rounds; ++r) c += s_rec[r] >= thr;
        if (c) atomicAdd(&hits[(size_t)cell * T + t], c);
    }
}

struct Workspace {
    double *ov;
    int *gt_off;
    size_t bytes;
};

Workspace carve(void *p, int N, int P, int Gtot) {
    Carver c(p);
    Workspace w;
    w.ov = c.take<double>((size_t)Gtot * (size_t)P);
    w.gt_off = c.take<int>((size_t)N + 1);
    w.bytes = c.off + 256;
    return w;
}

bool sizes_ok(int N, int P, int Gtot) { return N >= 0 && P >= 0 && P <= MAX_BOXES && Gtot >= 0; }

#define RECALL_CHECK(call)                                 \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) {                            \
            set_last_error(e_);                            \
            return WSSDL_ERR_LAUNCH;                       \
        }                                                  \
    } while (0)

}  // namespace
}  // namespace wssdl

using namespace wssdl;

extern "C" {

size_t wssdl_proposal_recall_workspace_bytes(int N, int P, int Gtot) {
    if (!sizes_ok(N, P, Gtot)) return 0;                                  // (pure host: sizes only)
    return carve(nullptr, N, P, Gtot).bytes;
}

int wssdl_proposal_recall(const float *boxes_f32, const float *scale, const double *boxes_f64, int row_stride,
                          const int32_t *counts, int N, int P, const double *gt_boxes, const double *gt_areas,
                          const int32_t *gt_image_offsets_host, int Gtot, const double *area_ranges, int A,
                          const int32_t *limits, int L, const double *thresholds, int T, int32_t *hits, int32_t *num_pos,
                          int32_t *flags, int32_t *match_gt, int32_t *match_box, double *match_ov, void *workspace,
                          size_t workspace_bytes, wssdl_stream_t stream) {
    // every check below is host arithmetic on the arguments: a rejected call has touched neither the device nor
    // the runtime
    if (!sizes_ok(N, P, Gtot) || A < 1 || L < 1 || T < 1 || row_stride < 4) return WSSDL_ERR_INVALID_ARGUMENT;
    if ((long long)A * L > 0x7fffffffLL || (long long)A * L * T > 0x7fffffffLL || (long long)A * L * (N > 0 ? N : 1) > 0x7fffffffLL)
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (!gt_image_offsets_host || !area_ranges || !limits || !thresholds || !hits || !num_pos || !flags) return WSSDL_ERR_INVALID_ARGUMENT;
    if (gt_image_offsets_host[0] != 0 || gt_image_offsets_host[N] != Gtot) return WSSDL_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < N; ++i) {
        const long long g = (long long)gt_image_offsets_host[i + 1] - gt_image_offsets_host[i];
        if (g < 0 || g > MAX_GT) return WSSDL_ERR_INVALID_ARGUMENT;
    }
    if ((boxes_f32 != nullptr) == (boxes_f64 != nullptr) && (boxes_f32 || (N > 0 && P > 0))) return WSSDL_ERR_INVALID_ARGUMENT;
    if (scale && !boxes_f32) return WSSDL_ERR_INVALID_ARGUMENT;
    if (N > 0 && !counts) return WSSDL_ERR_INVALID_ARGUMENT;
    if (Gtot > 0 && (!gt_boxes || !gt_areas)) return WSSDL_ERR_INVALID_ARGUMENT;
    const Workspace w = carve(workspace, N, P, Gtot);
    if (!workspace || workspace_bytes < w.bytes) return WSSDL_ERR_INVALID_ARGUMENT;

    hipStream_t st = as_stream(stream);
    const size_t cells = (size_t)A * L;
    RECALL_CHECK(hipMemsetAsync(hits, 0, sizeof(int) * cells * T, st));
    RECALL_CHECK(hipMemsetAsync(num_pos, 0, sizeof(int) * cells, st));
    RECALL_CHECK(hipMemsetAsync(flags, 0, sizeof(int) * cells, st));
    if (N == 0) return WSSDL_OK;
    RECALL_CHECK(hipMemcpyAsync(w.gt_off, gt_image_offsets_host, sizeof(int) * ((size_t)N + 1), hipMemcpyHostToDevice, st));
    if (Gtot > 0 && P > 0) {
        const Candidates cand{boxes_f32, scale, boxes_f64, row_stride};
        hipLaunchKernelGGL(recall_iou_kernel, dim3(N, cdiv(P, 256)), dim3(256), 0, st, cand, counts, P, gt_boxes, w.gt_off, Gtot, w.ov);
    }
    if (Gtot > 0)
        hipLaunchKernelGGL(recall_match_kernel, dim3((unsigned)(cells * N)), dim3(MATCH_THREADS), 0, st, w.ov, counts, P, gt_areas, w.gt_off,
                           Gtot, area_ranges, A, limits, L, thresholds, T, hits, num_pos, flags, match_gt, match_box, match_ov);
    return check_launch();
}

}  // extern "C"
