// Detection evaluation on the device: AP (11-point and area), CorLoc and the FROC counts of every class and every
// score threshold from one pass over the detections (reference: datasets/voc_eval_bus.py, called 44 times per
// validation by datasets/bus.py:_do_python_eval -- each call re-reads two files and walks every detection in Python).
//
// For one class the reference's loop restates as
//   ovmax_d, jmax_d  over the class's ground-truth boxes of detection d's image (first maximum, like np.argmax),
//   hit_d = ovmax_d > ovthresh,
//   in descending confidence: a hit on a non-difficult box is TP when it is the first hit on that box, else FP;
//                             a hit on a difficult box is neither; a non-hit is FP,
//   nok(t)         = images that have a box of the class and max{conf_d : hit_d} >= t,
//   num_all_fps(t) = detections with not hit_d and conf_d >= t,
// so one overlap pass, one sort, one first-hit-per-box pass and one prefix sum serve every threshold:
//   eval_gt_kernel        classes present per image (a 64-bit mask), npos, ni
//   eval_keys_kernel      quantise, overlaps (f64, the reference's operation order), unique 64-bit sort keys,
//                         per-image maximum hit confidence (atomicMax) and false positives at the base threshold
//   eval_runs_kernel      sorted runs of 2048 keys (sort_and_store_run of order_sort.hip.h)
//   eval_merge_kernel     log2(runs) merge passes by rank: an element's place in the merged pair is its own offset
//                         plus the number of greater keys in the sibling block (keys are unique: no tie handling)
//   eval_first_kernel     atomicMin of the sorted rank into one word per ground-truth box
//   eval_scan_*           chip-wide integer prefix sums of tp / fp / non-hit over the sorted order (reduce, spine, scan)
//   eval_curves_kernel    order, tp, fp, rec, prec per class (class segments are contiguous in the sorted order)
//   eval_ap_kernel        one workgroup per class sweeps its segment backwards: suffix maximum of prec -> both APs
//   eval_thresholds_kernel nok, num_all_fps per (class, threshold); arr_ok at the base threshold
// Nothing is allocated, read back or synchronised; every atomic is an integer atomic whose result does not depend
// on the order of arrival, so two runs give the same bits.
//
// ORDER AMONG EQUAL SCORES.  The reference sorts with np.argsort(-confidence), an unstable introsort: where two
// detections of a class share a confidence, their order -- and with it tp / fp / rec / prec / ap -- is an accident
// of NumPy's implementation.  Here ties are broken by input order (image index, then rank within the image): the
// stable sort of the result file's lines.  The low bits of every key hold the complement of the input index.
//
// QUANTISATION (WSSDL_EVAL_QUANTISE).  The reference scores what it wrote to the result file: the score as
// '{:.3f}', each coordinate as '{:.1f}' of the f32 value x + 1 (bus.py:257-261).  The parsed doubles are reproduced
// exactly: double(s) * 1000.0 and double(x +f32 1.0f) * 10.0 are exact in f64 (24-bit x 10-bit significands), rint
// in round-half-even is Python's correctly rounded formatting of the exact binary value, and the correctly rounded
// f64 division by 1000.0 / 10.0 is the decimal parse of the printed digits.
#include <float.h>
#include <math.h>

#include "order_sort.hip.h"

namespace wssdl {
namespace {

typedef unsigned long long u64;

constexpr int IDX_BITS = 25, SCORE_SHIFT = IDX_BITS, CLASS_SHIFT = IDX_BITS + 32;
constexpr u64 IDX_MASK = (1ull << IDX_BITS) - 1;
constexpr long long MAX_SLOTS = 1ll << 24;
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 8, SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;
static_assert(SCAN_BLOCK == RUN, "the padded length is a multiple of both");
constexpr int AP_THREADS = 1024;

struct DetInput {
    int batched;
    const float *boxes, *scores;        // flat: [D,4], [D]
    const int *image, *cls;             // flat: [D], [D]
    const float *dets;                  // batched: [N, K-1, P, 5]
    const int *counts;                  // batched: [N, K-1]
    int N, P, first_image;
};

// order-preserving map of a double onto unsigned 64-bit integers (every real value maps above 0)
__device__ __forceinline__ u64 ordered_bits(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_ordered_bits(u64 o) {
    const u64 b = (o >> 63) ? (o & 0x7fffffffffffffffull) : ~o;
    return __longlong_as_double((long long)b);
}

__global__ void eval_gt_kernel(const int *__restrict__ gt_class, const unsigned char *__restrict__ gt_difficult,
                               const int *__restrict__ gt_off, int G, int n_images, int K, u64 *__restrict__ has_mask,
                               int *__restrict__ npos, int *__restrict__ ni) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_images) return;
    const int g0 = max(gt_off[i], 0), g1 = min(gt_off[i + 1], G);
    u64 mask = 0;
    for (int g = g0; g < g1; ++g) {
        const int c = gt_class[g];
        if (c < 1 || c >= K) continue;
        mask |= 1ull << (c - 1);
        if (!gt_difficult[g]) atomicAdd(&npos[c - 1], 1);
    }
    has_mask[i] = mask;
    for (int c = 1; c < K; ++c)
        if ((mask >> (c - 1)) & 1) atomicAdd(&ni[c - 1], 1);
}

__global__ __launch_bounds__(256) void eval_keys_kernel(DetInput in, int D, int Dpad, int quantise, const double *__restrict__ gt_boxes,
                                                        const int *__restrict__ gt_class, const int *__restrict__ gt_off, int G,
                                                        int n_images, int K, double ovthresh, const double *__restrict__ thresholds, int base_t,
                                                        u64 *__restrict__ keys, double *__restrict__ conf_out, int *__restrict__ gbox,
                                                        int *__restrict__ class_count, u64 *__restrict__ max_hit,
                                                        int *__restrict__ num_fp_per_img) {
    __shared__ int s_count[64];
    if (threadIdx.x < 64) s_count[threadIdx.x] = 0;
    __syncthreads();
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < Dpad) {
        int img = -1, cls = 0;
        float s = 0.0f, b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (d < D) {
            if (in.batched) {
                const int p = d % in.P, ij = d / in.P, j = ij % (K - 1), i = ij / (K - 1);
                if (p < min(in.counts[ij], in.P)) {       // (a flagged image has counts[i, 0] = -1: no detections)
                    const float *row = in.dets + (size_t)d * 5;
                    b[0] = row[0];  b[1] = row[1];  b[2] = row[2];  b[3] = row[3];  s = row[4];
                    img = in.first_image + i;
                    cls = j + 1;
                }
            } else {
                img = in.image[d];
                cls = in.cls[d];
                s = in.scores[d];
                for (int q = 0; q < 4; ++q) b[q] = in.boxes[(size_t)d * 4 + q];
            }
        }
        const bool valid = img >= 0 && img < n_images && cls >= 1 && cls < K;
        u64 key = IDX_MASK - (u64)d;                      // an ignored slot: class field 0, still unique and non-zero
        if (valid) {
            double conf, bb[4];
            unsigned int score_part;
            if (quantise) {
                const double q = rint((double)s * 1000.0);
                conf = q / 1000.0;
                const double qc = fmin(fmax(q, -2147483648.0), 2147483647.0);
                score_part = (unsigned int)(int)qc ^ 0x80000000u;
                for (int k = 0; k < 4; ++k) bb[k] = rint((double)(b[k] + 1.0f) * 10.0) / 10.0;
            } else {
                conf = (double)s;
                const unsigned int u = __float_as_uint(s == 0.0f ? 0.0f : s);       // (-0 and +0 are one score)
                score_part = (u >> 31) ? ~u : (u | 0x80000000u);
                for (int k = 0; k < 4; ++k) bb[k] = (double)b[k];
            }
            // voc_eval_bus.py:221-236
            double ovmax = -INFINITY;
            int jmax = -1;
            const int g0 = max(gt_off[img], 0), g1 = min(gt_off[img + 1], G);
            for (int g = g0; g < g1; ++g) {
                if (gt_class[g] != cls) continue;
                const double *gb = gt_boxes + (size_t)g * 4;
                const double ixmin = fmax(gb[0], bb[0]), iymin = fmax(gb[1], bb[1]);
                const double ixmax = fmin(gb[2], bb[2]), iymax = fmin(gb[3], bb[3]);
                const double iw = fmax(ixmax - ixmin + 1., 0.), ih = fmax(iymax - iymin + 1., 0.);
                const double inters = iw * ih;
                const double uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (gb[2] - gb[0] + 1.) * (gb[3] - gb[1] + 1.) - inters);
                const double ov = inters / uni;
                if (ov > ovmax) { ovmax = ov;  jmax = g; }
            }
            const bool hit = ovmax > ovthresh;
            conf_out[d] = conf;
            gbox[d] = hit ? jmax : -1;
            if (hit) atomicMax(&max_hit[(size_t)(cls - 1) * n_images + img], ordered_bits(conf));
            else if (conf >= thresholds[base_t]) atomicAdd(&num_fp_per_img[(size_t)(cls - 1) * n_images + img], 1);
            atomicAdd(&s_count[cls - 1], 1);
            key = ((u64)(K - cls) << CLASS_SHIFT) | ((u64)score_part << SCORE_SHIFT) | (IDX_MASK - (u64)d);
        } else if (d < D) {
            conf_out[d] = 0.0;
            gbox[d] = -1;
        }
        keys[d] = key;
    }
    __syncthreads();
    if (threadIdx.x < K - 1 && s_count[threadIdx.x]) atomicAdd(&class_count[threadIdx.x], s_count[threadIdx.x]);
}

__global__ __launch_bounds__(SORT_THREADS) void eval_runs_kernel(const u64 *__restrict__ keys, u64 *__restrict__ sorted_runs) {
    __shared__ typename RunSort::storage_type storage;
    const size_t base = (size_t)blockIdx.x * RUN + threadIdx.x * SORT_ITEMS;
    u64 k[SORT_ITEMS];
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) k[i] = keys[base + i];
    sort_and_store_run(k, storage, sorted_runs + (size_t)blockIdx.x * RUN);
}

// blocks of w sorted (descending, unique) keys -> blocks of 2w; n is a multiple of RUN and w a multiple of RUN
__global__ __launch_bounds__(256) void eval_merge_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, int n, int w) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int blk = p / w, start_a = (blk & ~1) * w, start_b = start_a + w;
    const bool in_b = blk & 1;
    const int other = in_b ? start_a : start_b;
    const int len = in_b ? w : max(0, min(w, n - start_b));
    const u64 key = in[p];
    int lo = 0, hi = len;                                 // the sibling's keys greater than `key`: a prefix of it
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (in[other + mid] > key) lo = mid + 1;
        else hi = mid;
    }
    out[start_a + (p - (in_b ? start_b : start_a)) + lo] = key;
}

__global__ __launch_bounds__(256) void eval_first_kernel(const u64 *__restrict__ sorted, int n, const int *__restrict__ gbox,
                                                         int *__restrict__ first) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u64 key = sorted[r];
    if ((key >> CLASS_SHIFT) == 0) return;
    const int g = gbox[(int)(IDX_MASK - (key & IDX_MASK))];
    if (g >= 0) atomicMin(&first[g], r);
}

struct Flags { int tp, fp, nh; };
__device__ __forceinline__ Flags operator+(const Flags &a, const Flags &b) { return Flags{a.tp + b.tp, a.fp + b.fp, a.nh + b.nh}; }

// voc_eval_bus.py:238-251 for the detection at sorted rank r
__device__ __forceinline__ Flags flags_at(const u64 *__restrict__ sorted, int r, const int *__restrict__ gbox, const int *__restrict__ first,
                                          const unsigned char *__restrict__ gt_difficult) {
    Flags f{0, 0, 0};
    const u64 key = sorted[r];
    if ((key >> CLASS_SHIFT) == 0) return f;
    const int g = gbox[(int)(IDX_MASK - (key & IDX_MASK))];
    if (g < 0) { f.fp = 1;  f.nh = 1; }
    else if (!gt_difficult[g]) { if (first[g] == r) f.tp = 1; else f.fp = 1; }
    return f;
}

__device__ __forceinline__ Flags wave_inclusive(Flags v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int a = __shfl_up(v.tp, off, 64), b = __shfl_up(v.fp, off, 64), c = __shfl_up(v.nh, off, 64);
        if (lane >= off) { v.tp += a;  v.fp += b;  v.nh += c; }
    }
    return v;
}

// inclusive scan over the workgroup (THREADS a multiple of 64, at most 1024); *total = the workgroup's sum
template <int THREADS>
__device__ __forceinline__ Flags block_inclusive(Flags v, Flags *s_wave /* [THREADS / 64] */, Flags *total) {
    constexpr int WAVES = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Flags inc = wave_inclusive(v);
    __syncthreads();
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    Flags before{0, 0, 0}, all{0, 0, 0};
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before = before + s_wave[w];
        all = all + s_wave[w];
    }
    *total = all;
    return inc + before;
}

__global__ __launch_bounds__(SCAN_THREADS) void eval_scan_reduce_kernel(const u64 *__restrict__ sorted, const int *__restrict__ gbox,
                                                                        const int *__restrict__ first, const unsigned char *__restrict__ gt_difficult,
                                                                        Flags *__restrict__ block_sums) {
    __shared__ Flags s_wave[SCAN_THREADS / 64];
    const int base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    Flags v{0, 0, 0};
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) v = v + flags_at(sorted, base + i, gbox, first, gt_difficult);
    Flags total;
    block_inclusive<SCAN_THREADS>(v, s_wave, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block_sums -> exclusive prefix (in place); class_count -> class_offsets [K]
__global__ __launch_bounds__(1024) void eval_scan_spine_kernel(Flags *__restrict__ block_sums, int nb, const int *__restrict__ class_count, int K,
                                                               int *__restrict__ class_offsets) {
    __shared__ Flags s_wave[1024 / 64];
    Flags carry{0, 0, 0};
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        const Flags v = b < nb ? block_sums[b] : Flags{0, 0, 0};
        Flags total;
        const Flags inc = block_inclusive<1024>(v, s_wave, &total);
        if (b < nb) block_sums[b] = Flags{carry.tp + inc.tp - v.tp, carry.fp + inc.fp - v.fp, carry.nh + inc.nh - v.nh};
        carry = carry + total;
    }
    if (threadIdx.x == 0) {
        int acc = 0;
        class_offsets[0] = 0;
        for (int c = 1; c < K; ++c) { acc += class_count[c - 1];  class_offsets[c] = acc; }
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void eval_scan_kernel(const u64 *__restrict__ sorted, const int *__restrict__ gbox,
                                                                 const int *__restrict__ first, const unsigned char *__restrict__ gt_difficult,
                                                                 const Flags *__restrict__ block_offsets, Flags *__restrict__ cum) {
    __shared__ Flags s_wave[SCAN_THREADS / 64];
    const int base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    Flags f[SCAN_ITEMS], v{0, 0, 0};
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { f[i] = flags_at(sorted, base + i, gbox, first, gt_difficult);  v = v + f[i]; }
    Flags total;
    const Flags inc = block_inclusive<SCAN_THREADS>(v, s_wave, &total);
    const Flags off = block_offsets[blockIdx.x];
    Flags run{off.tp + inc.tp - v.tp, off.fp + inc.fp - v.fp, off.nh + inc.nh - v.nh};
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { run = run + f[i];  cum[base + i] = run; }
}

__global__ __launch_bounds__(256) void eval_curves_kernel(const u64 *__restrict__ sorted, int D, const Flags *__restrict__ cum,
                                                          const int *__restrict__ class_offsets, const int *__restrict__ npos, int K,
                                                          int *__restrict__ order, int *__restrict__ tp, int *__restrict__ fp,
                                                          double *__restrict__ rec, double *__restrict__ prec) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= D) return;
    const u64 key = sorted[r];
    const int field = (int)(key >> CLASS_SHIFT);
    if (field == 0) {                                    // past the last class's segment
        order[r] = -1;  tp[r] = 0;  fp[r] = 0;  rec[r] = 0.0;  prec[r] = 0.0;
        return;
    }
    const int c = K - field, b = class_offsets[c - 1];
    Flags v = cum[r];
    if (b > 0) { const Flags o = cum[b - 1];  v.tp -= o.tp;  v.fp -= o.fp; }
    order[r] = (int)(IDX_MASK - (key & IDX_MASK));
    tp[r] = v.tp;
    fp[r] = v.fp;
    rec[r] = (double)v.tp / (double)npos[c - 1];                           // voc_eval_bus.py:271
    prec[r] = (double)v.tp / fmax((double)v.tp + (double)v.fp, DBL_EPSILON);     // :274
}

// voc_ap of one class, both metrics, in one backward sweep of its segment (one workgroup per class)
__global__ __launch_bounds__(AP_THREADS) void eval_ap_kernel(const double *__restrict__ rec, const double *__restrict__ prec,
                                                             const int *__restrict__ class_offsets, double *__restrict__ ap07,
                                                             double *__restrict__ ap_area) {
    __shared__ double s_wave[AP_THREADS / 64], s_sum[AP_THREADS / 64], s_p[11];
    __shared__ int s_idx[11];
    const int c = blockIdx.x, base = class_offsets[c], n = class_offsets[c + 1] - base, t = threadIdx.x;
    if (n <= 0) {                                        // the reference's sentinel for an empty result file
        if (t == 0) { ap07[c] = -1.0;  ap_area[c] = -1.0; }
        return;
    }
    const double *R = rec + base, *Pq = prec + base;
    if (t < 11) {                                        // first index with rec >= t * 0.1 (rec ascends, or is all NaN)
        const double thr = t * 0.1;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (R[mid] >= thr) hi = mid;
            else lo = mid + 1;
        }
        s_idx[t] = lo;
        s_p[t] = 0.0;
    }
    __syncthreads();
    int idx[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) idx[i] = s_idx[i];
    const int lane = t & 63, wave = t >> 6;
    double carry = -INFINITY, sum = 0.0;
    for (int ch = (n - 1) / AP_THREADS; ch >= 0; --ch) {
        const int j = ch * AP_THREADS + t;
        double m = j < n ? Pq[j] : -INFINITY;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {         // suffix maximum inside the wave
            const double o = __shfl_down(m, off, 64);
            if (lane + off < 64) m = fmax(m, o);
        }
        __syncthreads();                                 // (s_wave of the previous chunk has been read)
        if (lane == 0) s_wave[wave] = m;
        __syncthreads();
        double chunk_max = -INFINITY;
        for (int w = AP_THREADS / 64 - 1; w >= 0; --w) {
            if (w > wave) m = fmax(m, s_wave[w]);
            chunk_max = fmax(chunk_max, s_wave[w]);
        }
        m = fmax(m, carry);                              // max of prec[j ..]
        carry = fmax(carry, chunk_max);
        if (j < n) {
#pragma unroll
            for (int i = 0; i < 11; ++i)
                if (idx[i] == j) s_p[i] = m;
            const double prev = j > 0 ? R[j - 1] : 0.0, cur = R[j];
            if (cur != prev) sum += (cur - prev) * fmax(m, 0.0);
        }
    }
    if (t == 0 && R[n - 1] != 1.0) sum += (1.0 - R[n - 1]) * 0.0;       // the sentinel step of mrec (adds 0, or NaN with rec)
#pragma unroll
    for (int off = 32; off; off >>= 1) sum += __shfl_down(sum, off, 64);
    __syncthreads();
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (t == 0) {
        double area = 0.0;
        for (int w = 0; w < AP_THREADS / 64; ++w) area += s_sum[w];
        ap_area[c] = area;
        double ap = 0.0;
        for (int i = 0; i < 11; ++i) {
            const double p = idx[i] < n ? s_p[i] : 0.0;
            ap = ap + p / 11.;
        }
        ap07[c] = ap;
    }
}

// one workgroup per (class, threshold)
__global__ __launch_bounds__(256) void eval_thresholds_kernel(const double *__restrict__ thresholds, int T, int base_t, int n_images, int K,
                                                              const u64 *__restrict__ has_mask, const u64 *__restrict__ max_hit,
                                                              const u64 *__restrict__ sorted, const double *__restrict__ conf,
                                                              const Flags *__restrict__ cum, const int *__restrict__ class_offsets,
                                                              int *__restrict__ nok, int *__restrict__ num_all_fps,
                                                              unsigned char *__restrict__ arr_ok) {
    __shared__ int s_part[256 / 64];
    const int c = blockIdx.x / T, ti = blockIdx.x - c * T;
    const double thr = thresholds[ti];
    int count = 0;
    for (int i = threadIdx.x; i < n_images; i += blockDim.x) {
        const u64 mh = max_hit[(size_t)c * n_images + i];
        const bool ok = ((has_mask[i] >> c) & 1) && mh != 0 && from_ordered_bits(mh) >= thr;
        count += ok;
        if (ti == base_t) arr_ok[(size_t)c * n_images + i] = ok;
    }
    for (int off = 32; off; off >>= 1) count += __shfl_down(count, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        nok[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        // detections of the class with conf >= thr: a prefix of its segment (descending confidence)
        const int b = class_offsets[c], n = class_offsets[c + 1] - b;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (conf[(int)(IDX_MASK - (sorted[b + mid] & IDX_MASK))] >= thr) lo = mid + 1;
            else hi = mid;
        }
        int fps = 0;
        if (lo > 0) fps = cum[b + lo - 1].nh - (b > 0 ? cum[b - 1].nh : 0);
        num_all_fps[blockIdx.x] = fps;
    }
}

struct Workspace {
    u64 *keys_a, *keys_b, *max_hit, *has_mask;
    double *conf;
    int *gbox, *first, *class_count;
    Flags *cum, *block_sums;
    size_t bytes;
};

Workspace carve(void *p, long long D, int G, int n_images, int K) {
    const size_t Dpad = (size_t)cdiv(D, RUN) * RUN;
    Carver c(p);
    Workspace w;
    w.keys_a = c.take<u64>(Dpad);
    w.keys_b = c.take<u64>(Dpad);
    w.max_hit = c.take<u64>((size_t)(K - 1) * n_images);
    w.has_mask = c.take<u64>(n_images);
    w.conf = c.take<double>(D);
    w.gbox = c.take<int>(D);
    w.first = c.take<int>(G);
    w.class_count = c.take<int>(64);
    w.cum = c.take<Flags>(Dpad);
    w.block_sums = c.take<Flags>(Dpad / SCAN_BLOCK);
    w.bytes = c.off + 256;
    return w;
}

bool sizes_ok(long long D, int G, int n_images, int K, int T) {
    return D >= 0 && D <= MAX_SLOTS && G >= 0 && n_images >= 0 && K >= 2 && K <= 65 && T >= 1 &&
           (long long)(K - 1) * T <= 0x7fffffffll && (long long)(K - 1) * n_images <= 0x7fffffffll;
}

#define EVAL_CHECK(call)                                   \
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

size_t wssdl_eval_detections_workspace_bytes(int64_t D, int G, int n_images, int n_classes) {
    if (!sizes_ok(D, G, n_images, n_classes, 1)) return 0;      // (pure host: sizes only)
    return carve(nullptr, D, G, n_images, n_classes).bytes;
}

int wssdl_eval_detections(int flags, const float *det_boxes, const float *det_scores, const int32_t *det_image,
                          const int32_t *det_class, int D, const float *dets, const int32_t *counts, int N, int P,
                          int first_image, const double *gt_boxes, const int32_t *gt_class, const uint8_t *gt_difficult,
                          const int32_t *gt_image_offsets, int G, int n_images, int n_classes, double ovthresh,
                          const double *thresholds, int T, int base_threshold, int32_t *order, int32_t *class_offsets,
                          int32_t *tp, int32_t *fp, double *rec, double *prec, double *ap07, double *ap_area, int32_t *npos,
                          int32_t *ni, int32_t *nok, int32_t *num_all_fps, uint8_t *arr_ok, int32_t *num_fp_per_img,
                          void *workspace, size_t workspace_bytes, wssdl_stream_t stream) {
    const int K = n_classes;
    const bool batched = flags & WSSDL_EVAL_BATCHED;
    if (flags & ~(WSSDL_EVAL_QUANTISE | WSSDL_EVAL_BATCHED)) return WSSDL_ERR_INVALID_ARGUMENT;
    if (K < 2 || K > 65) return WSSDL_ERR_INVALID_ARGUMENT;
    long long slots = D;
    if (batched) {
        if (N < 0 || P < 0) return WSSDL_ERR_INVALID_ARGUMENT;
        slots = (long long)N * (K - 1) * P;
    }
    if (!sizes_ok(slots, G, n_images, K, T) || base_threshold < 0 || base_threshold >= T) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!thresholds || !class_offsets || !ap07 || !ap_area || !npos || !ni || !nok || !num_all_fps) return WSSDL_ERR_INVALID_ARGUMENT;
    if (n_images > 0 && (!gt_image_offsets || !arr_ok || !num_fp_per_img)) return WSSDL_ERR_INVALID_ARGUMENT;
    if (G > 0 && (!gt_boxes || !gt_class || !gt_difficult)) return WSSDL_ERR_INVALID_ARGUMENT;
    if (slots > 0) {
        if (batched ? (!dets || !counts) : (!det_boxes || !det_scores || !det_image || !det_class)) return WSSDL_ERR_INVALID_ARGUMENT;
        if (!order || !tp || !fp || !rec || !prec) return WSSDL_ERR_INVALID_ARGUMENT;
    }
    const Workspace w = carve(workspace, slots, G, n_images, K);
    if (!workspace || workspace_bytes < w.bytes) return WSSDL_ERR_INVALID_ARGUMENT;
    const int Dn = (int)slots, Dpad = cdiv(slots, RUN) * RUN;
    hipStream_t st = as_stream(stream);

    EVAL_CHECK(hipMemsetAsync(npos, 0, sizeof(int) * (K - 1), st));
    EVAL_CHECK(hipMemsetAsync(ni, 0, sizeof(int) * (K - 1), st));
    EVAL_CHECK(hipMemsetAsync(w.class_count, 0, sizeof(int) * 64, st));
    if (n_images > 0) {
        EVAL_CHECK(hipMemsetAsync(w.max_hit, 0, sizeof(u64) * (size_t)(K - 1) * n_images, st));
        EVAL_CHECK(hipMemsetAsync(num_fp_per_img, 0, sizeof(int) * (size_t)(K - 1) * n_images, st));
        hipLaunchKernelGGL(eval_gt_kernel, dim3(cdiv(n_images, 256)), dim3(256), 0, st, gt_class, gt_difficult, gt_image_offsets, G, n_images,
                           K, w.has_mask, npos, ni);
    }
    if (G > 0) EVAL_CHECK(hipMemsetAsync(w.first, 0x7f, sizeof(int) * (size_t)G, st));
    const u64 *sorted = w.keys_b;
    if (Dpad > 0) {
        DetInput in{batched ? 1 : 0, det_boxes, det_scores, det_image, det_class, dets, counts, N, P, first_image};
        hipLaunchKernelGGL(eval_keys_kernel, dim3(Dpad / 256), dim3(256), 0, st, in, Dn, Dpad, (flags & WSSDL_EVAL_QUANTISE) ? 1 : 0, gt_boxes,
                           gt_class, gt_image_offsets, G, n_images, K, ovthresh, thresholds, base_threshold, w.keys_a, w.conf, w.gbox,
                           w.class_count, w.max_hit, num_fp_per_img);
        hipLaunchKernelGGL(eval_runs_kernel, dim3(Dpad / RUN), dim3(SORT_THREADS), 0, st, w.keys_a, w.keys_b);
        u64 *src = w.keys_b, *dst = w.keys_a;
        for (long long width = RUN; width < Dpad; width *= 2) {
            hipLaunchKernelGGL(eval_merge_kernel, dim3(Dpad / 256), dim3(256), 0, st, src, dst, Dpad, (int)width);
            u64 *tmp = src;  src = dst;  dst = tmp;
        }
        sorted = src;
        hipLaunchKernelGGL(eval_first_kernel, dim3(Dpad / 256), dim3(256), 0, st, sorted, Dpad, w.gbox, w.first);
        hipLaunchKernelGGL(eval_scan_reduce_kernel, dim3(Dpad / SCAN_BLOCK), dim3(SCAN_THREADS), 0, st, sorted, w.gbox, w.first, gt_difficult,
                           w.block_sums);
    }
    hipLaunchKernelGGL(eval_scan_spine_kernel, dim3(1), dim3(1024), 0, st, w.block_sums, Dpad / SCAN_BLOCK, w.class_count, K, class_offsets);
    if (Dpad > 0) {
        hipLaunchKernelGGL(eval_scan_kernel, dim3(Dpad / SCAN_BLOCK), dim3(SCAN_THREADS), 0, st, sorted, w.gbox, w.first, gt_difficult,
                           w.block_sums, w.cum);
        hipLaunchKernelGGL(eval_curves_kernel, dim3(cdiv(Dn, 256)), dim3(256), 0, st, sorted, Dn, w.cum, class_offsets, npos, K, order, tp, fp,
                           rec, prec);
    }
    hipLaunchKernelGGL(eval_ap_kernel, dim3(K - 1), dim3(AP_THREADS), 0, st, rec, prec, class_offsets, ap07, ap_area);
    hipLaunchKernelGGL(eval_thresholds_kernel, dim3((K - 1) * T), dim3(256), 0, st, thresholds, T, base_threshold, n_images, K, w.has_mask,
                       w.max_hit, sorted, w.conf, w.cum, class_offsets, nok, num_all_fps, arr_ok);
    return check_launch();
}

}  // extern "C"
