// Soft-NMS at test time (Bodla et al., 2017; not in the reference): wssdl_post_detections_soft, the views op
// (post_detect.hip) with a score decay in place of the deletion.  The contract is the header comment; the NumPy
// statement is tests/soft_nms_reference.py.
//
// The suppression is sequential -- every pick depends on the scores the pick before left -- so it does not fit the
// rank-once, mask-and-sweep kernels of nms.hip.  Three launches:
//   1. post_view_segments_kernel (post_detect.hip): the run of every output image in the blob;
//   2. soft_nms_kernel: ONE workgroup per (image, class) segment.  The candidates (rows above both floors, un-mirrored)
//      are compacted into LDS in ascending row order -- 24 bytes each: box 16, working score 4, area 4 -- so a
//      candidate's compact index orders like its local row and serves as the tie-break.  Then at most n turns of
//        scan    every thread takes the largest key (score bits << 32 | index; 0 = not live) of its strided share,
//        reduce  across the wave with cross-lane shuffles, across the waves with one LDS maximum,
//        emit    one thread appends (box, score) to the segment's list in the workspace,
//        decay   every thread lowers the live scores of its share and retires those at or below the floor.
//      The loop is a `for` bounded by the candidate count; its only exit reads ONE LDS word after a barrier, so the
//      whole workgroup leaves in the same turn.  Four waves per segment: a single-wave form of the same loop (no LDS
//      maximum, no barrier to wait at) took 2.2 times as long at 16 segments of pitch 600 (EXPERIMENTS.md, "Soft-NMS").
//   3. soft_cap_kernel: one workgroup per image, the max_per_image-th largest emitted score (select.hip.h, as
//      post_cap_kernel) and the copy of every class's prefix into dets.  post_cap_kernel itself does not fit: it
//      reads the scores of the kept rows from the input blob, and these are decayed.
#include "nms.hip.h"
#include "post_views.hip.h"
#include "select.hip.h"

#include <float.h>
#include <math.h>

namespace wssdl {

constexpr int SOFT_BLOCK = 256;
constexpr int SOFT_WAVES = SOFT_BLOCK / 64;
constexpr int SOFT_ROW_BYTES = 24;
static_assert((size_t)WSSDL_POST_SOFT_MAX_ROWS * SOFT_ROW_BYTES <= 160u * 1024u - 1024u,
              "a segment at the limit must fit the LDS of one workgroup next to the static part");

struct SoftWs {
    int *img_lo, *img_hi, *n_emit;
    float *emit;                // [nseg, P, 5]: every segment's picks in the order they were made
};

static size_t carve_soft(void *ws, int n_images, int P, int nc, SoftWs *out) {
    Carver c(ws);
    SoftWs w;
    const size_t nseg = (size_t)n_images * nc;
    w.img_lo = c.take<int>((size_t)n_images + 64);
    w.img_hi = c.take<int>((size_t)n_images + 64);
    w.n_emit = c.take<int>(nseg + 64);
    w.emit = c.take<float>(nseg * P * 5);
    if (out) *out = w;
    return c.off;
}

// the weight of one pick on one live candidate (header, "Weight"); ov is the cpu_nms overlap in f32
__device__ __forceinline__ float soft_weight(float ov, int method, double nms_thresh, double sigma) {
    if (method == 2) {
        if (ov == 0.0f) return 1.0f;
        const double o = (double)ov;
        const double q = -(o * o) / sigma;
        return (float)exp(q);
    }
    if (!((double)ov >= nms_thresh)) return 1.0f;
    return method == 1 ? 1.0f - ov : 0.0f;
}

__global__ __launch_bounds__(SOFT_BLOCK) void soft_nms_kernel(const float *__restrict__ rois, const int *__restrict__ lo,
                                                              const int *__restrict__ hi, const float *__restrict__ scores,
                                                              const float *__restrict__ boxes,
                                                              const float *__restrict__ flip_width, int R, int K,
                                                              int n_images, int views, int P, float score_thresh,
                                                              float min_score, int method, double nms_thresh, double sigma,
                                                              float *__restrict__ emit, int *__restrict__ n_emit) {
    extern __shared__ __align__(16) unsigned char soft_dyn[];
    __shared__ unsigned long long s_pick[2];
    __shared__ int s_wcount[SOFT_WAVES];
    const int nc = K - 1, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int seg = blockIdx.x, img = seg / nc, c = seg - img * nc;
    int start, count;
    image_rows(lo, hi, img, R, start, count);
    if (count > P) {            // the same for the whole workgroup; the cap kernel reports the image
        if (t == 0) n_emit[seg] = 0;
        return;
    }
    // count <= P rows: the three arrays are laid out for `count` candidates
    nms_float4v *s_box = reinterpret_cast<nms_float4v *>(soft_dyn);
    float *s_score = reinterpret_cast<float *>(s_box + count);
    float *s_area = s_score + count;
    if (t < 2) s_pick[t] = 0ull;

    // ---- candidates, compacted in ascending row order
    int n = 0;
    for (int base = 0; base < count; base += SOFT_BLOCK) {       // count is the same for the whole workgroup
        const int p = base + t;
        bool cand = false;
        float s = 0.0f, x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f;
        int src = -1;
        if (p < count && roi_view_image(rois, start + p, n_images, views, src) == img) {
            const size_t r = (size_t)(start + p);
            s = scores[r * K + c + 1];
            cand = s > score_thresh && s > min_score;            // NaN fails both
            if (cand) {
                const float *b = boxes + r * 4 * K + 4 * (c + 1);
                x1 = b[0];  y1 = b[1];  x2 = b[2];  y2 = b[3];
                unmirror_x(flip_width ? flip_width[src] : -1.0f, x1, x2);
            }
        }
        const unsigned long long m = __ballot(cand);
        if (lane == 0) s_wcount[wave] = __popcll(m);
        __syncthreads();
        int off = n, total = 0;
#pragma unroll
        for (int w = 0; w < SOFT_WAVES; ++w) {
            const int k = s_wcount[w];
            off += w < wave ? k : 0;
            total += k;
        }
        if (cand) {
            const int i = off + __popcll(m & ((1ull << lane) - 1ull));
            nms_float4v v;
            v.x = x1;  v.y = y1;  v.z = x2;  v.w = y2;
            s_box[i] = v;
            s_score[i] = s;
            s_area[i] = box_area_ref(x1, y1, x2, y2);
        }
        n += total;
        __syncthreads();
    }

    // ---- pick loop: at most n picks
    float *out = emit + (size_t)seg * P * 5;
    int emitted = 0;
    for (int it = 0; it < n; ++it) {
        unsigned long long best = 0ull;
        for (int i = t; i < n; i += SOFT_BLOCK) {
            const float s = s_score[i];
            const unsigned long long k = ((unsigned long long)__builtin_bit_cast(unsigned, s) << 32) | (unsigned)i;
            best = (s > 0.0f && k > best) ? k : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other > best ? other : best;
        }
        if (lane == 0 && best != 0ull) atomicMax(&s_pick[it & 1], best);
        __syncthreads();
        const unsigned long long pick = s_pick[it & 1];          // the one value every thread leaves on
        if (pick == 0ull) break;
        if (t == 0) s_pick[(it + 1) & 1] = 0ull;                 // read last before this turn's first barrier
        const int pi = (int)(unsigned)(pick & 0xffffffffull);
        const float ps = __builtin_bit_cast(float, (unsigned)(pick >> 32));
        const nms_float4v pb = s_box[pi];
        const float parea = s_area[pi];
        if (t == 0) {
            float *o = out + (size_t)it * 5;
            o[0] = pb.x;  o[1] = pb.y;  o[2] = pb.z;  o[3] = pb.w;  o[4] = ps;
        }
        emitted = it + 1;
        for (int j = t; j < n; j += SOFT_BLOCK) {
            const float s = s_score[j];
            if (j == pi) {
                s_score[j] = 0.0f;
            } else if (s > 0.0f) {
                const nms_float4v b = s_box[j];
                const float xx1 = fmax_ref(pb.x, b.x);
                const float yy1 = fmax_ref(pb.y, b.y);
                const float xx2 = fmin_ref(pb.z, b.z);
                const float yy2 = fmin_ref(pb.w, b.w);
                float w = xx2 - xx1;  w = fmax0_ref(w + 1.0f);
                float h = yy2 - yy1;  h = fmax0_ref(h + 1.0f);
                const float inter = w * h;
                float den = parea + s_area[j];
                den = den - inter;
                const float ov = inter / den;
                const float d = s * soft_weight(ov, method, nms_thresh, sigma);
                s_score[j] = d > min_score ? d : 0.0f;
            }
        }
        __syncthreads();
    }
    if (t == 0) n_emit[seg] = emitted;
}

// One workgroup per image: the max_per_image-th largest emitted score over the image's classes, then every class's
// prefix at or above it -- the emitted scores never increase, so the rows that pass are a prefix.  Only those rows are
// written.  An image with more rows than P reports counts[i, 0] = -1.
constexpr int SOFT_CAP_BLOCK = 1024;
constexpr int SOFT_CAP_LIST = 512;

__global__ __launch_bounds__(SOFT_CAP_BLOCK) void soft_cap_kernel(const int *__restrict__ lo, const int *__restrict__ hi,
                                                                  const float *__restrict__ emit,
                                                                  const int *__restrict__ n_emit, int R, int K, int P,
                                                                  int max_per_image, float *__restrict__ dets,
                                                                  int *__restrict__ counts) {
    __shared__ SelectScratch<SOFT_CAP_LIST> sc;
    __shared__ int s_count[64];
    const int nc = K - 1, t = threadIdx.x, img = blockIdx.x;
    int start, count;
    image_rows(lo, hi, img, R, start, count);
    const size_t seg0 = (size_t)img * nc;
    if (count > P) {            // the same for the whole workgroup: no barrier is skipped by part of it
        if (t < nc) counts[seg0 + t] = t == 0 ? -1 : 0;
        return;
    }
    const int *ne = n_emit + seg0;
    const float *e = emit + seg0 * P * 5;
    float *d = dets + seg0 * P * 5;
    if (t < 64) s_count[t] = 0;
    // item i = (class c, position p); its key: score bits over a unique low word
    auto key_at = [&](int i, unsigned long long &v) -> bool {
        const int c = i / P, p = i - c * P;
        if (p >= ne[c]) return false;
        v = score_key(e[(size_t)i * 5 + 4], (unsigned)i);
        return true;
    };
    const unsigned long long kth = block_radix_select<SOFT_CAP_BLOCK, SOFT_CAP_LIST, true>(
        key_at, nc * P, [max_per_image](int m) { return (max_per_image > 0 && m > max_per_image) ? max_per_image : 0; }, sc);
    // image_thresh as order-preserving score bits (0: no cap -- every emitted row passes)
    const unsigned cut = (unsigned)(kth >> 32);
    __syncthreads();
    for (int i = t; i < nc * P; i += SOFT_CAP_BLOCK) {
        const int c = i / P, p = i - c * P;
        if (p >= ne[c]) continue;
        const float *b = e + (size_t)i * 5;
        if ((unsigned)(score_key(b[4], 0u) >> 32) < cut) continue;
        float *o = d + (size_t)i * 5;
        o[0] = b[0];  o[1] = b[1];  o[2] = b[2];  o[3] = b[3];  o[4] = b[4];
        atomicAdd(&s_count[c], 1);
    }
    __syncthreads();
    if (t < nc && t < 64) counts[seg0 + t] = s_count[t];
}

}  // namespace wssdl

using namespace wssdl;

static bool soft_shape_ok(int n_images, int views, int P, int num_classes) {
    const long long nc = num_classes - 1;
    return n_images >= 1 && views >= 1 && views <= POST_MAX_VIEWS && P >= 1 && P <= WSSDL_POST_SOFT_MAX_ROWS &&
           num_classes >= 2 && nc <= 64 && n_images * nc * P <= POST_MAX_ITEMS && n_images * nc <= POST_MAX_SEGMENTS;
}

extern "C" size_t wssdl_post_detections_soft_workspace_bytes(int n_images, int views, int max_rows_per_image,
                                                             int num_classes) {
    if (!soft_shape_ok(n_images, views, max_rows_per_image, num_classes)) return 0;
    return carve_soft(nullptr, n_images, max_rows_per_image, num_classes - 1, nullptr);
}

extern "C" int wssdl_post_detections_soft(const float *rois, const float *scores, const float *boxes, int R, int n_images,
                                          int views, const float *flip_width, int max_rows_per_image, int num_classes,
                                          float score_thresh, int method, double nms_thresh, double sigma, float min_score,
                                          int max_per_image, float *dets, int32_t *counts, void *workspace,
                                          size_t workspace_bytes, wssdl_stream_t stream) {
    const int nc = num_classes - 1;
    const int P = max_rows_per_image;
    if (views < 1 || views > POST_MAX_VIEWS) return WSSDL_ERR_INVALID_ARGUMENT;
    if (method < 0 || method > 2) return WSSDL_ERR_INVALID_ARGUMENT;
    if (method == 2 && !(sigma > 0.0 && sigma <= DBL_MAX)) return WSSDL_ERR_INVALID_ARGUMENT;
    if (method != 2 && !(nms_thresh > 0.0 && nms_thresh <= 1.0)) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!(min_score >= FLT_MIN && min_score < 1.0f)) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!(score_thresh >= 0.0f)) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R < 0 || n_images < 0 || num_classes < 2 || nc > 64) return WSSDL_ERR_INVALID_ARGUMENT;
    if (P > WSSDL_POST_SOFT_MAX_ROWS) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R > 0 && (P < 1 || (long long)n_images * nc * P > POST_MAX_ITEMS || (long long)n_images * nc > POST_MAX_SEGMENTS))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (n_images == 0) return WSSDL_OK;
    if (!counts) return WSSDL_ERR_INVALID_ARGUMENT;
    hipStream_t st = as_stream(stream);
    if (R == 0) {
        if (hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_images * nc, st) != hipSuccess) return WSSDL_ERR_LAUNCH;
        return WSSDL_OK;
    }
    if (!rois || !scores || !boxes || !dets || !workspace) return WSSDL_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < wssdl_post_detections_soft_workspace_bytes(n_images, views, P, num_classes))
        return WSSDL_ERR_WORKSPACE;
    SoftWs w;
    carve_soft(workspace, n_images, P, nc, &w);
    // the candidates of a segment are rows of its image's run, never more than min(P, R)
    const size_t lds = (size_t)(P < R ? P : R) * SOFT_ROW_BYTES;
    if (lds > 48u * 1024u) {    // beyond the default dynamic LDS of a launch: raise the kernel's limit (a host-side attribute)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(soft_nms_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           WSSDL_POST_SOFT_MAX_ROWS * SOFT_ROW_BYTES);
        if (e != hipSuccess) {
            set_last_error(e);
            return WSSDL_ERR_LAUNCH;
        }
    }
    int rc;
    if ((rc = launch_post_view_segments(rois, R, n_images, views, w.img_lo, w.img_hi, st))) return rc;
    hipLaunchKernelGGL(soft_nms_kernel, dim3(n_images * nc), dim3(SOFT_BLOCK), lds, st, rois, w.img_lo, w.img_hi, scores, boxes,
                       flip_width, R, num_classes, n_images, views, P, score_thresh, min_score, method, nms_thresh, sigma,
                       w.emit, w.n_emit);
    if ((rc = check_launch())) return rc;
    hipLaunchKernelGGL(soft_cap_kernel, dim3(n_images), dim3(SOFT_CAP_BLOCK), 0, st, w.img_lo, w.img_hi, w.emit, w.n_emit, R,
                       num_classes, P, max_per_image, dets, counts);
    return check_launch();
}
