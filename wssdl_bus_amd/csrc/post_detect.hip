// f3: the post-detection step of the test path as ONE call, batched over the classes and the images.
//
// Reference: code/lib/fast_rcnn/test_bus.py:360-401.  For every class j >= 1:
//   inds = where(scores[:, j] > thresh); cls_dets = hstack(boxes[inds, 4j:4j+4], scores[inds, j]) (f32);
//   keep = nms(cls_dets, cfg.TEST.NMS)  (utils/cython_nms == the cpu_nms rule: f32 arithmetic, f64 compare,
//   candidates in descending score order); cls_dets = cls_dets[keep].
// Then the cap (:389-396): if more than max_per_image detections are left over all classes,
//   image_thresh = sort(all scores)[-max_per_image]  and every class keeps its rows with score >= image_thresh.
//
// Here the (image, class) pairs play the role the images play in the proposal layer: one "segment" per pair, of
// pitch P = max_rows_per_image, and one set of launches ranks, gathers and runs mask + sweep for all of them
// (nms.hip); the score filter is a zero key (no host read-back of `inds`), and the cap is a radix select over the
// kept scores of one image (select.hip.h), one workgroup per image.  A class's kept rows are in descending score
// order, so "score >= image_thresh" keeps a PREFIX of them: the op writes dets[i, c] = the kept rows in that order
// and counts[i, c] = the length of the prefix.
//
// The rows of image i are the contiguous run of the RoI blob whose batch index is i; a small kernel finds each run
// on the device (post_segments_kernel).  Inside a segment a row is named by its index LOCAL to its image (row -
// start): the keys' tie-break and the kept list are then those of the single-image call on that image's rows, so
// every image's output is bit for bit the one wssdl_post_detections gives on its rows alone.
// wssdl_post_detections itself is the one-image case (no RoI blob: rows 0 .. R-1, P = R).
//
// Class-agnostic variant (cfg.TEST.CLS_AGNOSTIC_NMS, test_bus.py:371-384): after the per-class step the classes'
// kept rows are concatenated in class order and a second NMS runs over that union; class j keeps the union's
// survivors that came from it.  Here the union of one image is one more segment, of pitch U = (K-1) * P (padded to
// a multiple of 16): item u = c * P + p is kept position p of class c, ranked by score_key(score, u).  u grows with
// the position in the reference's concatenation, so the order -- ties included -- is that of the NMS on the
// compacted array, whatever P is: the batched and the single-image call agree bit for bit here too.  The same
// ranking and mask + sweep launches run over the n_images union segments, and one workgroup per image takes the cap
// from the union's kept list and splits that list by class (c = u / P) in order.
#include "box_iou.hip.h"
#include "nms.hip.h"
#include "post_views.hip.h"
#include "select.hip.h"

namespace wssdl {

struct PostWs {
    unsigned long long *keys, *cand, *thresh, *mask, *summ;
    float *boxes, *sorted_boxes;
    int *sorted_index, *n_sorted, *cand_fill, *kept, *keep, *num_keep;
    int *img_lo, *img_hi;       // per image: first and last row of its run in the RoI blob (batched calls)
};

// nseg = n_images * nc segments of P rows each
static void carve_segments(Carver &c, int n_images, int P, int nc, PostWs &w) {
    const int ncb = nms_mask_pitch(P);
    const size_t nseg = (size_t)n_images * nc;
    w.keys = c.take<unsigned long long>(nseg * P);
    w.cand = c.take<unsigned long long>(nseg * P);
    w.thresh = c.take<unsigned long long>(nseg + 32);
    w.sorted_index = c.take<int>(nseg * P);
    w.n_sorted = c.take<int>(nseg + 64);
    w.cand_fill = c.take<int>(nseg + 64);
    w.kept = c.take<int>(nseg * ((size_t)P + 64));
    w.keep = c.take<int>(nseg * P);
    w.num_keep = c.take<int>(nseg + 64);
    w.boxes = c.take<float>(nseg * P * 4);
    w.sorted_boxes = c.take<float>(nseg * P * 4);
    w.mask = c.take<unsigned long long>(nseg * P * ncb);
    w.summ = c.take<unsigned long long>(nms_summary_alloc_words((int)nseg, P));
    w.img_lo = c.take<int>((size_t)n_images + 64);
    w.img_hi = c.take<int>((size_t)n_images + 64);
}

// the (image, class) segments of the per-class step: nc = num_classes - 1
static size_t carve_post(void *ws, int n_images, int P, int nc, PostWs *out) {
    Carver c(ws);
    PostWs w;
    carve_segments(c, n_images, P, nc, w);
    if (out) *out = w;
    return c.off;
}

// image of RoI row r: its batch index if in [0, n_images), -1 otherwise (dead padding rows, NaN, foreign images)
__device__ __forceinline__ int roi_image(const float *__restrict__ rois, int r, int n_images) {
    const float b = rois[(size_t)r * 5];
    return (b >= 0.0f && b < (float)n_images) ? (int)b : -1;
}

// One workgroup: the first and last row of every image's run (the ends of a run are the rows whose neighbour
// belongs to another image or to none).  Images without rows keep lo = INT_MAX, hi = -1.
constexpr int SEG_BLOCK = 1024;

__global__ __launch_bounds__(SEG_BLOCK) void post_segments_kernel(const float *__restrict__ rois, int R, int n_images,
                                                                   int *__restrict__ lo, int *__restrict__ hi) {
    const int t = threadIdx.x;
    for (int i = t; i < n_images; i += SEG_BLOCK) {
        lo[i] = 0x7fffffff;
        hi[i] = -1;
    }
    __syncthreads();
    for (int r = t; r < R; r += SEG_BLOCK) {
        const int b = roi_image(rois, r, n_images);
        if (b < 0) continue;
        if (r == 0 || roi_image(rois, r - 1, n_images) != b) atomicMin(&lo[b], r);
        if (r == R - 1 || roi_image(rois, r + 1, n_images) != b) atomicMax(&hi[b], r);
    }
}

// keys of segment (img, c = j - 1): score_key(score, local row) for the image's rows above the score threshold,
// 0 otherwise; the class's box columns side by side; the initialisations the ranking expects
__global__ __launch_bounds__(256) void post_keys_kernel(const float *__restrict__ rois, const int *__restrict__ lo,
                                                        const int *__restrict__ hi, const float *__restrict__ scores,
                                                        const float *__restrict__ boxes, int R, int K, int n_images, int P,
                                                        float score_thresh, unsigned long long *__restrict__ keys,
                                                        float *__restrict__ cboxes, int *__restrict__ sorted_index,
                                                        int *__restrict__ n_sorted, int *__restrict__ cand_fill) {
    const int nc = K - 1;
    const long long nseg = (long long)n_images * nc;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nseg) { n_sorted[i] = 0;  cand_fill[i] = 0; }
    if (i >= nseg * P) return;
    const int seg = (int)(i / P), p = (int)(i - (long long)seg * P);
    const int img = seg / nc, c = seg - img * nc;
    int start, count;
    image_rows(lo, hi, img, R, start, count);
    sorted_index[i] = -1;
    const int r = start + p;
    if (p >= count || (rois && roi_image(rois, r, n_images) != img)) {
        keys[i] = 0ull;
        return;
    }
    const float s = scores[(size_t)r * K + c + 1];
    keys[i] = (s > score_thresh) ? score_key(s, (unsigned)p) : 0ull;        // NaN fails the test like np.where
    const float *b = boxes + (size_t)r * 4 * K + 4 * (c + 1);
    float *o = cboxes + (size_t)i * 4;
    o[0] = b[0];  o[1] = b[1];  o[2] = b[2];  o[3] = b[3];
}

__global__ __launch_bounds__(256) void post_gather_kernel(const float *__restrict__ cboxes, const int *__restrict__ sorted_index,
                                                          const int *__restrict__ n_sorted, int P, int nseg,
                                                          float *__restrict__ sorted_boxes) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nseg * P) return;
    const int seg = (int)(i / P), p = (int)(i - (long long)seg * P);
    if (p >= n_sorted[seg]) return;
    const float *b = cboxes + ((size_t)seg * P + sorted_index[i]) * 4;
    float *o = sorted_boxes + (size_t)i * 4;
    o[0] = b[0];  o[1] = b[1];  o[2] = b[2];  o[3] = b[3];
}

// One workgroup per image: the max_per_image-th largest kept score over the image's classes
// (test_bus.py:389-392), then its rows.  An image with more rows than P reports counts[i, 0] = -1.
constexpr int CAP_BLOCK = 1024;
constexpr int CAP_LIST = 512;

__global__ __launch_bounds__(CAP_BLOCK) void post_cap_kernel(const int *__restrict__ lo, const int *__restrict__ hi,
                                                             const float *__restrict__ scores, const float *__restrict__ cboxes,
                                                             const int *__restrict__ keep, const int *__restrict__ num_keep,
                                                             int R, int K, int P, int max_per_image, float *__restrict__ dets,
                                                             int *__restrict__ counts) {
    __shared__ SelectScratch<CAP_LIST> sc;
    __shared__ int s_count[64];
    const int nc = K - 1, t = threadIdx.x, img = blockIdx.x;
    int start, count;
    image_rows(lo, hi, img, R, start, count);
    const size_t seg0 = (size_t)img * nc;
    if (count > P) {            // the same for the whole workgroup: no barrier is skipped by part of it
        if (t < nc) counts[seg0 + t] = t == 0 ? -1 : 0;
        return;
    }
    const int *nk = num_keep + seg0;
    const int *kp = keep + seg0 * P;
    const float *cb = cboxes + seg0 * P * 4;
    const float *sc_rows = scores + (size_t)start * K;
    float *d = dets + seg0 * P * 5;
    if (t < 64) s_count[t] = 0;
    // item i = (class c, kept position p); its key: score bits over a unique low word
    auto key_at = [&](int i, unsigned long long &v) -> bool {
        const int c = i / P, p = i - c * P;
        if (p >= nk[c]) return false;
        const int row = kp[(size_t)c * P + p];
        v = score_key(sc_rows[(size_t)row * K + c + 1], (unsigned)i);
        return true;
    };
    int members = 0;
    const unsigned long long kth = block_radix_select<CAP_BLOCK, CAP_LIST, true>(
        key_at, nc * P, [max_per_image](int m) { return (max_per_image > 0 && m > max_per_image) ? max_per_image : 0; }, sc,
        &members);
    // image_thresh as order-preserving score bits (0: no cap -- every kept row passes)
    const unsigned cut = (unsigned)(kth >> 32);
    __syncthreads();
    for (int i = t; i < nc * P; i += CAP_BLOCK) {
        const int c = i / P, p = i - c * P;
        if (p >= nk[c]) continue;
        const int row = kp[(size_t)c * P + p];
        const float s = sc_rows[(size_t)row * K + c + 1];
        const float *b = cb + ((size_t)c * P + row) * 4;
        float *o = d + (size_t)i * 5;
        o[0] = b[0];  o[1] = b[1];  o[2] = b[2];  o[3] = b[3];  o[4] = s;
        if ((unsigned)(score_key(s, 0u) >> 32) >= cut && c < 64) atomicAdd(&s_count[c], 1);     // a prefix: rows are in descending order
    }
    __syncthreads();
    if (t < nc && t < 64) counts[seg0 + t] = s_count[t];
}

// ---------------------------------------------------------------------------------- class-agnostic union ---
// union pitch: (K-1) * P padded to a multiple of 16 (the alignment contract of the fused mask + sweep, nms.hip.h)
static int union_pitch(int P, int nc) { return (int)(((long long)nc * P + 15) / 16 * 16); }

// the per-class slices first (the same offsets as the per-class op), behind them the same set for one segment of
// pitch U per image (its img_lo / img_hi, 2 x 256-byte slices for up to 64 images, stay unused: the union reads the
// per-class pair), and the union's scores [n_images, U].
// The union's boxes and scores are written for the items with a non-zero key only.  Nothing else is read: the box
// gather reads boxes[sorted_index[q]] for q < n_sorted, and sorted_index[q] is the low word of a non-zero key; the
// cap kernel reads item keep[q] for q < num_keep, a value of sorted_index.
static size_t carve_post_agnostic(void *ws, int n_images, int P, int nc, PostWs *pw, PostWs *uw, float **uscores) {
    Carver c(ws);
    PostWs w, u;
    const int U = union_pitch(P, nc);
    carve_segments(c, n_images, P, nc, w);
    carve_segments(c, n_images, U, 1, u);
    float *us = c.take<float>((size_t)n_images * U);
    if (pw) *pw = w;
    if (uw) *uw = u;
    if (uscores) *uscores = us;
    return c.off;
}

// keys of image img's union segment: item u = c * P + p is kept position p of class c -> score_key(score, u), its
// box and its score side by side; 0 for p >= num_keep[c], for the padding beyond (K-1) * P and for a kept entry
// that does not name a row of the image.  Also the initialisations the ranking expects.
__global__ __launch_bounds__(256) void post_union_keys_kernel(const int *__restrict__ lo, const int *__restrict__ hi,
                                                              const float *__restrict__ scores, const float *__restrict__ cboxes,
                                                              const int *__restrict__ keep, const int *__restrict__ num_keep,
                                                              int R, int K, int n_images, int P, int U,
                                                              unsigned long long *__restrict__ ukeys, float *__restrict__ uboxes,
                                                              float *__restrict__ uscores, int *__restrict__ sorted_index,
                                                              int *__restrict__ n_sorted, int *__restrict__ cand_fill) {
    const int nc = K - 1;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_images) { n_sorted[i] = 0;  cand_fill[i] = 0; }
    if (i >= (long long)n_images * U) return;
    const int img = (int)(i / U), u = (int)(i - (long long)img * U);
    sorted_index[i] = -1;
    ukeys[i] = 0ull;
    if (u >= nc * P) return;
    const int c = u / P, p = u - c * P;
    const size_t seg = (size_t)img * nc + c;
    if (p >= num_keep[seg]) return;
    int start, count;
    image_rows(lo, hi, img, R, start, count);
    const int row = keep[seg * P + p];
    if (row < 0 || row >= P || row >= count) return;
    const float s = scores[((size_t)start + row) * K + c + 1];
    const float *b = cboxes + (seg * P + row) * 4;
    float *o = uboxes + (size_t)i * 4;
    o[0] = b[0];  o[1] = b[1];  o[2] = b[2];  o[3] = b[3];
    uscores[i] = s;
    ukeys[i] = score_key(s, (unsigned)u);
}

// One workgroup per image: the max_per_image-th largest score of the union's kept list (test_bus.py:389-392), then
// the list split by class: kept position q holds item u = c * P + p, and class c receives its items in the order
// of the list, so every class stays in descending score order and "score >= image_thresh" keeps a prefix of it.
// An image with more rows than P reports counts[i, 0] = -1.
constexpr int CAP_WAVES = CAP_BLOCK / 64;

__global__ __launch_bounds__(CAP_BLOCK) void post_union_cap_kernel(const int *__restrict__ lo, const int *__restrict__ hi,
                                                                   const float *__restrict__ uboxes, const float *__restrict__ uscores,
                                                                   const int *__restrict__ ukeep, const int *__restrict__ unum_keep,
                                                                   int R, int K, int P, int U, int max_per_image,
                                                                   float *__restrict__ dets, int *__restrict__ counts) {
    __shared__ SelectScratch<CAP_LIST> sc;
    __shared__ int s_count[64], s_base[64];
    __shared__ int s_wave[CAP_WAVES][64];
    const int nc = K - 1, t = threadIdx.x, img = blockIdx.x, lane = t & 63, wave = t >> 6;
    int start, count;
    image_rows(lo, hi, img, R, start, count);
    const size_t seg0 = (size_t)img * nc;
    if (count > P) {            // the same for the whole workgroup: no barrier is skipped by part of it
        if (t < nc) counts[seg0 + t] = t == 0 ? -1 : 0;
        return;
    }
    const int live = nc * P;                                     // items of the union; U - live padding slots
    const int nk = min(max(unum_keep[img], 0), live);
    const int *kp = ukeep + (size_t)img * U;
    const float *ub = uboxes + (size_t)img * U * 4;
    const float *us = uscores + (size_t)img * U;
    float *d = dets + seg0 * P * 5;
    if (t < 64) { s_count[t] = 0;  s_base[t] = 0; }
    // item q = kept position q of the union; its key: score bits over a unique low word
    auto key_at = [&](int q, unsigned long long &v) -> bool {
        if (q >= nk) return false;
        const int u = kp[q];
        if ((unsigned)u >= (unsigned)live) return false;
        v = score_key(us[u], (unsigned)q);
        return true;
    };
    const unsigned long long kth = block_radix_select<CAP_BLOCK, CAP_LIST, true>(
        key_at, nk, [max_per_image](int m) { return (max_per_image > 0 && m > max_per_image) ? max_per_image : 0; }, sc);
    // image_thresh as order-preserving score bits (0: no cap -- every kept row passes)
    const unsigned cut = (unsigned)(kth >> 32);
    __syncthreads();
    for (int q0 = 0; q0 < nk; q0 += CAP_BLOCK) {                 // nk is the same for the whole workgroup
        const int q = q0 + t;
        int u = q < nk ? kp[q] : -1;
        const bool valid = (unsigned)u < (unsigned)live;
        const int c = valid ? u / P : 0;
        s_wave[wave][lane] = 0;
        // position among the wave's items of the same class, class by class (every lane of the wave takes every turn)
        int before = 0;
        unsigned long long active = __ballot(valid);
        while (active != 0ull) {
            const int leader = __ffsll((long long)active) - 1;
            const int c0 = __builtin_amdgcn_readlane(c, leader);
            const unsigned long long same = __ballot(valid && c == c0);
            if (valid && c == c0) before = __popcll(same & ((1ull << lane) - 1ull));
            if (lane == leader) s_wave[wave][c0] = __popcll(same);
            active &= ~same;
        }
        __syncthreads();
        if (valid) {
            int pos = s_base[c] + before;
            for (int w = 0; w < wave; ++w) pos += s_wave[w][c];
            const float s = us[u];
            if (pos < P) {
                const float *b = ub + (size_t)u * 4;
                float *o = d + ((size_t)c * P + pos) * 5;
                o[0] = b[0];  o[1] = b[1];  o[2] = b[2];  o[3] = b[3];  o[4] = s;
                if ((unsigned)(score_key(s, 0u) >> 32) >= cut) atomicAdd(&s_count[c], 1);    // a prefix: descending order
            }
        }
        __syncthreads();
        if (t < 64) {
            int add = 0;
            for (int w = 0; w < CAP_WAVES; ++w) add += s_wave[w][t];
            s_base[t] += add;
        }
        __syncthreads();
    }
    __syncthreads();
    if (t < nc && t < 64) counts[seg0 + t] = s_count[t];
}

// ------------------------------------------------------- views: flip augmentation and box voting at test time ---
// wssdl_post_detections_views: the blob holds n_images * views SOURCE images, source s = view s % views of output
// image s / views, so the rows of one output image are still one contiguous run.  The segment and key kernels below
// are the two above with the output image in place of the batch index; the key kernel also brings the boxes of a
// mirrored source back into the image's own frame while it copies them into the workspace (the inputs stay as they
// are).  Ranking, sweep, union pass and cap then run unchanged on those copies.  Box voting follows the cap: one wave
// per surviving detection, see post_vote_kernel.  (roi_view_image, unmirror_x: post_views.hip.h)
__global__ __launch_bounds__(SEG_BLOCK) void post_view_segments_kernel(const float *__restrict__ rois, int R, int n_images,
                                                                        int views, int *__restrict__ lo,
                                                                        int *__restrict__ hi) {
    const int t = threadIdx.x;
    for (int i = t; i < n_images; i += SEG_BLOCK) {
        lo[i] = 0x7fffffff;
        hi[i] = -1;
    }
    __syncthreads();
    int src;
    for (int r = t; r < R; r += SEG_BLOCK) {
        const int b = roi_view_image(rois, r, n_images, views, src);
        if (b < 0) continue;
        if (r == 0 || roi_view_image(rois, r - 1, n_images, views, src) != b) atomicMin(&lo[b], r);
        if (r == R - 1 || roi_view_image(rois, r + 1, n_images, views, src) != b) atomicMax(&hi[b], r);
    }
}

// post_keys_kernel over the views of an image; a row of a mirrored source (flip_width[src] = w >= 0) is copied as
//   x1' = max((w - x2) - 1, 0),  x2' = (w - x1) - 1     (wssdl_flip_boxes's two f32 steps, then the clamp)
__global__ __launch_bounds__(256) void post_view_keys_kernel(const float *__restrict__ rois, const int *__restrict__ lo,
                                                             const int *__restrict__ hi, const float *__restrict__ scores,
                                                             const float *__restrict__ boxes,
                                                             const float *__restrict__ flip_width, int R, int K, int n_images,
                                                             int views, int P, float score_thresh,
                                                             unsigned long long *__restrict__ keys, float *__restrict__ cboxes,
                                                             int *__restrict__ sorted_index, int *__restrict__ n_sorted,
                                                             int *__restrict__ cand_fill) {
    const int nc = K - 1;
    const long long nseg = (long long)n_images * nc;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nseg) { n_sorted[i] = 0;  cand_fill[i] = 0; }
    if (i >= nseg * P) return;
    const int seg = (int)(i / P), p = (int)(i - (long long)seg * P);
    const int img = seg / nc, c = seg - img * nc;
    int start, count, src = -1;
    image_rows(lo, hi, img, R, start, count);
    sorted_index[i] = -1;
    const int r = start + p;
    if (p >= count || roi_view_image(rois, r, n_images, views, src) != img) {
        keys[i] = 0ull;
        return;
    }
    const float s = scores[(size_t)r * K + c + 1];
    keys[i] = (s > score_thresh) ? score_key(s, (unsigned)p) : 0ull;        // NaN fails the test like np.where
    const float *b = boxes + (size_t)r * 4 * K + 4 * (c + 1);
    float *o = cboxes + (size_t)i * 4;
    float x1 = b[0], x2 = b[2];
    unmirror_x(flip_width ? flip_width[src] : -1.0f, x1, x2);
    o[0] = x1;  o[1] = b[1];  o[2] = x2;  o[3] = b[3];
}

// Box voting: one wave per detection d that survived NMS and the cap (segment = (image, class), position below the
// segment's count).  The candidates are the segment's rows above the score threshold, pre-NMS and un-mirrored, as
// post_view_keys_kernel left them in the workspace.  64 candidates at a time: every lane takes the f64 overlap of one
// (box_iou.hip.h, the candidate as the box and d as the query), the wave ballots the members (overlap >= vote_thresh),
// and the sums run over the set bits only, lowest first -- ascending row order, the statement's:
//   sw += (double)s_c;  sx[k] += (double)s_c * (double)c[k]        (the product of two f32 is exact in f64)
// d[k] = (float)(sx[k] / sw).  Every lane carries the same sums; lane 0 writes.  A wave reads its own detection and the
// workspace and writes its own detection's four coordinates: no wave reads what another writes.
constexpr int VOTE_BLOCK = 256;

__global__ __launch_bounds__(VOTE_BLOCK) void post_vote_kernel(const float *__restrict__ rois, const int *__restrict__ lo,
                                                               const int *__restrict__ hi, const float *__restrict__ scores,
                                                               const float *__restrict__ cboxes,
                                                               const int *__restrict__ counts, int R, int K, int n_images,
                                                               int views, int P, float score_thresh, double vote_thresh,
                                                               float *__restrict__ dets) {
    const int nc = K - 1, lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * (VOTE_BLOCK / 64) + (threadIdx.x >> 6);
    if (wv >= (long long)n_images * nc * P) return;
    const int seg = (int)(wv / P), pos = (int)(wv - (long long)seg * P);
    if (pos >= counts[seg]) return;                              // the same for the whole wave; -1 (overflow) has no rows
    const int img = seg / nc, c = seg - img * nc;
    int start, count;
    image_rows(lo, hi, img, R, start, count);
    if (count > P) return;
    float *d = dets + ((size_t)seg * P + pos) * 5;
    const double qx1 = d[0], qy1 = d[1], qx2 = d[2], qy2 = d[3];
    const double qarea = box_area_f64(qx1, qy1, qx2, qy2);
    double sw = 0.0, sx0 = 0.0, sx1 = 0.0, sx2 = 0.0, sx3 = 0.0;
    for (int base = 0; base < count; base += 64) {               // count is the same for the whole wave
        const int p = base + lane;
        float s = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
        bool member = false;
        int src;
        if (p < count && roi_view_image(rois, start + p, n_images, views, src) == img) {
            s = scores[(size_t)(start + p) * K + c + 1];
            if (s > score_thresh) {
                const float *b = cboxes + ((size_t)seg * P + p) * 4;
                b0 = b[0];  b1 = b[1];  b2 = b[2];  b3 = b[3];
                member = iou_pair(b0, b1, b2, b3, qx1, qy1, qx2, qy2, qarea) >= vote_thresh;
            }
        }
        unsigned long long m = __ballot(member);
        while (m != 0ull) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const double ws = (double)__shfl(s, l);
            sw += ws;
            sx0 += ws * (double)__shfl(b0, l);
            sx1 += ws * (double)__shfl(b1, l);
            sx2 += ws * (double)__shfl(b2, l);
            sx3 += ws * (double)__shfl(b3, l);
        }
    }
    if (lane == 0 && sw > 0.0) {
        d[0] = (float)(sx0 / sw);
        d[1] = (float)(sx1 / sw);
        d[2] = (float)(sx2 / sw);
        d[3] = (float)(sx3 / sw);
    }
}

int launch_post_view_segments(const float *rois, int R, int n_images, int views, int *lo, int *hi, hipStream_t st) {
    hipLaunchKernelGGL(post_view_segments_kernel, dim3(1), dim3(SEG_BLOCK), 0, st, rois, R, n_images, views, lo, hi);
    return check_launch();
}

// (the limits of the batched form, POST_MAX_ITEMS and POST_MAX_SEGMENTS: post_views.hip.h)
// The union segment of the class-agnostic form: (K-1) * P items per image in one ranking and one mask + sweep with
// max_keep = the segment.  12000 is the segment the proposal layer runs both at; the kept list of the general
// sweep (which takes over beyond 2240 kept) fits LDS up to 15296 entries, the suppression matrix is
// U * nms_mask_pitch(U) words = 18.4 MB per image there.
constexpr long long POST_MAX_UNION = WSSDL_POST_AGNOSTIC_MAX_UNION;
static_assert(POST_MAX_UNION % 16 == 0, "the padded union pitch must not pass the limit");

static int post_detections_run(const float *rois, const float *scores, const float *boxes, int R, int n_images, int P,
                               int num_classes, float score_thresh, double nms_thresh, int max_per_image, float *dets,
                               int32_t *counts, void *workspace, bool agnostic, hipStream_t st, int views = 0,
                               const float *flip_width = nullptr) {
    const int nc = num_classes - 1;
    const int nseg = n_images * nc;
    PostWs w, uw;
    float *uscores = nullptr;
    if (agnostic)
        carve_post_agnostic(workspace, n_images, P, nc, &w, &uw, &uscores);
    else
        carve_post(workspace, n_images, P, nc, &w);
    const int *lo = nullptr, *hi = nullptr;
    const int blocks = cdiv((long long)nseg * P, 256);
    int rc;
    if (views > 0) {            // wssdl_post_detections_views: the output image of a row is its source image / views
        if ((rc = launch_post_view_segments(rois, R, n_images, views, w.img_lo, w.img_hi, st))) return rc;
        lo = w.img_lo;
        hi = w.img_hi;
        hipLaunchKernelGGL(post_view_keys_kernel, dim3(blocks), dim3(256), 0, st, rois, lo, hi, scores, boxes, flip_width, R,
                           num_classes, n_images, views, P, score_thresh, w.keys, w.boxes, w.sorted_index, w.n_sorted,
                           w.cand_fill);
        if ((rc = check_launch())) return rc;
    } else {
        if (rois) {
            hipLaunchKernelGGL(post_segments_kernel, dim3(1), dim3(SEG_BLOCK), 0, st, rois, R, n_images, w.img_lo, w.img_hi);
            if ((rc = check_launch())) return rc;
            lo = w.img_lo;
            hi = w.img_hi;
        }
        hipLaunchKernelGGL(post_keys_kernel, dim3(blocks), dim3(256), 0, st, rois, lo, hi, scores, boxes, R, num_classes,
                           n_images, P, score_thresh, w.keys, w.boxes, w.sorted_index, w.n_sorted, w.cand_fill);
        if ((rc = check_launch())) return rc;
    }
    if ((rc = launch_rank_topk(w.keys, P, nseg, P, w.cand, w.thresh, w.cand_fill, w.sorted_index, w.n_sorted, w.mask,
                               sizeof(unsigned long long) * (size_t)nseg * P * nms_mask_pitch(P), st)))
        return rc;
    hipLaunchKernelGGL(post_gather_kernel, dim3(blocks), dim3(256), 0, st, w.boxes, w.sorted_index, w.n_sorted, P, nseg,
                       w.sorted_boxes);
    if ((rc = check_launch())) return rc;
    // w.cand is free once the ranking is done: it receives the transposed diagonal blocks of the mask
    if ((rc = launch_nms_two_pass(w.sorted_boxes, P * 4, w.n_sorted, P, nseg, nms_thresh, w.mask, w.cand, w.summ, P,
                                  w.sorted_index, P, w.keep, w.num_keep, nullptr, w.kept, nullptr, st)))
        return rc;
    if (agnostic) {
        const int U = union_pitch(P, nc);
        const int ublocks = cdiv((long long)n_images * U, 256);
        hipLaunchKernelGGL(post_union_keys_kernel, dim3(ublocks), dim3(256), 0, st, lo, hi, scores, w.boxes, w.keep,
                           w.num_keep, R, num_classes, n_images, P, U, uw.keys, uw.boxes, uscores, uw.sorted_index,
                           uw.n_sorted, uw.cand_fill);
        if ((rc = check_launch())) return rc;
        if ((rc = launch_rank_topk(uw.keys, U, n_images, U, uw.cand, uw.thresh, uw.cand_fill, uw.sorted_index, uw.n_sorted,
                                   uw.mask, sizeof(unsigned long long) * (size_t)n_images * U * nms_mask_pitch(U), st)))
            return rc;
        hipLaunchKernelGGL(post_gather_kernel, dim3(ublocks), dim3(256), 0, st, uw.boxes, uw.sorted_index, uw.n_sorted, U,
                           n_images, uw.sorted_boxes);
        if ((rc = check_launch())) return rc;
        if ((rc = launch_nms_two_pass(uw.sorted_boxes, U * 4, uw.n_sorted, U, n_images, nms_thresh, uw.mask, uw.cand,
                                      uw.summ, U, uw.sorted_index, U, uw.keep, uw.num_keep, nullptr, uw.kept, nullptr, st)))
            return rc;
        hipLaunchKernelGGL(post_union_cap_kernel, dim3(n_images), dim3(CAP_BLOCK), 0, st, lo, hi, uw.boxes, uscores,
                           uw.keep, uw.num_keep, R, num_classes, P, U, max_per_image, dets, counts);
        return check_launch();
    }
    hipLaunchKernelGGL(post_cap_kernel, dim3(n_images), dim3(CAP_BLOCK), 0, st, lo, hi, scores, w.boxes, w.keep, w.num_keep,
                       R, num_classes, P, max_per_image, dets, counts);
    return check_launch();
}

}  // namespace wssdl

using namespace wssdl;

extern "C" size_t wssdl_post_detections_batched_workspace_bytes(int n_images, int max_rows_per_image, int num_classes) {
    if (n_images < 1 || max_rows_per_image < 1 || num_classes < 2) return 256;
    return carve_post(nullptr, n_images, max_rows_per_image, num_classes - 1, nullptr);
}

extern "C" size_t wssdl_post_detections_workspace_bytes(int R, int num_classes) {
    return wssdl_post_detections_batched_workspace_bytes(1, R, num_classes);
}

extern "C" size_t wssdl_post_detections_agnostic_batched_workspace_bytes(int n_images, int max_rows_per_image, int num_classes) {
    if (n_images < 1 || max_rows_per_image < 1 || num_classes < 2) return 256;
    return carve_post_agnostic(nullptr, n_images, max_rows_per_image, num_classes - 1, nullptr, nullptr, nullptr);
}

extern "C" size_t wssdl_post_detections_agnostic_workspace_bytes(int R, int num_classes) {
    return wssdl_post_detections_agnostic_batched_workspace_bytes(1, R, num_classes);
}

static int post_detections_entry(const float *rois, const float *scores, const float *boxes, int R, int n_images,
                                 int max_rows_per_image, int num_classes, float score_thresh, double nms_thresh,
                                 int max_per_image, float *dets, int32_t *counts, void *workspace, size_t workspace_bytes,
                                 bool agnostic, wssdl_stream_t stream) {
    const int nc = num_classes - 1;
    const int P = max_rows_per_image;
    if (R < 0 || n_images < 0 || num_classes < 2 || nc > 64) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R > 0 && (P < 1 || (long long)n_images * nc * P > POST_MAX_ITEMS || (long long)n_images * nc > POST_MAX_SEGMENTS))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (R > 0 && agnostic && (long long)nc * P > POST_MAX_UNION) return WSSDL_ERR_INVALID_ARGUMENT;
    if (n_images == 0) return WSSDL_OK;
    if (!counts) return WSSDL_ERR_INVALID_ARGUMENT;
    hipStream_t st = as_stream(stream);
    if (R == 0) {
        if (hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_images * nc, st) != hipSuccess) return WSSDL_ERR_LAUNCH;
        return WSSDL_OK;
    }
    if (!scores || !boxes || !dets || !workspace || (!rois && n_images != 1)) return WSSDL_ERR_INVALID_ARGUMENT;
    const size_t need = agnostic ? wssdl_post_detections_agnostic_batched_workspace_bytes(n_images, P, num_classes)
                                 : wssdl_post_detections_batched_workspace_bytes(n_images, P, num_classes);
    if (workspace_bytes < need) return WSSDL_ERR_WORKSPACE;
    return post_detections_run(rois, scores, boxes, R, n_images, P, num_classes, score_thresh, nms_thresh, max_per_image,
                               dets, counts, workspace, agnostic, st);
}

extern "C" int wssdl_post_detections_batched(const float *rois, const float *scores, const float *boxes, int R,
                                             int n_images, int max_rows_per_image, int num_classes, float score_thresh,
                                             double nms_thresh, int max_per_image, float *dets, int32_t *counts,
                                             void *workspace, size_t workspace_bytes, wssdl_stream_t stream) {
    return post_detections_entry(rois, scores, boxes, R, n_images, max_rows_per_image, num_classes, score_thresh, nms_thresh,
                                 max_per_image, dets, counts, workspace, workspace_bytes, false, stream);
}

extern "C" int wssdl_post_detections_agnostic_batched(const float *rois, const float *scores, const float *boxes, int R,
                                                      int n_images, int max_rows_per_image, int num_classes,
                                                      float score_thresh, double nms_thresh, int max_per_image, float *dets,
                                                      int32_t *counts, void *workspace, size_t workspace_bytes,
                                                      wssdl_stream_t stream) {
    return post_detections_entry(rois, scores, boxes, R, n_images, max_rows_per_image, num_classes, score_thresh, nms_thresh,
                                 max_per_image, dets, counts, workspace, workspace_bytes, true, stream);
}

// The workspace is that of the batched op: the class-agnostic one where the shape admits a class-agnostic call, so
// that one query serves both values of `agnostic`.  The un-mirrored boxes are its per-class box slice.
extern "C" size_t wssdl_post_detections_views_workspace_bytes(int n_images, int views, int max_rows_per_image,
                                                              int num_classes) {
    if (n_images < 1 || views < 1 || max_rows_per_image < 1 || num_classes < 2) return 256;
    if ((long long)(num_classes - 1) * max_rows_per_image > POST_MAX_UNION)      // no class-agnostic call at this shape
        return carve_post(nullptr, n_images, max_rows_per_image, num_classes - 1, nullptr);
    return carve_post_agnostic(nullptr, n_images, max_rows_per_image, num_classes - 1, nullptr, nullptr, nullptr);
}

extern "C" int wssdl_post_detections_views(const float *rois, const float *scores, const float *boxes, int R, int n_images,
                                           int views, const float *flip_width, int max_rows_per_image, int num_classes,
                                           float score_thresh, double nms_thresh, int agnostic, double vote_thresh,
                                           int max_per_image, float *dets, int32_t *counts, void *workspace,
                                           size_t workspace_bytes, wssdl_stream_t stream) {
    const int nc = num_classes - 1;
    const int P = max_rows_per_image;
    if (views < 1 || views > POST_MAX_VIEWS) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R < 0 || n_images < 0 || num_classes < 2 || nc > 64) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R > 0 && (P < 1 || (long long)n_images * nc * P > POST_MAX_ITEMS || (long long)n_images * nc > POST_MAX_SEGMENTS))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (R > 0 && agnostic && (long long)nc * P > POST_MAX_UNION) return WSSDL_ERR_INVALID_ARGUMENT;
    if (vote_thresh > 1.0 || vote_thresh != vote_thresh) return WSSDL_ERR_INVALID_ARGUMENT;
    if (vote_thresh > 0.0 && !(score_thresh >= 0.0f)) return WSSDL_ERR_INVALID_ARGUMENT;    // the weights must be positive
    if (n_images == 0) return WSSDL_OK;
    if (!counts) return WSSDL_ERR_INVALID_ARGUMENT;
    hipStream_t st = as_stream(stream);
    if (R == 0) {
        if (hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_images * nc, st) != hipSuccess) return WSSDL_ERR_LAUNCH;
        return WSSDL_OK;
    }
    if (!rois || !scores || !boxes || !dets || !workspace) return WSSDL_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < wssdl_post_detections_views_workspace_bytes(n_images, views, P, num_classes))
        return WSSDL_ERR_WORKSPACE;
    int rc = post_detections_run(rois, scores, boxes, R, n_images, P, num_classes, score_thresh, nms_thresh, max_per_image,
                                 dets, counts, workspace, agnostic != 0, st, views, flip_width);
    if (rc || !(vote_thresh > 0.0)) return rc;
    PostWs w;
    carve_post(workspace, n_images, P, nc, &w);                  // the per-class slices come first in both layouts
    const long long waves = (long long)n_images * nc * P;
    hipLaunchKernelGGL(post_vote_kernel, dim3(cdiv(waves, VOTE_BLOCK / 64)), dim3(VOTE_BLOCK), 0, st, rois, w.img_lo, w.img_hi,
                       scores, w.boxes, counts, R, num_classes, n_images, views, P, score_thresh, vote_thresh, dets);
    return check_launch();
}

extern "C" int wssdl_post_detections(const float *scores, const float *boxes, int R, int num_classes,
                                     float score_thresh, double nms_thresh, int max_per_image, float *dets,
                                     int32_t *counts, void *workspace, size_t workspace_bytes,
                                     wssdl_stream_t stream) {
    if (R < 0 || num_classes < 2 || num_classes - 1 > 64 || !counts) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R == 0) return wssdl_post_detections_batched(nullptr, scores, boxes, 0, 1, 1, num_classes, score_thresh, nms_thresh,
                                                     max_per_image, dets, counts, workspace, workspace_bytes, stream);
    return wssdl_post_detections_batched(nullptr, scores, boxes, R, 1, R, num_classes, score_thresh, nms_thresh,
                                         max_per_image, dets, counts, workspace, workspace_bytes, stream);
}

extern "C" int wssdl_post_detections_agnostic(const float *scores, const float *boxes, int R, int num_classes,
                                              float score_thresh, double nms_thresh, int max_per_image, float *dets,
                                              int32_t *counts, void *workspace, size_t workspace_bytes,
                                              wssdl_stream_t stream) {
    if (R < 0 || num_classes < 2 || num_classes - 1 > 64 || !counts) return WSSDL_ERR_INVALID_ARGUMENT;
    return wssdl_post_detections_agnostic_batched(nullptr, scores, boxes, R, 1, R == 0 ? 1 : R, num_classes, score_thresh,
                                                  nms_thresh, max_per_image, dets, counts, workspace, workspace_bytes,
                                                  stream);
}
