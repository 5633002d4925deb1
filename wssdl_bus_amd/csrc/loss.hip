// Multi-task loss of the supervised images for gfx950: the four terms
// and their gradients in one forward and one backward launch.
//
// Reference: code/lib/fast_rcnn/train_bus.py
//   :186-192 / :605-610  rpn_cross_entropy  mean CE over the anchors whose label != -1
//   :203-210 / :613-620  rpn_loss_box       10 * mean over (image, channel) of
//                        sum_{h,w} out_w * [ 0.5 (3 in_w d)^2 s + (|d| - 0.5/9)(1 - s) ],  s = |d| < 1
//                        (the threshold 1 with the sigma = 3 pieces: the reference's formula as written);
//                        combined mode takes the first IMS_PER_BATCH images only (:613-616)
//   :218 / :623-630      cross_entropy      mean CE over the first len(label) rows of cls_score
//   :231-235 / :641-647  loss_box           mean over those rows of sum_j out_w * in_w * |pred - target|
// In the reference these are ~40 TF element-wise / reduction ops on tensors of at most 0.7 M
// elements (launch-bound); here every element is read once per direction.  Layouts are the layers'
// own: rpn_cls_score [N,H,W,2A] (channel c*A + a; the reshape of network.py:283-291 is an index map:
// row (a*H + h, w) of rpn_cls_score_reshape = channels (a, A + a) of cell (h, w)), rpn_labels
// [N,1,A*H,W] i32, rpn_bbox_pred [N,H,W,4A] against targets / weights [N,4A,H,W].
// Sums are accumulated in f64 per workgroup and combined in a fixed order (same result for the
// same launch shape); label -1 rows of the RoI list are padding (not rows of the reference's blob).
#include "common.hip.h"

#include <math.h>

namespace wssdl {

constexpr int MTL_BLOCK = 256;
constexpr int MTL_ITEMS = 8;                 // elements per thread and term
constexpr int MTL_MAX_CLASSES = 32;

struct MtlState {                            // head of the workspace, read by the backward
    double rpn_count, row_count;             // anchors with label != -1; rows with label != -1
};

__device__ __forceinline__ double block_sum(double v, double *scratch) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < MTL_BLOCK / 64; ++i) s += scratch[i];
    return s;                                // valid on thread 0
}

struct MtlArgs {
    const float *rpn_cls_score;
    const int *rpn_labels;
    const float *rpn_bbox_pred, *rpn_tg, *rpn_inw, *rpn_outw;
    int n_images, n_box_images, H, W, A;
    const float *cls_score;
    const int *labels;
    const float *bbox_pred, *tg, *inw, *outw;
    int n_rows, rows_total, K;
    int nb_cls, nb_box;                      // workgroups of the two RPN terms; one more for the R-CNN terms
};

// label / score addressing of anchor e = ((n*H + h)*W + w)*A + a
__device__ __forceinline__ void rpn_anchor(const MtlArgs &x, long long e, long long &score_off, long long &label_off) {
    const int a = (int)(e % x.A);
    const long long cell = e / x.A;                      // (n*H + h)*W + w
    const int w = (int)(cell % x.W);
    const long long nh = cell / x.W;
    const int h = (int)(nh % x.H);
    const long long n = nh / x.H;
    score_off = cell * (2 * x.A) + a;                    // bg; fg = + A
    label_off = ((n * x.A + a) * x.H + h) * x.W + w;     // [N,1,A*H,W]
}

// element e = ((n*H + h)*W + w)*4A + ch of rpn_bbox_pred  ->  offset in the [N,4A,H,W] tensors
__device__ __forceinline__ long long rpn_target_off(const MtlArgs &x, long long e) {
    const int C4 = 4 * x.A;
    const int ch = (int)(e % C4);
    const long long cell = e / C4;
    const int w = (int)(cell % x.W);
    const long long nh = cell / x.W;
    const int h = (int)(nh % x.H);
    const long long n = nh / x.H;
    return ((n * C4 + ch) * x.H + h) * x.W + w;
}

// The per-element arithmetic of the forward, shared by the batch kernel and the per-image kernel (same f32
// expressions, so the same bits).  One labelled anchor's CE term is added to s and counted in c:
__device__ __forceinline__ void rpn_ce_element(const MtlArgs &x, long long e, double &s, double &c) {
    long long so, lo;
    rpn_anchor(x, e, so, lo);
    const int l = x.rpn_labels[lo];
    if (l < 0) return;
    const float bg = x.rpn_cls_score[so], fg = x.rpn_cls_score[so + x.A];
    // (max - own score) + log1p(...): adding the maximum first and subtracting it again would round the small term away
    s += (double)((fmaxf(bg, fg) - (l ? fg : bg)) + log1pf(expf(-fabsf(bg - fg))));
    c += 1.0;
}

// element e of rpn_bbox_pred: out_w * [0.5 (3 in_w d)^2 or |d| - 0.5/9]
__device__ __forceinline__ double rpn_box_element(const MtlArgs &x, long long e) {
    const long long to = rpn_target_off(x, e);
    const float d = x.rpn_bbox_pred[e] - x.rpn_tg[to];
    const float iw = x.rpn_inw[to], ow = x.rpn_outw[to];
    const float ad = fabsf(d);
    const float q = iw * d * 3.0f;
    const float per = (ad < 1.0f) ? 0.5f * q * q : (ad - (float)(0.5 / 9.0));
    return (double)(ow * per);
}

// CE term of row r against label l in [0, K)
__device__ __forceinline__ double rcnn_ce_row(const MtlArgs &x, int r, int l) {
    const float *sc = x.cls_score + (size_t)r * x.K;
    float m;
    const float lz = lse_minus_max(sc, x.K, &m);
    return (double)((m - sc[l]) + lz);
}

// sum_j out_w * in_w * |pred - target| of row r, added in f32 in column order
__device__ __forceinline__ double rcnn_box_row(const MtlArgs &x, int r) {
    const size_t o = (size_t)r * 4 * x.K;
    float row = 0.0f;
    for (int j = 0; j < 4 * x.K; ++j) row += x.outw[o + j] * (x.inw[o + j] * fabsf(x.bbox_pred[o + j] - x.tg[o + j]));
    return (double)row;
}

// partials: [nb_cls] CE sums, [nb_cls] counts, [nb_box] box sums, then 3 values of the R-CNN block
__global__ __launch_bounds__(MTL_BLOCK) void mtl_forward_kernel(MtlArgs x, double *__restrict__ partials) {
    __shared__ double scratch[MTL_BLOCK / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    if (b < x.nb_cls) {
        const long long total = (long long)x.n_images * x.H * x.W * x.A;
        double s = 0.0, c = 0.0;
        for (int i = 0; i < MTL_ITEMS; ++i) {
            const long long e = ((long long)b * MTL_ITEMS + i) * MTL_BLOCK + t;
            if (e >= total) break;
            rpn_ce_element(x, e, s, c);
        }
        const double ss = block_sum(s, scratch), cc = block_sum(c, scratch);
        if (t == 0) { partials[b] = ss;  partials[x.nb_cls + b] = cc; }
    } else if (b < x.nb_cls + x.nb_box) {
        const int bb = b - x.nb_cls;
        const long long total = (long long)x.n_box_images * x.H * x.W * 4 * x.A;
        double s = 0.0;
        for (int i = 0; i < MTL_ITEMS; ++i) {
            const long long e = ((long long)bb * MTL_ITEMS + i) * MTL_BLOCK + t;
            if (e >= total) break;
            s += rpn_box_element(x, e);
        }
        const double ss = block_sum(s, scratch);
        if (t == 0) partials[2 * x.nb_cls + bb] = ss;
    } else {
        // R-CNN terms: one workgroup, a thread per row
        double ce = 0.0, cnt = 0.0, box = 0.0;
        for (int r = t; r < x.n_rows; r += MTL_BLOCK) {
            const int l = x.labels[r];
            if (l >= 0 && l < x.K) {       // (a label outside [0, K) is ignored like padding, not read through)
                ce += rcnn_ce_row(x, r, l);
                cnt += 1.0;
            }
            box += rcnn_box_row(x, r);
        }
        const double a = block_sum(ce, scratch), c = block_sum(cnt, scratch), d = block_sum(box, scratch);
        if (t == 0) {
            double *p = partials + 2 * x.nb_cls + x.nb_box;
            p[0] = a;  p[1] = c;  p[2] = d;
        }
    }
}

// The four values from one set of partials (the batch's, or one image's): workgroup sums in index order per thread,
// then block_sum.  rcnn = the 3 values of the R-CNN block.  Valid on thread 0.
struct MtlTerms { float v[4];  double rpn_count, row_count; };

__device__ __forceinline__ MtlTerms finish_terms(const double *__restrict__ ce, const double *__restrict__ cnt,
                                                 const double *__restrict__ box, const double *__restrict__ rcnn,
                                                 int nb_cls, int nb_box, int n_box_images, int A, double *scratch) {
    const int t = threadIdx.x;
    double s = 0.0, c = 0.0, b = 0.0;
    for (int i = t; i < nb_cls; i += MTL_BLOCK) { s += ce[i];  c += cnt[i]; }
    for (int i = t; i < nb_box; i += MTL_BLOCK) b += box[i];
    const double ss = block_sum(s, scratch), cc = block_sum(c, scratch), bb = block_sum(b, scratch);
    MtlTerms o;
    o.rpn_count = cc;
    o.row_count = rcnn[1];
    o.v[0] = (float)(ss / cc);                                               // no labelled anchor: NaN, like the mean of nothing
    o.v[1] = (float)(10.0 * bb / ((double)n_box_images * 4.0 * A));
    o.v[2] = (float)(rcnn[0] / rcnn[1]);
    o.v[3] = (float)(rcnn[2] / (rcnn[1] < 1.0 ? 1.0 : rcnn[1]));
    return o;
}

__global__ __launch_bounds__(MTL_BLOCK) void mtl_finish_kernel(const double *__restrict__ partials, int nb_cls,
                                                               int nb_box, int n_box_images, int A,
                                                               MtlState *__restrict__ state, float *__restrict__ losses) {
    __shared__ double scratch[MTL_BLOCK / 64];
    const MtlTerms o = finish_terms(partials, partials + nb_cls, partials + 2 * nb_cls, partials + 2 * nb_cls + nb_box,
                                    nb_cls, nb_box, n_box_images, A, scratch);
    if (threadIdx.x == 0) {
        state->rpn_count = o.rpn_count;
        state->row_count = o.row_count;
        for (int k = 0; k < 4; ++k) losses[k] = o.v[k];
    }
}

// ---- the four terms per image, forward only (the validation pass: fast_rcnn/train_bus.py:427-534 / :792-899 run the
// training losses on one validation image per step).  Image i is treated as a batch of its own: pc workgroups of
// MTL_BLOCK * MTL_ITEMS anchors starting at the image's first anchor, pb workgroups of box elements likewise, and one
// workgroup that scans ALL rows of the RoI list and keeps those whose image column equals i (rows need not be grouped
// or ordered; an index outside [0, N) matches no workgroup; R is at most a few thousand).  The partials of image i
// are [pc] CE sums, [pc] counts, [pb] box sums, 3 R-CNN values, laid out as the batch kernel's.
struct MtlImageArgs {
    const float *roi_image;                  // image index of row r at roi_image[r * stride] (column 0 of the rois blob)
    int stride;
    int pc, pb;                              // workgroups per image of the two RPN terms
};

__global__ __launch_bounds__(MTL_BLOCK) void mtl_per_image_kernel(MtlArgs x, MtlImageArgs y, double *__restrict__ partials) {
    __shared__ double scratch[MTL_BLOCK / 64];
    const int per = y.pc + y.pb + 1;
    const int img = blockIdx.x / per, j = blockIdx.x % per, t = threadIdx.x;
    double *p = partials + (size_t)img * (2 * y.pc + y.pb + 3);
    if (j < y.pc) {
        const long long n = (long long)x.H * x.W * x.A, base = (long long)img * n;
        double s = 0.0, c = 0.0;
        for (int i = 0; i < MTL_ITEMS; ++i) {
            const long long e = ((long long)j * MTL_ITEMS + i) * MTL_BLOCK + t;
            if (e >= n) break;
            rpn_ce_element(x, base + e, s, c);
        }
        const double ss = block_sum(s, scratch), cc = block_sum(c, scratch);
        if (t == 0) { p[j] = ss;  p[y.pc + j] = cc; }
    } else if (j < y.pc + y.pb) {
        const int jb = j - y.pc;
        const long long n = (long long)x.H * x.W * 4 * x.A, base = (long long)img * n;
        double s = 0.0;
        for (int i = 0; i < MTL_ITEMS; ++i) {
            const long long e = ((long long)jb * MTL_ITEMS + i) * MTL_BLOCK + t;
            if (e >= n) break;
            s += rpn_box_element(x, base + e);
        }
        const double ss = block_sum(s, scratch);
        if (t == 0) p[2 * y.pc + jb] = ss;
    } else {
        // the box sum too is over the labelled rows only (the batch kernel adds every row's; a padding row carries
        // zero weights there)
        const float want = (float)img;
        double ce = 0.0, cnt = 0.0, box = 0.0;
        for (int r = t; r < x.n_rows; r += MTL_BLOCK) {
            const int l = x.labels[r];
            if (y.roi_image[(size_t)r * y.stride] == want && l >= 0 && l < x.K) {
                ce += rcnn_ce_row(x, r, l);
                cnt += 1.0;
                box += rcnn_box_row(x, r);
            }
        }
        const double a = block_sum(ce, scratch), c = block_sum(cnt, scratch), d = block_sum(box, scratch);
        if (t == 0) {
            double *q = p + 2 * y.pc + y.pb;
            q[0] = a;  q[1] = c;  q[2] = d;
        }
    }
}

// one workgroup per image: finish_terms on the image's partials (n_box_images = 1: the image alone)
__global__ __launch_bounds__(MTL_BLOCK) void mtl_per_image_finish_kernel(const double *__restrict__ partials, int pc, int pb,
                                                                         int A, float *__restrict__ losses,
                                                                         float *__restrict__ counts) {
    __shared__ double scratch[MTL_BLOCK / 64];
    const int img = blockIdx.x;
    const double *p = partials + (size_t)img * (2 * pc + pb + 3);
    const MtlTerms o = finish_terms(p, p + pc, p + 2 * pc, p + 2 * pc + pb, pc, pb, 1, A, scratch);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; ++k) losses[img * 4 + k] = o.v[k];
        counts[img * 2] = (float)o.rpn_count;
        counts[img * 2 + 1] = (float)o.row_count;
    }
}

__device__ __forceinline__ float sgnf(float d) { return (d > 0.0f) ? 1.0f : ((d < 0.0f) ? -1.0f : 0.0f); }

__global__ __launch_bounds__(MTL_BLOCK) void mtl_backward_kernel(MtlArgs x, const MtlState *__restrict__ state,
                                                                 const float *__restrict__ gl, float *__restrict__ g_rpn_cls,
                                                                 float *__restrict__ g_rpn_box, float *__restrict__ g_cls,
                                                                 float *__restrict__ g_box) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b < x.nb_cls) {
        const long long total = (long long)x.n_images * x.H * x.W * x.A;
        const float scale = (state->rpn_count > 0.0) ? (float)((double)gl[0] / state->rpn_count) : 0.0f;
        for (int i = 0; i < MTL_ITEMS; ++i) {
            const long long e = ((long long)b * MTL_ITEMS + i) * MTL_BLOCK + t;
            if (e >= total) break;
            long long so, lo;
            rpn_anchor(x, e, so, lo);
            const int l = x.rpn_labels[lo];
            float gb = 0.0f, gf = 0.0f;
            if (l >= 0) {
                const float bg = x.rpn_cls_score[so], fg = x.rpn_cls_score[so + x.A];
                // softmax in the difference form expf((s_k - max) - lz), lz = log(sum) - max as in the forward: s_k - max
                // is exactly 0 for the larger score and -|bg - fg| for the other.  Forming max + lz first would round
                // ulp(|max|) / 2 into the exponent, an error that grows with the scores' common offset
                const float dlt = -fabsf(bg - fg);
                const float lz = log1pf(expf(dlt));
                const float phi = expf(0.0f - lz), plo = expf(dlt - lz);
                // (two classes: the label's component is minus the other class's probability)
                const float pb = (bg >= fg) ? phi : plo, pf = (bg >= fg) ? plo : phi;
                gb = (l == 0 ? -pf : pb) * scale;
                gf = (l == 1 ? -pb : pf) * scale;
            }
            g_rpn_cls[so] = gb;
            g_rpn_cls[so + x.A] = gf;
        }
    } else if (b < x.nb_cls + x.nb_box) {
        // (covers ALL images: the ones beyond n_box_images get zeros)
        const int bb = b - x.nb_cls;
        const long long total = (long long)x.n_images * x.H * x.W * 4 * x.A;
        const long long live = (long long)x.n_box_images * x.H * x.W * 4 * x.A;
        const float scale = (float)(10.0 * (double)gl[1] / ((double)x.n_box_images * 4.0 * x.A));
        for (int i = 0; i < MTL_ITEMS; ++i) {
            const long long e = ((long long)bb * MTL_ITEMS + i) * MTL_BLOCK + t;
            if (e >= total) break;
            float g = 0.0f;
            if (e < live) {
                const long long to = rpn_target_off(x, e);
                const float d = x.rpn_bbox_pred[e] - x.rpn_tg[to];
                const float iw = x.rpn_inw[to], ow = x.rpn_outw[to];
                g = ow * ((fabsf(d) < 1.0f) ? 9.0f * iw * iw * d : sgnf(d)) * scale;
            }
            g_rpn_box[e] = g;
        }
    } else {
        const float sc_ce = (state->row_count > 0.0) ? (float)((double)gl[2] / state->row_count) : 0.0f;
        const float sc_box = (float)((double)gl[3] / (state->row_count < 1.0 ? 1.0 : state->row_count));
        // a thread per row, a workgroup per MTL_BLOCK rows (one workgroup for all 8512 rows of a combined step
        // was a 32 us chain)
        const int r = (b - x.nb_cls - x.nb_box) * MTL_BLOCK + t;
        if (r < x.rows_total) {
            float *gc = g_cls + (size_t)r * x.K;
            float *gb = g_box + (size_t)r * 4 * x.K;
            const int l = (r < x.n_rows) ? x.labels[r] : -1;
            if (l >= 0 && l < x.K) {
                const float *sc = x.cls_score + (size_t)r * x.K;
                float m;
                const float lz = lse_minus_max(sc, x.K, &m);
                // (difference form, see the RPN term above; the label's component as -(sum of the other
                // probabilities): accurate when p_l -> 1)
                float others = 0.0f;
                for (int k = 0; k < x.K; ++k) {
                    const float pk = expf((sc[k] - m) - lz);
                    gc[k] = pk * sc_ce;
                    others += (k == l) ? 0.0f : pk;
                }
                gc[l] = -others * sc_ce;
            } else {
                for (int k = 0; k < x.K; ++k) gc[k] = 0.0f;
            }
            if (r < x.n_rows) {
                const size_t o = (size_t)r * 4 * x.K;
                for (int j = 0; j < 4 * x.K; ++j)
                    gb[j] = x.outw[o + j] * x.inw[o + j] * sgnf(x.bbox_pred[o + j] - x.tg[o + j]) * sc_box;
            } else {
                for (int j = 0; j < 4 * x.K; ++j) gb[j] = 0.0f;
            }
        }
    }
}

// expf / log1pf as the kernels of this file get them, element by element (wssdl_loss_libm_probe)
__global__ __launch_bounds__(MTL_BLOCK) void libm_probe_kernel(const float *__restrict__ x, long long n, int which,
                                                               float *__restrict__ y) {
    const long long i = (long long)blockIdx.x * MTL_BLOCK + threadIdx.x;
    if (i < n) y[i] = which ? log1pf(x[i]) : expf(x[i]);
}

static int fill_args(MtlArgs *x, const float *rpn_cls_score, const int32_t *rpn_labels, const float *rpn_bbox_pred,
                     const float *rpn_tg, const float *rpn_inw, const float *rpn_outw, int n_images, int n_box_images,
                     int H, int W, int A, const float *cls_score, const int32_t *labels, const float *bbox_pred,
                     const float *tg, const float *inw, const float *outw, int n_rows, int rows_total, int K,
                     bool backward) {
    if (n_images < 1 || n_box_images < 1 || n_box_images > n_images || H < 1 || W < 1 || A < 1 || A > WSSDL_MAX_ANCHORS)
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (n_rows < 0 || rows_total < n_rows || K < 2 || K > MTL_MAX_CLASSES) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!rpn_cls_score || !rpn_labels || !rpn_bbox_pred || !rpn_tg || !rpn_inw || !rpn_outw) return WSSDL_ERR_INVALID_ARGUMENT;
    if (n_rows > 0 && (!cls_score || !labels || !bbox_pred || !tg || !inw || !outw)) return WSSDL_ERR_INVALID_ARGUMENT;
    const long long anchors = (long long)n_images * H * W * A;
    if (anchors * 4 > 0x7fffffffLL * (long long)MTL_ITEMS) return WSSDL_ERR_INVALID_ARGUMENT;
    x->rpn_cls_score = rpn_cls_score;  x->rpn_labels = rpn_labels;  x->rpn_bbox_pred = rpn_bbox_pred;
    x->rpn_tg = rpn_tg;  x->rpn_inw = rpn_inw;  x->rpn_outw = rpn_outw;
    x->n_images = n_images;  x->n_box_images = n_box_images;  x->H = H;  x->W = W;  x->A = A;
    x->cls_score = cls_score;  x->labels = labels;  x->bbox_pred = bbox_pred;  x->tg = tg;  x->inw = inw;  x->outw = outw;
    x->n_rows = n_rows;  x->rows_total = rows_total;  x->K = K;
    const long long per = (long long)MTL_BLOCK * MTL_ITEMS;
    x->nb_cls = (int)((anchors + per - 1) / per);
    // the backward writes the box gradient of every image, the forward only reads the first n_box_images
    const long long box_elems = (long long)(backward ? n_images : n_box_images) * H * W * 4 * A;
    x->nb_box = (int)((box_elems + per - 1) / per);
    return WSSDL_OK;
}

static size_t mtl_workspace(int n_images, int H, int W, int A) {
    const long long per = (long long)MTL_BLOCK * MTL_ITEMS;
    const long long nb_cls = ((long long)n_images * H * W * A + per - 1) / per;
    const long long nb_box = ((long long)n_images * H * W * 4 * A + per - 1) / per;
    return 256 + sizeof(double) * (size_t)(2 * nb_cls + nb_box + 4);
}

static long long mtl_blocks(long long elements) {
    const long long per = (long long)MTL_BLOCK * MTL_ITEMS;
    return (elements + per - 1) / per;
}

static size_t mtl_per_image_workspace(int n_images, int H, int W, int A) {
    const long long pc = mtl_blocks((long long)H * W * A), pb = mtl_blocks((long long)H * W * 4 * A);
    return sizeof(double) * (size_t)n_images * (size_t)(2 * pc + pb + 3);
}

}  // namespace wssdl

using namespace wssdl;

extern "C" size_t wssdl_multi_task_loss_workspace_bytes(int n_images, int H, int W, int A) {
    if (n_images < 1 || H < 1 || W < 1 || A < 1) return 0;
    return mtl_workspace(n_images, H, W, A);
}

extern "C" int wssdl_multi_task_loss_forward(
    const float *rpn_cls_score, const int32_t *rpn_labels, const float *rpn_bbox_pred, const float *rpn_bbox_targets,
    const float *rpn_inside_w, const float *rpn_outside_w, int n_images, int n_box_images, int H, int W, int A,
    const float *cls_score, const int32_t *labels, const float *bbox_pred, const float *bbox_targets,
    const float *bbox_inside_w, const float *bbox_outside_w, int n_rows, int num_classes, float *losses,
    void *workspace, size_t workspace_bytes, wssdl_stream_t stream) {
    MtlArgs x;
    int rc = fill_args(&x, rpn_cls_score, rpn_labels, rpn_bbox_pred, rpn_bbox_targets, rpn_inside_w, rpn_outside_w,
                       n_images, n_box_images, H, W, A, cls_score, labels, bbox_pred, bbox_targets, bbox_inside_w,
                       bbox_outside_w, n_rows, n_rows, num_classes, false);
    if (rc) return rc;
    if (!losses || !workspace) return WSSDL_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < mtl_workspace(n_images, H, W, A)) return WSSDL_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    MtlState *state = static_cast<MtlState *>(workspace);
    double *partials = reinterpret_cast<double *>(static_cast<char *>(workspace) + 256);
    hipLaunchKernelGGL(mtl_forward_kernel, dim3(x.nb_cls + x.nb_box + 1), dim3(MTL_BLOCK), 0, st, x, partials);
    if ((rc = check_launch())) return rc;
    hipLaunchKernelGGL(mtl_finish_kernel, dim3(1), dim3(MTL_BLOCK), 0, st, partials, x.nb_cls, x.nb_box, n_box_images, A,
                       state, losses);
    return check_launch();
}

extern "C" size_t wssdl_multi_task_loss_per_image_workspace_bytes(int n_images, int H, int W, int A) {
    if (n_images < 1 || H < 1 || W < 1 || A < 1) return 0;
    return mtl_per_image_workspace(n_images, H, W, A);
}

extern "C" int wssdl_multi_task_loss_per_image(
    const float *rpn_cls_score, const int32_t *rpn_labels, const float *rpn_bbox_pred, const float *rpn_bbox_targets,
    const float *rpn_inside_w, const float *rpn_outside_w, int n_images, int H, int W, int A, const float *cls_score,
    const int32_t *labels, const float *bbox_pred, const float *bbox_targets, const float *bbox_inside_w,
    const float *bbox_outside_w, int n_rows, int num_classes, const float *roi_image, int roi_image_stride,
    float *losses, float *counts, void *workspace, size_t workspace_bytes, wssdl_stream_t stream) {
    MtlArgs x;
    int rc = fill_args(&x, rpn_cls_score, rpn_labels, rpn_bbox_pred, rpn_bbox_targets, rpn_inside_w, rpn_outside_w,
                       n_images, n_images, H, W, A, cls_score, labels, bbox_pred, bbox_targets, bbox_inside_w,
                       bbox_outside_w, n_rows, n_rows, num_classes, false);
    if (rc) return rc;
    if (!losses || !counts || !workspace || roi_image_stride < 1 || (n_rows > 0 && !roi_image))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < mtl_per_image_workspace(n_images, H, W, A)) return WSSDL_ERR_INVALID_ARGUMENT;
    MtlImageArgs y;
    y.roi_image = roi_image;  y.stride = roi_image_stride;
    y.pc = (int)mtl_blocks((long long)H * W * A);
    y.pb = (int)mtl_blocks((long long)H * W * 4 * A);
    const long long grid = (long long)n_images * (y.pc + y.pb + 1);
    if (grid > 0x7fffffffLL) return WSSDL_ERR_INVALID_ARGUMENT;
    hipStream_t st = as_stream(stream);
    double *partials = static_cast<double *>(workspace);
    hipLaunchKernelGGL(mtl_per_image_kernel, dim3((unsigned)grid), dim3(MTL_BLOCK), 0, st, x, y, partials);
    if ((rc = check_launch())) return rc;
    hipLaunchKernelGGL(mtl_per_image_finish_kernel, dim3(n_images), dim3(MTL_BLOCK), 0, st, partials, y.pc, y.pb, A, losses,
                       counts);
    return check_launch();
}

extern "C" int wssdl_multi_task_loss_backward(
    const float *rpn_cls_score, const int32_t *rpn_labels, const float *rpn_bbox_pred, const float *rpn_bbox_targets,
    const float *rpn_inside_w, const float *rpn_outside_w, int n_images, int n_box_images, int H, int W, int A,
    const float *cls_score, const int32_t *labels, const float *bbox_pred, const float *bbox_targets,
    const float *bbox_inside_w, const float *bbox_outside_w, int n_rows, int rows_total, int num_classes,
    const float *grad_losses, const void *workspace, float *grad_rpn_cls_score, float *grad_rpn_bbox_pred,
    float *grad_cls_score, float *grad_bbox_pred, wssdl_stream_t stream) {
    MtlArgs x;
    int rc = fill_args(&x, rpn_cls_score, rpn_labels, rpn_bbox_pred, rpn_bbox_targets, rpn_inside_w, rpn_outside_w,
                       n_images, n_box_images, H, W, A, cls_score, labels, bbox_pred, bbox_targets, bbox_inside_w,
                       bbox_outside_w, n_rows, rows_total, num_classes, true);
    if (rc) return rc;
    if (!grad_losses || !workspace || !grad_rpn_cls_score || !grad_rpn_bbox_pred) return WSSDL_ERR_INVALID_ARGUMENT;
    if (rows_total > 0 && (!grad_cls_score || !grad_bbox_pred)) return WSSDL_ERR_INVALID_ARGUMENT;
    const int row_blocks = rows_total > 0 ? cdiv(rows_total, MTL_BLOCK) : 0;
    hipLaunchKernelGGL(mtl_backward_kernel, dim3(x.nb_cls + x.nb_box + row_blocks), dim3(MTL_BLOCK), 0, as_stream(stream), x,
                       static_cast<const MtlState *>(workspace), grad_losses, grad_rpn_cls_score, grad_rpn_bbox_pred,
                       grad_cls_score, grad_bbox_pred);
    return check_launch();
}

extern "C" int wssdl_loss_libm_probe(const float *x, int64_t n, int which, float *y, wssdl_stream_t stream) {
    if (n < 0 || n > 0x7fffffffLL || which < 0 || which > 1) return WSSDL_ERR_INVALID_ARGUMENT;
    if (n == 0) return WSSDL_OK;
    if (!x || !y) return WSSDL_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(libm_probe_kernel, dim3(cdiv(n, MTL_BLOCK)), dim3(MTL_BLOCK), 0, as_stream(stream), x, n, which, y);
    return check_launch();
}
