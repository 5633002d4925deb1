// MIL bag functions for gfx950.
//
// Reference: code/lib/mil/core.py:11-46 (get_bag_logit) with its five bag functions:
//   get_mal_max_logit :60-69 (row with the largest class-2 logit), get_ben_max_logit :49-57 (class 1),
//   get_mass_max_logit :88-96 (smallest class-0 logit), get_disc_max_logit :77-85 (largest logit over the classes
//   1..K-1) -- these four SELECT one row of the bag -- and get_mean_ben_logit :71-74, which POOLS: the bag's logit row
//   is [0, mean of the bag's class-1 logits, 0, ...].
// fast_rcnn/train_bus.py:241 wires a pair of them (alternating: mass-max for bag label 1, mal-max otherwise), :655
// another (combined: mal-max for both).  ~20 TF slice/concat ops per weak image become one launch: one workgroup per
// bag scans the instances whose bag index matches and returns the row to gather (first extremum, like tf.arg_max /
// tf.arg_min).  A pooling bag rides in the same scan: its key is the constant 0, so the "first extremum" is the bag's
// first row, and every thread adds its rows' class-1 logits in f64; the partials are added by the fixed tree of the
// reduction, so the sum has the same bits on every run.  It is divided by the count in f64 and rounded to f32 once.
#include "common.hip.h"

namespace wssdl {

enum { MIL_SEL_MAL_MAX = 0, MIL_SEL_BEN_MAX = 1, MIL_SEL_MASS_MAX = 2, MIL_SEL_DISC_MAX = 3, MIL_SEL_MEAN_BEN = 4 };

__device__ __forceinline__ int mil_selector(int label, int sel_label1, int sel_other) {
    return (label == 1) ? sel_label1 : sel_other;
}

// one thread's scan of the rows r = t, t + 256, ... of its bag.  MODE 0: the key is sign * logits[r, col] (mal-max,
// ben-max, mass-max); 1: disc-max, the largest logit over the classes 1..K-1; 2: mean-ben, no key (it stays 0, so the
// first row met is kept and the reduction below reports the bag's first row) and the f64 sum of the class-1 logits
template <int MODE>
__device__ __forceinline__ void mil_scan(const float *__restrict__ logits, int R, int K,
                                         const float *__restrict__ bag_of_row, int bag_stride, float bag_offset, int bag,
                                         int col, float sign, float &best, int &bi, int &cnt, double &sum) {
    for (int r = threadIdx.x; r < R; r += 256) {
        if ((int)(bag_of_row[(size_t)r * bag_stride] - bag_offset) != bag) continue;
        ++cnt;
        if (MODE == 2) {
            sum += (double)logits[(size_t)r * K + 1];
            if (bi < 0) bi = r;
            continue;
        }
        float v = sign * logits[(size_t)r * K + col];
        if (MODE == 1)
            for (int k = 2; k < K; ++k) v = fmaxf(v, logits[(size_t)r * K + k]);
        if (bi < 0 || v > best) { best = v; bi = r; }                  // rows ascend: first extremum wins
    }
}

// bag_logits (optional) [n_bags, K]: the logit row the bag's term is taken of -- the selected row's, the pooled row of
// a mean-ben bag, zeros for an empty bag
__global__ __launch_bounds__(256) void mil_select_kernel(
    const float *__restrict__ logits, int R, int K, const float *__restrict__ bag_of_row, int bag_stride,
    float bag_offset, const int *__restrict__ bag_labels, int sel_label1, int sel_other, int *__restrict__ row_out,
    int *__restrict__ count_out, float *__restrict__ bag_logits) {
    __shared__ float s_val[256];
    __shared__ int s_idx[256];
    __shared__ double s_sum[256];
    __shared__ int s_cnt;
    const int bag = blockIdx.x, t = threadIdx.x;
    const int sel = mil_selector(bag_labels[bag], sel_label1, sel_other);
    const bool pool = sel == MIL_SEL_MEAN_BEN;
    const int col = (sel == MIL_SEL_MAL_MAX) ? 2 : ((sel == MIL_SEL_MASS_MAX) ? 0 : 1);
    const float sign = (sel == MIL_SEL_MASS_MAX) ? -1.0f : 1.0f;       // arg-min == arg-max of the negation
    if (t == 0) s_cnt = 0;
    __syncthreads();
    float best = 0.0f;
    double sum = 0.0;
    int bi = -1, cnt = 0;
    if (pool)
        mil_scan<2>(logits, R, K, bag_of_row, bag_stride, bag_offset, bag, col, sign, best, bi, cnt, sum);
    else if (sel == MIL_SEL_DISC_MAX)
        mil_scan<1>(logits, R, K, bag_of_row, bag_stride, bag_offset, bag, col, sign, best, bi, cnt, sum);
    else
        mil_scan<0>(logits, R, K, bag_of_row, bag_stride, bag_offset, bag, col, sign, best, bi, cnt, sum);
    s_val[t] = best;
    s_idx[t] = bi;
    if (pool) s_sum[t] = sum;
    atomicAdd(&s_cnt, cnt);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const int oi = s_idx[t + s];
            const float ov = s_val[t + s];
            const int mi = s_idx[t];
            if (oi >= 0 && (mi < 0 || ov > s_val[t] || (ov == s_val[t] && oi < mi))) {
                s_val[t] = ov;
                s_idx[t] = oi;
            }
            if (pool) s_sum[t] += s_sum[t + s];
        }
        __syncthreads();
    }
    const int row = s_idx[0];
    if (t == 0) {
        row_out[bag] = row;
        if (count_out) count_out[bag] = s_cnt;
    }
    if (bag_logits && t < K) {
        float v = 0.0f;
        if (row >= 0) v = pool ? ((t == 1) ? (float)(s_sum[0] / (double)s_cnt) : 0.0f) : logits[(size_t)row * K + t];
        bag_logits[(size_t)bag * K + t] = v;
    }
}

// ---- the MIL loss as one op ("bag-logit selection + weighted CE") ----
// fast_rcnn/train_bus.py:239-260 / :650-671: per bag the selected instance's logits, softmax CE
// against the bag label, weighted by the class prior [0, WS_MAL_PCT, 1 - WS_MAL_PCT] (:252,:664)
// and the step-dependent scale (:248,:659), mean over the bags.  An empty bag contributes 0 (and
// still counts in the mean).  One workgroup per bag: selection as above, then the bag's term.
constexpr int MIL_MAX_CLASSES = 8;
struct MilWeights { float w[MIL_MAX_CLASSES]; };

__global__ __launch_bounds__(64) void mil_loss_finish_kernel(const float *__restrict__ bag_loss, int n_bags,
                                                            float scale, float *__restrict__ loss) {
    // bags in index order, f64: the same value for any launch shape
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < n_bags; ++b) s += (double)bag_loss[b];
        loss[0] = (float)((double)scale * s / (double)n_bags);
    }
}

// the term of every bag, of its logit row: bag_logits[b] where the selection wrote them (a pooled row is nowhere else),
// else the selected row of the logits block -- the same floats for a selecting bag
__global__ __launch_bounds__(64) void mil_bag_term_kernel(const float *__restrict__ logits, int K,
                                                         const int *__restrict__ bag_labels,
                                                         const int *__restrict__ rows,
                                                         const float *__restrict__ bag_logits, MilWeights cw,
                                                         int n_bags, float *__restrict__ bag_loss) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_bags) return;
    const int r = rows[b], l = bag_labels[b];
    float v = 0.0f;
    if (r >= 0 && l >= 0 && l < K) {
        const float *s = bag_logits ? bag_logits + (size_t)b * K : logits + (size_t)r * K;
        float m;
        const float lz = lse_minus_max(s, K, &m);
        v = cw.w[l] * ((m - s[l]) + lz);
    }
    bag_loss[b] = v;
}

// gradient of the whole [R,K] logits block.  A selecting bag: zeros except its selected row, which gets the
// cross-entropy gradient of that row.  A pooling bag (mean-ben; needs bag_count and bag_logits): every row of the bag
// gets c * d / count in column 1, d the class-1 component of the cross-entropy gradient of the pooled row, and zeros
// elsewhere.  Rows of no bag: zeros.
__global__ __launch_bounds__(256) void mil_loss_backward_kernel(
    const float *__restrict__ logits, int R, int K, const float *__restrict__ bag_of_row, int bag_stride,
    float bag_offset, const int *__restrict__ bag_labels, int sel_label1, int sel_other,
    const int *__restrict__ rows, const int *__restrict__ bag_count, const float *__restrict__ bag_logits,
    MilWeights cw, int n_bags, float scale, const float *__restrict__ grad_loss, float *__restrict__ grad_logits) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float *g = grad_logits + (size_t)r * K;
    const int bag = (int)(bag_of_row[(size_t)r * bag_stride] - bag_offset);
    const bool in_bag = bag >= 0 && bag < n_bags;
    const int l = in_bag ? bag_labels[bag] : -1;
    const bool pooled = in_bag && mil_selector(l, sel_label1, sel_other) == MIL_SEL_MEAN_BEN;
    const bool mine = in_bag && (pooled ? rows[bag] >= 0 : rows[bag] == r);
    if (!mine || l < 0 || l >= K) {
        for (int k = 0; k < K; ++k) g[k] = 0.0f;
        return;
    }
    const float *s = pooled ? bag_logits + (size_t)bag * K : logits + (size_t)r * K;
    float m;
    const float lz = lse_minus_max(s, K, &m);
    const float c = grad_loss[0] * scale * cw.w[l] / (float)n_bags;
    // softmax in the difference form expf((s_k - m) - lz): m + lz formed first would round ulp(|m|) / 2 into the
    // exponent.  The label's component is p_l - 1 = -(sum of the other probabilities): the sum keeps its accuracy
    // when p_l -> 1
    float others = 0.0f, p1 = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float pk = expf((s[k] - m) - lz);
        g[k] = pooled ? 0.0f : c * pk;
        others += (k == l) ? 0.0f : pk;
        if (k == 1) p1 = pk;
    }
    if (pooled)
        g[1] = c * ((l == 1) ? -others : p1) / (float)bag_count[bag];
    else
        g[l] = -c * others;
}

}  // namespace wssdl

// selectors: every one (pooling = true) or the row-selecting ones only
static bool mil_selector_ok(int sel, bool pooling) {
    return sel >= 0 && sel <= (pooling ? wssdl::MIL_SEL_MEAN_BEN : wssdl::MIL_SEL_DISC_MAX);
}

static int mil_weights(const float *class_weights_host, int K, wssdl::MilWeights *out) {
    if (!class_weights_host || K < 3 || K > wssdl::MIL_MAX_CLASSES) return WSSDL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < wssdl::MIL_MAX_CLASSES; ++k) out->w[k] = (k < K) ? class_weights_host[k] : 0.0f;
    return WSSDL_OK;
}

// the one forward behind wssdl_mil_loss_forward (bag_count, bag_logits null) and wssdl_mil_pool_forward: select, bag
// term, finish
static int mil_forward(const float *instance_logits, int R, int K, const float *bag_of_row, int bag_stride,
                       float bag_offset, const int32_t *bag_labels, int n_bags, int sel1, int sel_other,
                       const wssdl::MilWeights &cw, float scale, float *loss, int32_t *row_out, int32_t *bag_count,
                       float *bag_logits, float *bag_loss, wssdl_stream_t stream) {
    hipStream_t st = wssdl::as_stream(stream);
    hipLaunchKernelGGL(wssdl::mil_select_kernel, dim3(n_bags), dim3(256), 0, st, instance_logits, R, K, bag_of_row,
                       bag_stride, bag_offset, bag_labels, sel1, sel_other, row_out, bag_count, bag_logits);
    int rc = wssdl::check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(wssdl::mil_bag_term_kernel, dim3(wssdl::cdiv(n_bags, 64)), dim3(64), 0, st, instance_logits, K,
                       bag_labels, row_out, (const float *)bag_logits, cw, n_bags, bag_loss);
    if ((rc = wssdl::check_launch())) return rc;
    hipLaunchKernelGGL(wssdl::mil_loss_finish_kernel, dim3(1), dim3(64), 0, st, bag_loss, n_bags, scale, loss);
    return wssdl::check_launch();
}

extern "C" int wssdl_mil_select(const float *instance_logits, int R, int num_classes,
                                const float *bag_of_row, int bag_stride, float bag_offset,
                                const int32_t *bag_labels, int n_bags, int selector_label1,
                                int selector_other, int32_t *row_out, int32_t *count_out,
                                wssdl_stream_t stream) {
    if (R < 0 || num_classes < 3 || n_bags < 0 || bag_stride < 1) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!mil_selector_ok(selector_label1, true) || !mil_selector_ok(selector_other, true))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (n_bags == 0) return WSSDL_OK;
    if (!bag_labels || !row_out || (R > 0 && (!instance_logits || !bag_of_row)))
        return WSSDL_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(wssdl::mil_select_kernel, dim3(n_bags), dim3(256), 0, wssdl::as_stream(stream),
                       instance_logits, R, num_classes, bag_of_row, bag_stride, bag_offset, bag_labels,
                       selector_label1, selector_other, row_out, count_out, (float *)nullptr);
    return wssdl::check_launch();
}

extern "C" int wssdl_mil_loss_forward(const float *instance_logits, int R, int num_classes,
                                      const float *bag_of_row, int bag_stride, float bag_offset,
                                      const int32_t *bag_labels, int n_bags, int selector_label1,
                                      int selector_other, const float *class_weights_host, float scale,
                                      float *loss, int32_t *row_out, float *bag_loss, wssdl_stream_t stream) {
    wssdl::MilWeights cw;
    int rc = mil_weights(class_weights_host, num_classes, &cw);
    if (rc) return rc;
    if (n_bags < 1 || !loss || !row_out || !bag_loss) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R < 0 || bag_stride < 1) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!mil_selector_ok(selector_label1, false) || !mil_selector_ok(selector_other, false))
        return WSSDL_ERR_INVALID_ARGUMENT;                              // a pooled row needs wssdl_mil_pool_forward
    if (!bag_labels || (R > 0 && (!instance_logits || !bag_of_row))) return WSSDL_ERR_INVALID_ARGUMENT;
    return mil_forward(instance_logits, R, num_classes, bag_of_row, bag_stride, bag_offset, bag_labels, n_bags,
                       selector_label1, selector_other, cw, scale, loss, row_out, nullptr, nullptr, bag_loss, stream);
}

extern "C" int wssdl_mil_pool_forward(const float *instance_logits, int R, int num_classes,
                                      const float *bag_of_row, int bag_stride, float bag_offset,
                                      const int32_t *bag_labels, int n_bags, int selector_label1,
                                      int selector_other, const float *class_weights_host, float scale,
                                      float *loss, int32_t *row_out, int32_t *bag_count, float *bag_logits,
                                      float *bag_loss, wssdl_stream_t stream) {
    wssdl::MilWeights cw;
    int rc = mil_weights(class_weights_host, num_classes, &cw);
    if (rc) return rc;
    if (R < 0 || n_bags < 1 || bag_stride < 1) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!mil_selector_ok(selector_label1, true) || !mil_selector_ok(selector_other, true))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (!bag_labels || !loss || !row_out || !bag_count || !bag_logits || !bag_loss ||
        (R > 0 && (!instance_logits || !bag_of_row)))
        return WSSDL_ERR_INVALID_ARGUMENT;
    return mil_forward(instance_logits, R, num_classes, bag_of_row, bag_stride, bag_offset, bag_labels, n_bags,
                       selector_label1, selector_other, cw, scale, loss, row_out, bag_count, bag_logits, bag_loss,
                       stream);
}

// the one backward behind both exports; a selecting pair needs neither bag_count nor bag_logits
static int mil_backward(const float *instance_logits, int R, int K, const float *bag_of_row, int bag_stride,
                        float bag_offset, const int32_t *bag_labels, int n_bags, int sel1, int sel_other,
                        const int32_t *rows, const int32_t *bag_count, const float *bag_logits,
                        const wssdl::MilWeights &cw, float scale, const float *grad_loss, float *grad_logits,
                        wssdl_stream_t stream) {
    hipLaunchKernelGGL(wssdl::mil_loss_backward_kernel, dim3(wssdl::cdiv(R, 256)), dim3(256), 0,
                       wssdl::as_stream(stream), instance_logits, R, K, bag_of_row, bag_stride, bag_offset,
                       bag_labels, sel1, sel_other, rows, bag_count, bag_logits, cw, n_bags, scale, grad_loss,
                       grad_logits);
    return wssdl::check_launch();
}

extern "C" int wssdl_mil_loss_backward(const float *instance_logits, int R, int num_classes,
                                       const float *bag_of_row, int bag_stride, float bag_offset,
                                       const int32_t *bag_labels, int n_bags, const int32_t *rows,
                                       const float *class_weights_host, float scale, const float *grad_loss,
                                       float *grad_logits, wssdl_stream_t stream) {
    wssdl::MilWeights cw;
    int rc = mil_weights(class_weights_host, num_classes, &cw);
    if (rc) return rc;
    if (R < 0 || n_bags < 1 || bag_stride < 1) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R == 0) return WSSDL_OK;
    if (!instance_logits || !bag_of_row || !bag_labels || !rows || !grad_loss || !grad_logits)
        return WSSDL_ERR_INVALID_ARGUMENT;
    // whatever selecting pair made `rows`: the gradient goes to the rows it names
    return mil_backward(instance_logits, R, num_classes, bag_of_row, bag_stride, bag_offset, bag_labels, n_bags,
                        wssdl::MIL_SEL_MAL_MAX, wssdl::MIL_SEL_MAL_MAX, rows, nullptr, nullptr, cw, scale, grad_loss,
                        grad_logits, stream);
}

extern "C" int wssdl_mil_pool_backward(const float *instance_logits, int R, int num_classes,
                                       const float *bag_of_row, int bag_stride, float bag_offset,
                                       const int32_t *bag_labels, int n_bags, int selector_label1,
                                       int selector_other, const int32_t *rows, const int32_t *bag_count,
                                       const float *bag_logits, const float *class_weights_host, float scale,
                                       const float *grad_loss, float *grad_logits, wssdl_stream_t stream) {
    wssdl::MilWeights cw;
    int rc = mil_weights(class_weights_host, num_classes, &cw);
    if (rc) return rc;
    if (R < 0 || n_bags < 1 || bag_stride < 1) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!mil_selector_ok(selector_label1, true) || !mil_selector_ok(selector_other, true))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (!bag_labels || !rows || !bag_count || !bag_logits || !grad_loss ||
        (R > 0 && (!instance_logits || !bag_of_row || !grad_logits)))
        return WSSDL_ERR_INVALID_ARGUMENT;
    if (R == 0) return WSSDL_OK;
    return mil_backward(instance_logits, R, num_classes, bag_of_row, bag_stride, bag_offset, bag_labels, n_bags,
                        selector_label1, selector_other, rows, bag_count, bag_logits, cw, scale, grad_loss,
                        grad_logits, stream);
}
