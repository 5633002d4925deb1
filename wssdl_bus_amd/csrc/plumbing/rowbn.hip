// Training-mode batch norm over the rows of an [M, C] f32 matrix, fused with ReLU, for the
// per-RoI ResNet head (networks/roi_head.py).  NOT part of the drop-in C ABI of the detection
// hot path (include/wssdl_bus_hip.h): this is plumbing around it, in its own library
// (libwssdl_plumbing_hip.so).  The head's activations are [R*h*w, C] with R*h*w up to ~4e5
// rows: with stock elementwise ops a BN+ReLU layer costs ~19 passes over the tensor per
// training step (forward 5, backward 14); here
//   forward : column sums (1 read)            -> y = relu(x*scale + shift)        (1 read, 1 write)
//   backward: column sums of g and g*x, g = dy masked by the recomputed activation (2 reads)
//                                              -> dx = a*g - k0 - k1*x             (2 reads, 1 write)
// Column sums are accumulated in f64 per thread, reduced in a fixed order (partials per
// workgroup, then one thread per column): results do not depend on scheduling.
//
// LIVE-ROW MASK (the *_masked entry points).  The rows come in groups of `per` (the h*w positions of
// one RoI); `mask[roi]` = 0 marks a dead RoI -- a padding row of the fixed-shape RoI blob, or of a
// supervised image that ran short of candidates.  Dead rows are skipped by the column sums (not even
// loaded), the statistics are taken over the live rows (n = per * sum(mask), computed on the device:
// no host read-back), and the layer writes zeros for dead rows in both directions, so the live rows
// come out exactly as if the blob had been compacted first.
// The *_masked_pm entry points take the same mask on POSITION-MAJOR rows (row r belongs to RoI
// r % n_rois: the head's 4x4 section, networks/roi_head.py); statistics and outputs are the same.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLUMB_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_PARTIAL_BLOCKS = 1024;

typedef float float4v __attribute__((ext_vector_type(4)));

// RoI of row r under the live-row mask: MASK 1 = roi-major rows (r / div, div = per),
// MASK 2 = position-major rows (r % div, div = n_rois).  (M < 2^31 is checked by the entry points.)
template <int MASK>
__device__ __forceinline__ unsigned mask_roi(long long r, int div) {
    return MASK == 2 ? (unsigned)r % (unsigned)div : (unsigned)r / (unsigned)div;
}

// ---- arithmetic shared by every kernel of this file (the join kernels below must round as these do) ----
// The fused multiply-adds are written out: left to the compiler's contraction, the same expression came out
// fused in one kernel and as separate multiplies and subtractions in another (even lane by lane within one
// kernel), and a join must round exactly as the layers it replaces.
// y = x*scale + shift
__device__ __forceinline__ float bn_affine(float x, float sc, float sh) { return __builtin_fmaf(x, sc, sh); }
// dx = a*u - k0 - k1*x (coefficients of rowbn_bwd_finish_kernel)
__device__ __forceinline__ float bn_dx(float ka, float u, float k0, float k1, float x) {
    return __builtin_fmaf(-k1, x, __builtin_fmaf(ka, u, -k0));
}
// the f64 column sums of a thread: two rows per step, then a one-row tail
__device__ __forceinline__ void acc_rows2(double &s, double &q, float v0, float w0, float v1, float w1) {
    s += (double)v0 + (double)v1;
    q += (double)v0 * (double)w0 + (double)v1 * (double)w1;
}
__device__ __forceinline__ void acc_row(double &s, double &q, float v, float w) {
    s += (double)v;
    q += (double)v * (double)w;
}

// Thread t of a slab kernel owns float4 column (t % L) + cc * L and the rows r0 + t / L + k * RS;
// L = min(C/4, 256), RS = 256 / L.
struct Slab {
    int C4, L, RS, lc, lr;
    long long r0, r1;
    __device__ __forceinline__ Slab(long long M, int C, long long rows_per_block) {
        C4 = C >> 2;
        L = C4 < BLOCK ? C4 : BLOCK;
        RS = BLOCK / L;
        lc = threadIdx.x % L;
        lr = threadIdx.x / L;
        r0 = (long long)blockIdx.x * rows_per_block;
        r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
    }
};

// fixed-order reduction over the RS row phases of float4 column c4: out[0..C) = s, out[C..2C) = q
__device__ __forceinline__ void slab_reduce(const Slab &b, int C, int c4, const double (&s)[4], const double (&q)[4],
                                            double (*red)[8], double *__restrict__ out) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[t][j] = s[j]; red[t][4 + j] = q[j]; }
    __syncthreads();
    if (b.lr == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double ss = 0.0, qq = 0.0;
            for (int k = 0; k < b.RS; ++k) { ss += red[k * b.L + b.lc][j]; qq += red[k * b.L + b.lc][4 + j]; }
            out[c4 * 4 + j] = ss;
            out[C + c4 * 4 + j] = qq;
        }
    }
}

// ---- block 1's entry gradient (networks/roi_head.py, _EntryNormFn) ----
// Block 1's pre-activation output y (roi-major rows, `per` positions per RoI) feeds conv1 at every position and
// the projection shortcut at the positions it samples.  Its gradient at row r = roi * per + p is
//   dy[r] + (possel[p] >= 0 ? dys[possel[p] * R + roi] + 0 : 0)
// with dy conv1's gradient, dys the shortcut's position-major gradient and possel[p] the shortcut's slot of
// position p (-1: not sampled).  The ENTRY variants of the two backward kernels form it in registers.  The
// "+ 0" is kept: the separate ops scatter dys into a zero tensor first, which turns a -0 into +0.
struct EntryGrad {
    const float *dys;       // [n_slots * R, C]
    const int *possel;      // [per]
    int per, R;
};

template <bool ENTRY>
__device__ __forceinline__ float4v load_dy(const float *__restrict__ dy, const EntryGrad &e, long long r, int C, int c4) {
    const float4v g = reinterpret_cast<const float4v *>(dy + (size_t)r * C)[c4];
    if (!ENTRY) return g;
    const unsigned roi = (unsigned)r / (unsigned)e.per, p = (unsigned)r - roi * (unsigned)e.per;
    const int slot = e.possel[p];
    const float4v zero4 = {0, 0, 0, 0};
    float4v d = zero4;
    if (slot >= 0) d = reinterpret_cast<const float4v *>(e.dys + ((size_t)slot * e.R + roi) * C)[c4] + zero4;
    return g + d;
}

// Partial column sums of one row slab (thread mapping: Slab).
// MODE 0: s = sum x,  q = sum x*x
// MODE 1: s = sum g,  q = sum g*x   with g = dy, masked by (x*scale + shift > 0) when RELU
// ENTRY: dy is block 1's entry gradient (EntryGrad; MODE 1, roi-major rows, M < 2^31)
template <int MODE, bool RELU, int MASK, bool ENTRY = false>
__global__ __launch_bounds__(BLOCK) void rowbn_partial_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ scale,
    const float *__restrict__ shift, long long M, int C, long long rows_per_block,
    double *__restrict__ partial, const float *__restrict__ mask, int per, EntryGrad eg = EntryGrad()) {
    __shared__ double red[BLOCK][8];
    const Slab b(M, C, rows_per_block);
    const int C4 = b.C4, L = b.L, RS = b.RS, lc = b.lc, lr = b.lr;
    const long long r0 = b.r0, r1 = b.r1;
    double *out = partial + (size_t)blockIdx.x * 2 * C;
    for (int cc = 0; cc * L < C4; ++cc) {
        const int c4 = cc * L + lc;
        double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        float4v sc = {0, 0, 0, 0}, sh = {0, 0, 0, 0};
        if (MODE == 1 && RELU) {
            sc = reinterpret_cast<const float4v *>(scale)[c4];
            sh = reinterpret_cast<const float4v *>(shift)[c4];
        }
        if (lr < RS) {
            long long r = r0 + lr;
            // two rows in flight per step
            for (; r + RS < r1; r += 2 * RS) {
                bool live0 = true, live1 = true;
                if (MASK) {
                    live0 = mask[mask_roi<MASK>(r, per)] != 0.0f;
                    live1 = mask[mask_roi<MASK>(r + RS, per)] != 0.0f;
                    if (!live0 && !live1) continue;
                }
                const float4v zero4 = {0, 0, 0, 0};
                const float4v a0 = live0 ? reinterpret_cast<const float4v *>(x + (size_t)r * C)[c4] : zero4;
                const float4v a1 = live1 ? reinterpret_cast<const float4v *>(x + (size_t)(r + RS) * C)[c4] : zero4;
                float4v g0, g1;
                if (MODE == 1) {
                    g0 = live0 ? load_dy<ENTRY>(dy, eg, r, C, c4) : zero4;
                    g1 = live1 ? load_dy<ENTRY>(dy, eg, r + RS, C, c4) : zero4;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (MODE == 0) {
                        acc_rows2(s[j], q[j], a0[j], a0[j], a1[j], a1[j]);
                    } else {
                        float u0 = g0[j], u1 = g1[j];
                        if (RELU) {
                            if (!(bn_affine(a0[j], sc[j], sh[j]) > 0.0f)) u0 = 0.0f;
                            if (!(bn_affine(a1[j], sc[j], sh[j]) > 0.0f)) u1 = 0.0f;
                        }
                        if (MASK) {                 // a dead row adds nothing (x = 0 would still pass the ReLU test)
                            if (!live0) u0 = 0.0f;
                            if (!live1) u1 = 0.0f;
                        }
                        acc_rows2(s[j], q[j], u0, a0[j], u1, a1[j]);
                    }
                }
            }
            for (; r < r1; r += RS) {
                if (MASK && mask[mask_roi<MASK>(r, per)] == 0.0f) continue;
                const float4v a0 = reinterpret_cast<const float4v *>(x + (size_t)r * C)[c4];
                float4v g0;
                if (MODE == 1) g0 = load_dy<ENTRY>(dy, eg, r, C, c4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (MODE == 0) {
                        acc_row(s[j], q[j], a0[j], a0[j]);
                    } else {
                        float u0 = g0[j];
                        if (RELU && !(bn_affine(a0[j], sc[j], sh[j]) > 0.0f)) u0 = 0.0f;
                        acc_row(s[j], q[j], u0, a0[j]);
                    }
                }
            }
        }
        slab_reduce(b, C, c4, s, q, red, out);
    }
}

// Sum of the per-workgroup partials of 16 columns, in a fixed order: 64 row groups of 16 lanes
// each add every 64th partial (in order), then lane-wise the 64 group sums are added in order.
constexpr int FIN_COLS = 16, FIN_GROUPS = 64;

__device__ __forceinline__ void finish_reduce(const double *__restrict__ partial, int nblocks, int C,
                                              int c, int grp, double (*red)[FIN_COLS][2], double &s,
                                              double &q) {
    double ss = 0.0, qq = 0.0;
    if (c < C)
        for (int b = grp; b < nblocks; b += FIN_GROUPS) {
            ss += partial[(size_t)b * 2 * C + c];
            qq += partial[(size_t)b * 2 * C + C + c];
        }
    red[grp][threadIdx.x % FIN_COLS][0] = ss;
    red[grp][threadIdx.x % FIN_COLS][1] = qq;
    __syncthreads();
    s = 0.0;
    q = 0.0;
    if (grp == 0)
        for (int g = 0; g < FIN_GROUPS; ++g) {
            s += red[g][threadIdx.x][0];
            q += red[g][threadIdx.x][1];
        }
}

// rows the statistics are taken over: M, or per * (number of live RoIs) with a mask (at least 1).
// Every thread of the workgroup returns the same value; the sum runs in a fixed order.
__device__ __forceinline__ double live_rows(const float *__restrict__ mask, int n_rois, int per, long long M,
                                            double *scratch /* [FIN_COLS * FIN_GROUPS] LDS */) {
    if (!mask) return (double)M;
    double c = 0.0;
    for (int i = threadIdx.x; i < n_rois; i += FIN_COLS * FIN_GROUPS) c += mask[i] != 0.0f ? 1.0 : 0.0;
    __syncthreads();
    scratch[threadIdx.x] = c;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < FIN_COLS * FIN_GROUPS; ++i) t += scratch[i];
    __syncthreads();
    t *= (double)per;
    return t < 1.0 ? 1.0 : t;
}

// The layer's running statistics (nn.BatchNorm's buffers), updated by the forward finish kernel from the batch
// statistics it has just written; any pointer may be null (that buffer is left alone).
//   running_mean += momentum * (mean - running_mean)
//   running_var  += momentum * (var * n / max(n - 1, 1) - running_var)      n = the rows the statistics cover
// evaluated in f64 from the f32 mean / var and rounded to f32 once; num_batches_tracked (int64 [1]) += 1.
struct Running {
    float *mean, *var;
    float momentum;
    long long *batches;
};

// r + mom * (stat * unbias - r), every f64 operation rounded on its own (no contraction: the host restates it)
__device__ __forceinline__ float running_update(float r, float stat, double unbias, double mom) {
#pragma clang fp contract(off)
    const double t = (double)stat * unbias;
    const double d = t - (double)r;
    const double p = mom * d;
    return (float)((double)r + p);
}

// forward finish: mean / biased var / scale / shift per column, and the running statistics
__global__ __launch_bounds__(FIN_COLS * FIN_GROUPS) void rowbn_fwd_finish_kernel(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ bias, float eps,
    float *__restrict__ mean, float *__restrict__ var, float *__restrict__ rstd,
    float *__restrict__ scale, float *__restrict__ shift, const float *__restrict__ mask, int n_rois, int per,
    float *__restrict__ count, Running run) {
    __shared__ double red[FIN_GROUPS][FIN_COLS][2];
    const int grp = threadIdx.x / FIN_COLS;
    const int c = blockIdx.x * FIN_COLS + threadIdx.x % FIN_COLS;
    const double Mn = live_rows(mask, n_rois, per, M, &red[0][0][0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (count) count[0] = (float)Mn;
        if (run.batches) run.batches[0] = run.batches[0] + 1;
    }
    double s, q;
    finish_reduce(partial, nblocks, C, c, grp, red, s, q);
    if (grp != 0 || c >= C) return;
    const double mu = s / Mn;
    double v = q / Mn - mu * mu;
    if (v < 0.0) v = 0.0;
    const float rs = (float)(1.0 / sqrt(v + (double)eps));
    const float scl = rs * weight[c];
    mean[c] = (float)mu;
    var[c] = (float)v;
    rstd[c] = rs;
    scale[c] = scl;
    shift[c] = bias[c] - (float)mu * scl;
    const double mom = (double)run.momentum;
    if (run.mean) run.mean[c] = running_update(run.mean[c], (float)mu, 1.0, mom);
    if (run.var) run.var[c] = running_update(run.var[c], (float)v, Mn / (Mn - 1.0 > 1.0 ? Mn - 1.0 : 1.0), mom);
}

// backward finish: dweight, dbias and the three coefficients of dx = a*g - k0 - k1*x
__global__ __launch_bounds__(FIN_COLS * FIN_GROUPS) void rowbn_bwd_finish_kernel(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ mean,
    const float *__restrict__ rstd, float *__restrict__ dweight, float *__restrict__ dbias,
    float *__restrict__ coef, const float *__restrict__ mask, int n_rois, int per) {
    __shared__ double red[FIN_GROUPS][FIN_COLS][2];
    const int grp = threadIdx.x / FIN_COLS;
    const int c = blockIdx.x * FIN_COLS + threadIdx.x % FIN_COLS;
    const double Mn = live_rows(mask, n_rois, per, M, &red[0][0][0]);
    double sg, sgx;
    finish_reduce(partial, nblocks, C, c, grp, red, sg, sgx);
    if (grp != 0 || c >= C) return;
    const double mu = mean[c], rs = rstd[c], w = weight[c];
    const double sum_g_xhat = (sgx - mu * sg) * rs;
    const double a = w * rs;
    const double k1 = a * rs * sum_g_xhat / Mn;
    const double k0 = a * sg / Mn - k1 * mu;
    dweight[c] = (float)sum_g_xhat;
    dbias[c] = (float)sg;
    coef[c] = (float)a;
    coef[C + c] = (float)k0;
    coef[2 * C + c] = (float)k1;
}

template <bool RELU, int MASK>
__global__ __launch_bounds__(BLOCK) void rowbn_apply_fwd_kernel(
    const float *__restrict__ x, const float *__restrict__ scale, const float *__restrict__ shift,
    long long total4, int C4, float *__restrict__ y, const float *__restrict__ mask, int per) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total4;
         i += (long long)gridDim.x * BLOCK) {
        const int c4 = (int)(i % C4);
        if (MASK && mask[mask_roi<MASK>(i / C4, per)] == 0.0f) {
            const float4v zero4 = {0, 0, 0, 0};
            reinterpret_cast<float4v *>(y)[i] = zero4;
            continue;
        }
        const float4v a = reinterpret_cast<const float4v *>(x)[i];
        const float4v sc = reinterpret_cast<const float4v *>(scale)[c4];
        const float4v sh = reinterpret_cast<const float4v *>(shift)[c4];
        float4v o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = bn_affine(a[j], sc[j], sh[j]);
            if (RELU) v = v > 0.0f ? v : 0.0f;
            o[j] = v;
        }
        reinterpret_cast<float4v *>(y)[i] = o;
    }
}

template <bool RELU, int MASK, bool ENTRY = false>
__global__ __launch_bounds__(BLOCK) void rowbn_apply_bwd_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ scale,
    const float *__restrict__ shift, const float *__restrict__ coef, long long total4, int C4,
    float *__restrict__ dx, const float *__restrict__ mask, int per, EntryGrad eg = EntryGrad()) {
    const int C = C4 * 4;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total4;
         i += (long long)gridDim.x * BLOCK) {
        const int c4 = (int)(i % C4);
        if (MASK && mask[mask_roi<MASK>(i / C4, per)] == 0.0f) {
            const float4v zero4 = {0, 0, 0, 0};
            reinterpret_cast<float4v *>(dx)[i] = zero4;
            continue;
        }
        const float4v a = reinterpret_cast<const float4v *>(x)[i];
        const float4v g = ENTRY ? load_dy<true>(dy, eg, i / C4, C, c4) : reinterpret_cast<const float4v *>(dy)[i];
        const float4v ka = reinterpret_cast<const float4v *>(coef)[c4];
        const float4v k0 = reinterpret_cast<const float4v *>(coef + C)[c4];
        const float4v k1 = reinterpret_cast<const float4v *>(coef + 2 * C)[c4];
        float4v sc = {0, 0, 0, 0}, sh = {0, 0, 0, 0};
        if (RELU) {
            sc = reinterpret_cast<const float4v *>(scale)[c4];
            sh = reinterpret_cast<const float4v *>(shift)[c4];
        }
        float4v o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float u = g[j];
            if (RELU && !(bn_affine(a[j], sc[j], sh[j]) > 0.0f)) u = 0.0f;
            o[j] = bn_dx(ka[j], u, k0[j], k1[j], a[j]);
        }
        reinterpret_cast<float4v *>(dx)[i] = o;
    }
}

// ---- residual joins of the head's position-major section (networks/roi_head.py, _JoinFn) ----
// A join is the end of a block: out = bn3(x3) + other, where other is the identity shortcut (a plain
// tensor) or, with DUAL, the projection shortcut's own batch norm of xs; the next block's pre-activation
// norm (or the head's final norm) then takes its statistics over out.  Both join kernels walk row slabs
// exactly as rowbn_partial_kernel does (Slab, acc_rows2 / acc_row, slab_reduce), so the f64 partials
// they leave are those that kernel would compute from the tensor they write.
// MASK is 0 or 2 (the joins are position-major).

template <int MASK>
__device__ __forceinline__ bool row_live(const float *__restrict__ mask, long long r, int div) {
    return MASK ? mask[mask_roi<MASK>(r, div)] != 0.0f : true;
}

__device__ __forceinline__ float4v load4(const float *__restrict__ p, long long r, int C, int c4, bool on) {
    const float4v zero4 = {0, 0, 0, 0};
    return on ? reinterpret_cast<const float4v *>(p + (size_t)r * C)[c4] : zero4;
}

// Forward join: writes out = act_mask(x3*sc3 + sh3) + (DUAL ? act_mask(other*sco + sho) : other), act_mask
// being zero on dead rows, and the partials (sum, sum of squares over the live rows) of out.
template <bool DUAL, int MASK>
__global__ __launch_bounds__(BLOCK) void rowbn_join_fwd_kernel(
    const float *__restrict__ x3, const float *__restrict__ sc3, const float *__restrict__ sh3,
    const float *__restrict__ other, const float *__restrict__ sco, const float *__restrict__ sho, long long M,
    int C, long long rows_per_block, float *__restrict__ out, double *__restrict__ partial,
    const float *__restrict__ mask, int div) {
    __shared__ double red[BLOCK][8];
    const Slab b(M, C, rows_per_block);
    double *pout = partial + (size_t)blockIdx.x * 2 * C;
    for (int cc = 0; cc * b.L < b.C4; ++cc) {
        const int c4 = cc * b.L + b.lc;
        double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        const float4v k3 = reinterpret_cast<const float4v *>(sc3)[c4], h3 = reinterpret_cast<const float4v *>(sh3)[c4];
        float4v ko = {0, 0, 0, 0}, ho = {0, 0, 0, 0};
        if (DUAL) {
            ko = reinterpret_cast<const float4v *>(sco)[c4];
            ho = reinterpret_cast<const float4v *>(sho)[c4];
        }
        // one element of out; a dead row is zero from the norm(s), plus the identity
        auto join = [&](float a, float o, int j, bool live) {
            const float t = live ? bn_affine(a, k3[j], h3[j]) : 0.0f;
            const float u = DUAL ? (live ? bn_affine(o, ko[j], ho[j]) : 0.0f) : o;
            return t + u;
        };
        if (b.lr < b.RS) {
            const int RS = b.RS;
            long long r = b.r0 + b.lr;
#pragma unroll 1
            for (; r + RS < b.r1; r += 2 * RS) {
                const bool live0 = row_live<MASK>(mask, r, div), live1 = row_live<MASK>(mask, r + RS, div);
                const float4v a0 = load4(x3, r, C, c4, live0), a1 = load4(x3, r + RS, C, c4, live1);
                const float4v o0 = load4(other, r, C, c4, !DUAL || live0), o1 = load4(other, r + RS, C, c4, !DUAL || live1);
                float4v y0, y1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y0[j] = join(a0[j], o0[j], j, live0);
                    y1[j] = join(a1[j], o1[j], j, live1);
                    const float v0 = live0 ? y0[j] : 0.0f, v1 = live1 ? y1[j] : 0.0f;
                    acc_rows2(s[j], q[j], v0, v0, v1, v1);
                }
                reinterpret_cast<float4v *>(out + (size_t)r * C)[c4] = y0;
                reinterpret_cast<float4v *>(out + (size_t)(r + RS) * C)[c4] = y1;
            }
            for (; r < b.r1; r += RS) {
                const bool live0 = row_live<MASK>(mask, r, div);
                const float4v a0 = load4(x3, r, C, c4, live0), o0 = load4(other, r, C, c4, !DUAL || live0);
                float4v y0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y0[j] = join(a0[j], o0[j], j, live0);
                    if (live0) acc_row(s[j], q[j], y0[j], y0[j]);
                }
                reinterpret_cast<float4v *>(out + (size_t)r * C)[c4] = y0;
            }
        }
        slab_reduce(b, C, c4, s, q, red, pout);
    }
}

// Backward join: writes g = (a*u - k0 - k1*xo) + d_res -- the dx of the norm that follows the join (its
// coefficients in coef, u = dy masked by the recomputed ReLU of xo*scn + shn; zero on dead rows) plus, with
// RES, the gradient arriving over the residual path -- and the partials bn3's backward takes over it:
// partial3 = (sum g, sum g*x3) and, with DUAL, partials = (sum g, sum g*xs), live rows only.
template <bool DUAL, bool RES, int MASK>
__global__ __launch_bounds__(BLOCK) void rowbn_join_bwd_kernel(
    const float *__restrict__ xo, const float *__restrict__ dy, const float *__restrict__ scn,
    const float *__restrict__ shn, const float *__restrict__ coef, const float *__restrict__ dres,
    const float *__restrict__ x3, const float *__restrict__ xs, long long M, int C, long long rows_per_block,
    float *__restrict__ g, double *__restrict__ partial3, double *__restrict__ partials,
    const float *__restrict__ mask, int div) {
    __shared__ double red[BLOCK][8];
    const Slab b(M, C, rows_per_block);
    double *p3 = partial3 + (size_t)blockIdx.x * 2 * C;
    double *ps = DUAL ? partials + (size_t)blockIdx.x * 2 * C : nullptr;
    for (int cc = 0; cc * b.L < b.C4; ++cc) {
        const int c4 = cc * b.L + b.lc;
        double s[4] = {0, 0, 0, 0}, q3[4] = {0, 0, 0, 0}, qs[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
        const float4v sc = reinterpret_cast<const float4v *>(scn)[c4], sh = reinterpret_cast<const float4v *>(shn)[c4];
        const float4v ka = reinterpret_cast<const float4v *>(coef)[c4];
        const float4v k0 = reinterpret_cast<const float4v *>(coef + C)[c4];
        const float4v k1 = reinterpret_cast<const float4v *>(coef + 2 * C)[c4];
        auto grad = [&](float x, float d, float res, int j, bool live) {
            float u = d;
            if (!(bn_affine(x, sc[j], sh[j]) > 0.0f)) u = 0.0f;
            const float dx = live ? bn_dx(ka[j], u, k0[j], k1[j], x) : 0.0f;
            return RES ? dx + res : dx;
        };
        if (b.lr < b.RS) {
            const int RS = b.RS;
            long long r = b.r0 + b.lr;
#pragma unroll 1
            for (; r + RS < b.r1; r += 2 * RS) {
                const bool live0 = row_live<MASK>(mask, r, div), live1 = row_live<MASK>(mask, r + RS, div);
                const float4v x0 = load4(xo, r, C, c4, live0), x1 = load4(xo, r + RS, C, c4, live1);
                const float4v d0 = load4(dy, r, C, c4, live0), d1 = load4(dy, r + RS, C, c4, live1);
                const float4v e0 = load4(dres, r, C, c4, RES), e1 = load4(dres, r + RS, C, c4, RES);
                const float4v a0 = load4(x3, r, C, c4, live0), a1 = load4(x3, r + RS, C, c4, live1);
                const float4v b0 = load4(xs, r, C, c4, DUAL && live0), b1 = load4(xs, r + RS, C, c4, DUAL && live1);
                float4v g0, g1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    g0[j] = grad(x0[j], d0[j], e0[j], j, live0);
                    g1[j] = grad(x1[j], d1[j], e1[j], j, live1);
                    const float v0 = live0 ? g0[j] : 0.0f, v1 = live1 ? g1[j] : 0.0f;
                    acc_rows2(s[j], q3[j], v0, a0[j], v1, a1[j]);
                    if (DUAL) acc_rows2(s2[j], qs[j], v0, b0[j], v1, b1[j]);
                }
                reinterpret_cast<float4v *>(g + (size_t)r * C)[c4] = g0;
                reinterpret_cast<float4v *>(g + (size_t)(r + RS) * C)[c4] = g1;
            }
            for (; r < b.r1; r += RS) {
                const bool live0 = row_live<MASK>(mask, r, div);
                const float4v x0 = load4(xo, r, C, c4, live0), d0 = load4(dy, r, C, c4, live0);
                const float4v e0 = load4(dres, r, C, c4, RES), a0 = load4(x3, r, C, c4, live0);
                const float4v b0 = load4(xs, r, C, c4, DUAL && live0);
                float4v g0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    g0[j] = grad(x0[j], d0[j], e0[j], j, live0);
                    if (live0) {
                        acc_row(s[j], q3[j], g0[j], a0[j]);
                        if (DUAL) acc_row(s2[j], qs[j], g0[j], b0[j]);
                    }
                }
                reinterpret_cast<float4v *>(g + (size_t)r * C)[c4] = g0;
            }
        }
        slab_reduce(b, C, c4, s, q3, red, p3);
        if (DUAL) slab_reduce(b, C, c4, s, qs, red, ps);
    }
}

// Block 1's two backward applies in one pass over g: dx3 and dxs from their own coefficient sets (neither
// norm has a ReLU).
template <int MASK>
__global__ __launch_bounds__(BLOCK) void rowbn_apply_bwd_dual_kernel(
    const float *__restrict__ x3, const float *__restrict__ xs, const float *__restrict__ g,
    const float *__restrict__ coef3, const float *__restrict__ coefs, long long total4, int C4,
    float *__restrict__ dx3, float *__restrict__ dxs, const float *__restrict__ mask, int div) {
    const int C = C4 * 4;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total4;
         i += (long long)gridDim.x * BLOCK) {
        const int c4 = (int)(i % C4);
        if (MASK && mask[mask_roi<MASK>(i / C4, div)] == 0.0f) {
            const float4v zero4 = {0, 0, 0, 0};
            reinterpret_cast<float4v *>(dx3)[i] = zero4;
            reinterpret_cast<float4v *>(dxs)[i] = zero4;
            continue;
        }
        const float4v a = reinterpret_cast<const float4v *>(x3)[i];
        const float4v e = reinterpret_cast<const float4v *>(xs)[i];
        const float4v u = reinterpret_cast<const float4v *>(g)[i];
        const float4v ka3 = reinterpret_cast<const float4v *>(coef3)[c4], kas = reinterpret_cast<const float4v *>(coefs)[c4];
        const float4v k03 = reinterpret_cast<const float4v *>(coef3 + C)[c4], k0s = reinterpret_cast<const float4v *>(coefs + C)[c4];
        const float4v k13 = reinterpret_cast<const float4v *>(coef3 + 2 * C)[c4], k1s = reinterpret_cast<const float4v *>(coefs + 2 * C)[c4];
        float4v o3, os;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o3[j] = bn_dx(ka3[j], u[j], k03[j], k13[j], a[j]);
            os[j] = bn_dx(kas[j], u[j], k0s[j], k1s[j], e[j]);
        }
        reinterpret_cast<float4v *>(dx3)[i] = o3;
        reinterpret_cast<float4v *>(dxs)[i] = os;
    }
}

inline int partial_blocks(long long M, int C) {
    const int C4 = C / 4;
    const int L = C4 < BLOCK ? C4 : BLOCK;
    const int RS = BLOCK / L;
    long long want = (M + (long long)RS * 16 - 1) / ((long long)RS * 16);   // >= 16 row steps each
    if (want < 1) want = 1;
    return (int)(want < MAX_PARTIAL_BLOCKS ? want : MAX_PARTIAL_BLOCKS);
}

inline bool shape_ok(long long M, int C) {
    if (M < 1 || C < 4 || (C & 3)) return false;
    const int C4 = C / 4;
    return C4 <= BLOCK ? (BLOCK % C4 == 0) : (C4 % BLOCK == 0);
}

inline int apply_grid(long long total4) {
    long long b = (total4 + BLOCK - 1) / BLOCK;
    return (int)(b < 65536 ? b : 65536);
}

}  // namespace

// bytes of scratch for the partial sums (f64) of one call
PLUMB_API size_t wsplumb_rowbn_workspace_bytes(long long M, int C) {
    if (!shape_ok(M, C)) return 0;
    return (size_t)partial_blocks(M, C) * 2 * (size_t)C * sizeof(double);
}

// 1 when the kernels support the shape (C % 4 == 0 and C/4 divides or is a multiple of 256)
PLUMB_API int wsplumb_rowbn_supported(long long M, int C) { return shape_ok(M, C) ? 1 : 0; }

static int forward_impl(const float *x, long long M, int C, const float *weight, const float *bias, float eps,
                        int relu, float *y, float *mean, float *var, float *rstd, float *scale, float *shift,
                        const float *mask, int n_rois, int per, float *count, void *workspace,
                        size_t workspace_bytes, void *stream, Running run, bool pm = false) {
    if (!shape_ok(M, C) || workspace_bytes < wsplumb_rowbn_workspace_bytes(M, C)) return 1;
    if (mask && (per < 1 || n_rois < 1 || (long long)n_rois * per != M || M > 0x7fffffffLL)) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = partial_blocks(M, C);
    const long long rpb = (M + nb - 1) / nb;
    double *partial = static_cast<double *>(workspace);
    const int div = pm ? n_rois : per;          // row -> RoI divisor of the mask modes (mask_roi)
    if (mask && pm)
        hipLaunchKernelGGL((rowbn_partial_kernel<0, false, 2>), dim3(nb), dim3(BLOCK), 0, st, x, nullptr,
                           nullptr, nullptr, M, C, rpb, partial, mask, div);
    else if (mask)
        hipLaunchKernelGGL((rowbn_partial_kernel<0, false, 1>), dim3(nb), dim3(BLOCK), 0, st, x, nullptr,
                           nullptr, nullptr, M, C, rpb, partial, mask, per);
    else
        hipLaunchKernelGGL((rowbn_partial_kernel<0, false, 0>), dim3(nb), dim3(BLOCK), 0, st, x, nullptr,
                           nullptr, nullptr, M, C, rpb, partial, nullptr, 1);
    hipLaunchKernelGGL(rowbn_fwd_finish_kernel, dim3((C + FIN_COLS - 1) / FIN_COLS), dim3(FIN_COLS * FIN_GROUPS), 0, st, partial, nb, C,
                       M, weight, bias, eps, mean, var, rstd, scale, shift, mask, n_rois, per, count, run);
    const long long total4 = M * (C / 4);
#define WSPLUMB_APPLY(RELU, MASK) \
    hipLaunchKernelGGL((rowbn_apply_fwd_kernel<RELU, MASK>), dim3(apply_grid(total4)), dim3(BLOCK), 0, st, x, scale, \
                       shift, total4, C / 4, y, mask, div)
    const int mode = mask ? (pm ? 2 : 1) : 0;
    if (relu) { if (mode == 2) WSPLUMB_APPLY(true, 2); else if (mode) WSPLUMB_APPLY(true, 1); else WSPLUMB_APPLY(true, 0); }
    else { if (mode == 2) WSPLUMB_APPLY(false, 2); else if (mode) WSPLUMB_APPLY(false, 1); else WSPLUMB_APPLY(false, 0); }
#undef WSPLUMB_APPLY
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// y = act(batch_norm(x)); writes mean, var (biased), rstd, scale = rstd*weight,
// shift = bias - mean*scale (all [C]).  Returns 0 on success.
// running_mean / running_var (f32 [C]) and num_batches_tracked (int64 [1]) are the layer's buffers, updated
// in place with `momentum` (struct Running); each may be null.  The same four close every forward entry point.
PLUMB_API int wsplumb_rowbn_forward(const float *x, long long M, int C, const float *weight,
                                    const float *bias, float eps, int relu, float *y, float *mean,
                                    float *var, float *rstd, float *scale, float *shift,
                                    void *workspace, size_t workspace_bytes, void *stream,
                                    float *running_mean, float *running_var, float momentum,
                                    long long *num_batches_tracked) {
    return forward_impl(x, M, C, weight, bias, eps, relu, y, mean, var, rstd, scale, shift, nullptr, 0, 1, nullptr,
                        workspace, workspace_bytes, stream,
                        Running{running_mean, running_var, momentum, num_batches_tracked});
}

// the same over the live rows only: mask [n_rois] f32 (0 = dead), rows r*per .. r*per+per-1 belong to
// RoI r (M = n_rois * per); dead rows of y are written as zeros; count[0] receives the number of live
// rows (>= 1) as a float, for the caller's running-variance correction
PLUMB_API int wsplumb_rowbn_forward_masked(const float *x, long long M, int C, const float *weight,
                                           const float *bias, float eps, int relu, const float *mask,
                                           int n_rois, int per, float *y, float *mean, float *var,
                                           float *rstd, float *scale, float *shift, float *count,
                                           void *workspace, size_t workspace_bytes, void *stream,
                                           float *running_mean, float *running_var, float momentum,
                                           long long *num_batches_tracked) {
    if (!mask || !count) return 1;
    return forward_impl(x, M, C, weight, bias, eps, relu, y, mean, var, rstd, scale, shift, mask, n_rois, per, count,
                        workspace, workspace_bytes, stream,
                        Running{running_mean, running_var, momentum, num_batches_tracked});
}

// y = act(x*scale + shift) with given per-column scale / shift (inference statistics)
PLUMB_API int wsplumb_rowbn_apply(const float *x, long long M, int C, const float *scale,
                                  const float *shift, int relu, float *y, void *stream) {
    if (M < 1 || C < 4 || (C & 3)) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long total4 = M * (C / 4);
    if (relu)
        hipLaunchKernelGGL((rowbn_apply_fwd_kernel<true, 0>), dim3(apply_grid(total4)), dim3(BLOCK), 0, st, x,
                           scale, shift, total4, C / 4, y, nullptr, 1);
    else
        hipLaunchKernelGGL((rowbn_apply_fwd_kernel<false, 0>), dim3(apply_grid(total4)), dim3(BLOCK), 0, st, x,
                           scale, shift, total4, C / 4, y, nullptr, 1);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

static int backward_impl(const float *x, const float *dy, long long M, int C, const float *weight,
                         const float *mean, const float *rstd, const float *scale, const float *shift, int relu,
                         float *dx, float *dweight, float *dbias, float *coef, const float *mask, int n_rois,
                         int per, void *workspace, size_t workspace_bytes, void *stream, bool pm = false) {
    if (!shape_ok(M, C) || workspace_bytes < wsplumb_rowbn_workspace_bytes(M, C)) return 1;
    if (mask && (per < 1 || n_rois < 1 || (long long)n_rois * per != M || M > 0x7fffffffLL)) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = partial_blocks(M, C);
    const long long rpb = (M + nb - 1) / nb;
    double *partial = static_cast<double *>(workspace);
    const int div = pm ? n_rois : per;
    const int mode = mask ? (pm ? 2 : 1) : 0;
#define WSPLUMB_PARTIAL(RELU, MASK) \
    hipLaunchKernelGGL((rowbn_partial_kernel<1, RELU, MASK>), dim3(nb), dim3(BLOCK), 0, st, x, dy, scale, shift, M, C, \
                       rpb, partial, mask, div)
    if (relu) { if (mode == 2) WSPLUMB_PARTIAL(true, 2); else if (mode) WSPLUMB_PARTIAL(true, 1); else WSPLUMB_PARTIAL(true, 0); }
    else { if (mode == 2) WSPLUMB_PARTIAL(false, 2); else if (mode) WSPLUMB_PARTIAL(false, 1); else WSPLUMB_PARTIAL(false, 0); }
#undef WSPLUMB_PARTIAL
    hipLaunchKernelGGL(rowbn_bwd_finish_kernel, dim3((C + FIN_COLS - 1) / FIN_COLS), dim3(FIN_COLS * FIN_GROUPS), 0, st, partial, nb, C,
                       M, weight, mean, rstd, dweight, dbias, coef, mask, n_rois, per);
    const long long total4 = M * (C / 4);
#define WSPLUMB_APPLY(RELU, MASK) \
    hipLaunchKernelGGL((rowbn_apply_bwd_kernel<RELU, MASK>), dim3(apply_grid(total4)), dim3(BLOCK), 0, st, x, dy, scale, \
                       shift, coef, total4, C / 4, dx, mask, div)
    if (relu) { if (mode == 2) WSPLUMB_APPLY(true, 2); else if (mode) WSPLUMB_APPLY(true, 1); else WSPLUMB_APPLY(true, 0); }
    else { if (mode == 2) WSPLUMB_APPLY(false, 2); else if (mode) WSPLUMB_APPLY(false, 1); else WSPLUMB_APPLY(false, 0); }
#undef WSPLUMB_APPLY
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// gradients of wsplumb_rowbn_forward: dx [M,C], dweight [C], dbias [C]; coef is [3*C] scratch
PLUMB_API int wsplumb_rowbn_backward(const float *x, const float *dy, long long M, int C,
                                     const float *weight, const float *mean, const float *rstd,
                                     const float *scale, const float *shift, int relu, float *dx,
                                     float *dweight, float *dbias, float *coef, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return backward_impl(x, dy, M, C, weight, mean, rstd, scale, shift, relu, dx, dweight, dbias, coef, nullptr, 0, 1,
                         workspace, workspace_bytes, stream);
}

// gradients of wsplumb_rowbn_forward_masked (dead rows: dy ignored, dx = 0)
PLUMB_API int wsplumb_rowbn_backward_masked(const float *x, const float *dy, long long M, int C,
                                            const float *weight, const float *mean, const float *rstd,
                                            const float *scale, const float *shift, int relu,
                                            const float *mask, int n_rois, int per, float *dx,
                                            float *dweight, float *dbias, float *coef, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    if (!mask) return 1;
    return backward_impl(x, dy, M, C, weight, mean, rstd, scale, shift, relu, dx, dweight, dbias, coef, mask, n_rois, per,
                         workspace, workspace_bytes, stream);
}

// the masked forward on position-major rows: row r belongs to RoI r % n_rois (M = n_rois * per)
PLUMB_API int wsplumb_rowbn_forward_masked_pm(const float *x, long long M, int C, const float *weight,
                                              const float *bias, float eps, int relu, const float *mask,
                                              int n_rois, int per, float *y, float *mean, float *var,
                                              float *rstd, float *scale, float *shift, float *count,
                                              void *workspace, size_t workspace_bytes, void *stream,
                                              float *running_mean, float *running_var, float momentum,
                                              long long *num_batches_tracked) {
    if (!mask || !count) return 1;
    return forward_impl(x, M, C, weight, bias, eps, relu, y, mean, var, rstd, scale, shift, mask, n_rois, per, count,
                        workspace, workspace_bytes, stream,
                        Running{running_mean, running_var, momentum, num_batches_tracked}, true);
}

// gradients of wsplumb_rowbn_forward_masked_pm
PLUMB_API int wsplumb_rowbn_backward_masked_pm(const float *x, const float *dy, long long M, int C,
                                               const float *weight, const float *mean, const float *rstd,
                                               const float *scale, const float *shift, int relu,
                                               const float *mask, int n_rois, int per, float *dx,
                                               float *dweight, float *dbias, float *coef, void *workspace,
                                               size_t workspace_bytes, void *stream) {
    if (!mask) return 1;
    return backward_impl(x, dy, M, C, weight, mean, rstd, scale, shift, relu, dx, dweight, dbias, coef, mask, n_rois, per,
                         workspace, workspace_bytes, stream, true);
}

// gradients of wsplumb_rowbn_forward[_masked] with ReLU for block 1's pre-activation norm, the output's gradient
// given in its two parts (EntryGrad above): dy [n_rois * per, C] roi-major from conv1, dys [n_slots * n_rois, C]
// position-major from the projection shortcut, possel [per] (device) the slot of each position or -1.
// mask may be null.  Bit-identical to wsplumb_rowbn_backward[_masked] on dy + scatter(dys).
PLUMB_API int wsplumb_rowbn_backward_entry(const float *x, const float *dy, const float *dys, const int *possel,
                                           int n_slots, long long M, int C, const float *weight, const float *mean,
                                           const float *rstd, const float *scale, const float *shift,
                                           const float *mask, int n_rois, int per, float *dx, float *dweight,
                                           float *dbias, float *coef, void *workspace, size_t workspace_bytes,
                                           void *stream) {
    if (!shape_ok(M, C) || workspace_bytes < wsplumb_rowbn_workspace_bytes(M, C)) return 1;
    if (!dys || !possel || per < 1 || n_rois < 1 || n_slots < 1 || n_slots > per ||
        (long long)n_rois * per != M || M > 0x7fffffffLL)
        return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = partial_blocks(M, C);
    const long long rpb = (M + nb - 1) / nb;
    double *partial = static_cast<double *>(workspace);
    const EntryGrad eg = {dys, possel, per, n_rois};
    if (mask)
        hipLaunchKernelGGL((rowbn_partial_kernel<1, true, 1, true>), dim3(nb), dim3(BLOCK), 0, st, x, dy, scale, shift, M,
                           C, rpb, partial, mask, per, eg);
    else
        hipLaunchKernelGGL((rowbn_partial_kernel<1, true, 0, true>), dim3(nb), dim3(BLOCK), 0, st, x, dy, scale, shift, M,
                           C, rpb, partial, mask, 1, eg);
    hipLaunchKernelGGL(rowbn_bwd_finish_kernel, dim3((C + FIN_COLS - 1) / FIN_COLS), dim3(FIN_COLS * FIN_GROUPS), 0, st,
                       partial, nb, C, M, weight, mean, rstd, dweight, dbias, coef, mask, n_rois, per);
    const long long total4 = M * (C / 4);
    if (mask)
        hipLaunchKernelGGL((rowbn_apply_bwd_kernel<true, 1, true>), dim3(apply_grid(total4)), dim3(BLOCK), 0, st, x, dy,
                           scale, shift, coef, total4, C / 4, dx, mask, per, eg);
    else
        hipLaunchKernelGGL((rowbn_apply_bwd_kernel<true, 0, true>), dim3(apply_grid(total4)), dim3(BLOCK), 0, st, x, dy,
                           scale, shift, coef, total4, C / 4, dx, mask, 1, eg);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// ---- residual joins (position-major rows; mask may be null: every row live) ----
// Statistic blocks are [5, C] f32: mean, var, rstd, scale, shift (the layout of the Python binding).

// bytes of scratch of one join call: two partial buffers
PLUMB_API size_t wsplumb_rowbn_join_workspace_bytes(long long M, int C) {
    return 2 * wsplumb_rowbn_workspace_bytes(M, C);
}

namespace {

struct JoinGeom {
    hipStream_t st;
    int nb, mode, div;
    long long rpb, total4;
    double *p0, *p1;
};

// 0 when the arguments of a join entry point are usable
inline int join_geom(long long M, int C, const float *mask, int n_rois, int per, void *workspace,
                     size_t workspace_bytes, void *stream, JoinGeom &g) {
    if (!shape_ok(M, C) || workspace_bytes < wsplumb_rowbn_join_workspace_bytes(M, C)) return 1;
    if (mask && (per < 1 || n_rois < 1 || (long long)n_rois * per != M || M > 0x7fffffffLL)) return 1;
    g.st = static_cast<hipStream_t>(stream);
    g.nb = partial_blocks(M, C);
    g.rpb = (M + g.nb - 1) / g.nb;
    g.total4 = M * (C / 4);
    g.mode = mask ? 2 : 0;
    g.div = mask ? n_rois : 1;
    g.p0 = static_cast<double *>(workspace);
    g.p1 = g.p0 + (size_t)g.nb * 2 * C;
    return 0;
}

// statistics of x (no apply): partial sums into g.p0, then the finish kernel
inline void join_stats(const JoinGeom &g, const float *x, long long M, int C, const float *weight, const float *bias,
                       float eps, float *stats, const float *mask, int n_rois, int per, float *count, Running run) {
    if (g.mode)
        hipLaunchKernelGGL((rowbn_partial_kernel<0, false, 2>), dim3(g.nb), dim3(BLOCK), 0, g.st, x, nullptr, nullptr,
                           nullptr, M, C, g.rpb, g.p0, mask, g.div);
    else
        hipLaunchKernelGGL((rowbn_partial_kernel<0, false, 0>), dim3(g.nb), dim3(BLOCK), 0, g.st, x, nullptr, nullptr,
                           nullptr, M, C, g.rpb, g.p0, nullptr, 1);
    hipLaunchKernelGGL(rowbn_fwd_finish_kernel, dim3((C + FIN_COLS - 1) / FIN_COLS), dim3(FIN_COLS * FIN_GROUPS), 0,
                       g.st, g.p0, g.nb, C, M, weight, bias, eps, stats, stats + C, stats + 2 * C, stats + 3 * C,
                       stats + 4 * C, mask, n_rois, per, count, run);
}

inline void join_bwd_finish(const JoinGeom &g, const double *partial, long long M, int C, const float *weight,
                            const float *stats, float *dwb, float *coef, const float *mask, int n_rois, int per) {
    hipLaunchKernelGGL(rowbn_bwd_finish_kernel, dim3((C + FIN_COLS - 1) / FIN_COLS), dim3(FIN_COLS * FIN_GROUPS), 0,
                       g.st, partial, g.nb, C, M, weight, stats, stats + 2 * C, dwb, dwb + C, coef, mask, n_rois, per);
}

}  // namespace

// out = bn3(x3) + other, y = relu(bn_n(out)), all in training mode over the live rows:
//   other is the identity shortcut when weight_s is null, else the input xs of the shortcut's own norm
//   (out = bn3(x3) + bn_s(xs); stats_s is written only then);
//   stats3 / stats_s / stats_n [5, C] and count [1] are what wsplumb_rowbn_forward_masked_pm writes for the
//   three layers (count: once, they share the mask; untouched without a mask);
//   running [6] / momentum [3] / batches [3] (host arrays, or null): the running_mean, running_var pointers, the
//   momentum and the num_batches_tracked pointer of bn3, bn_s, bn_n in that order (struct Running), each
//   updated once, by the finish kernel that writes the layer's statistics.
// Dead rows: out = other (identity form) or 0, y = 0.  Bit-identical to the three (four) separate calls and
// the add between them.
PLUMB_API int wsplumb_rowbn_join_forward(const float *x3, const float *other, long long M, int C,
                                         const float *weight3, const float *bias3, float eps3,
                                         const float *weight_s, const float *bias_s, float eps_s,
                                         const float *weight_n, const float *bias_n, float eps_n,
                                         const float *mask, int n_rois, int per, float *out, float *y,
                                         float *stats3, float *stats_s, float *stats_n, float *count,
                                         void *workspace, size_t workspace_bytes, void *stream,
                                         float *const *running, const float *momentum,
                                         long long *const *batches) {
    JoinGeom g;
    if (join_geom(M, C, mask, n_rois, per, workspace, workspace_bytes, stream, g)) return 1;
    if (mask && !count) return 1;
    const bool dual = weight_s != nullptr;
    if (dual && (!bias_s || !stats_s)) return 1;
    Running run[3] = {};
    for (int k = 0; k < 3; ++k) {
        if (running) { run[k].mean = running[2 * k]; run[k].var = running[2 * k + 1]; }
        if (momentum) run[k].momentum = momentum[k];
        if (batches) run[k].batches = batches[k];
    }
    join_stats(g, x3, M, C, weight3, bias3, eps3, stats3, mask, n_rois, per, nullptr, run[0]);
    if (dual) join_stats(g, other, M, C, weight_s, bias_s, eps_s, stats_s, mask, n_rois, per, nullptr, run[1]);
    const float *sco = dual ? stats_s + 3 * C : nullptr, *sho = dual ? stats_s + 4 * C : nullptr;
#define WSPLUMB_JOIN(DUAL, MASK) \
    hipLaunchKernelGGL((rowbn_join_fwd_kernel<DUAL, MASK>), dim3(g.nb), dim3(BLOCK), 0, g.st, x3, stats3 + 3 * C, \
                       stats3 + 4 * C, other, sco, sho, M, C, g.rpb, out, g.p0, mask, g.div)
    if (dual) { if (g.mode) WSPLUMB_JOIN(true, 2); else WSPLUMB_JOIN(true, 0); }
    else { if (g.mode) WSPLUMB_JOIN(false, 2); else WSPLUMB_JOIN(false, 0); }
#undef WSPLUMB_JOIN
    hipLaunchKernelGGL(rowbn_fwd_finish_kernel, dim3((C + FIN_COLS - 1) / FIN_COLS), dim3(FIN_COLS * FIN_GROUPS), 0,
                       g.st, g.p0, g.nb, C, M, weight_n, bias_n, eps_n, stats_n, stats_n + C, stats_n + 2 * C,
                       stats_n + 3 * C, stats_n + 4 * C, mask, n_rois, per, mask ? count : nullptr, run[2]);
    if (g.mode)
        hipLaunchKernelGGL((rowbn_apply_fwd_kernel<true, 2>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, out,
                           stats_n + 3 * C, stats_n + 4 * C, g.total4, C / 4, y, mask, g.div);
    else
        hipLaunchKernelGGL((rowbn_apply_fwd_kernel<true, 0>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, out,
                           stats_n + 3 * C, stats_n + 4 * C, g.total4, C / 4, y, nullptr, 1);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// gradients of wsplumb_rowbn_join_forward: dy is the gradient of y, dres that of out over the residual path
// (null: none).  g = dx of bn_n + dres is the gradient of `other` in the identity form; dx3 (and dxs, when
// xs / weight_s / stats_s are given) are bn3's (the shortcut norm's) input gradients.  dwb_* are [2, C]:
// dweight, dbias.  coef is [9, C] scratch.
PLUMB_API int wsplumb_rowbn_join_backward(const float *out, const float *dy, const float *dres, const float *x3,
                                          const float *xs, long long M, int C, const float *weight_n,
                                          const float *stats_n, const float *weight3, const float *stats3,
                                          const float *weight_s, const float *stats_s, const float *mask,
                                          int n_rois, int per, float *gout, float *dx3, float *dxs, float *dwb_n,
                                          float *dwb3, float *dwb_s, float *coef, void *workspace,
                                          size_t workspace_bytes, void *stream) {
    JoinGeom g;
    if (join_geom(M, C, mask, n_rois, per, workspace, workspace_bytes, stream, g)) return 1;
    const bool dual = xs != nullptr;
    if (dual && (!weight_s || !stats_s || !dxs || !dwb_s)) return 1;
    float *coef_n = coef, *coef3 = coef + 3 * C, *coefs = coef + 6 * C;
    const float *scn = stats_n + 3 * C, *shn = stats_n + 4 * C;
    if (g.mode)
        hipLaunchKernelGGL((rowbn_partial_kernel<1, true, 2>), dim3(g.nb), dim3(BLOCK), 0, g.st, out, dy, scn, shn, M, C,
                           g.rpb, g.p0, mask, g.div);
    else
        hipLaunchKernelGGL((rowbn_partial_kernel<1, true, 0>), dim3(g.nb), dim3(BLOCK), 0, g.st, out, dy, scn, shn, M, C,
                           g.rpb, g.p0, nullptr, 1);
    join_bwd_finish(g, g.p0, M, C, weight_n, stats_n, dwb_n, coef_n, mask, n_rois, per);
#define WSPLUMB_JOIN(DUAL, RES, MASK) \
    hipLaunchKernelGGL((rowbn_join_bwd_kernel<DUAL, RES, MASK>), dim3(g.nb), dim3(BLOCK), 0, g.st, out, dy, scn, shn, \
                       coef_n, dres, x3, xs, M, C, g.rpb, gout, g.p0, g.p1, mask, g.div)
#define WSPLUMB_JOIN_M(DUAL, RES) do { if (g.mode) WSPLUMB_JOIN(DUAL, RES, 2); else WSPLUMB_JOIN(DUAL, RES, 0); } while (0)
    if (dual) { if (dres) WSPLUMB_JOIN_M(true, true); else WSPLUMB_JOIN_M(true, false); }
    else { if (dres) WSPLUMB_JOIN_M(false, true); else WSPLUMB_JOIN_M(false, false); }
#undef WSPLUMB_JOIN_M
#undef WSPLUMB_JOIN
    join_bwd_finish(g, g.p0, M, C, weight3, stats3, dwb3, coef3, mask, n_rois, per);
    if (dual) {
        join_bwd_finish(g, g.p1, M, C, weight_s, stats_s, dwb_s, coefs, mask, n_rois, per);
        if (g.mode)
            hipLaunchKernelGGL((rowbn_apply_bwd_dual_kernel<2>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, x3, xs,
                               gout, coef3, coefs, g.total4, C / 4, dx3, dxs, mask, g.div);
        else
            hipLaunchKernelGGL((rowbn_apply_bwd_dual_kernel<0>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, x3, xs,
                               gout, coef3, coefs, g.total4, C / 4, dx3, dxs, nullptr, 1);
    } else if (g.mode) {
        hipLaunchKernelGGL((rowbn_apply_bwd_kernel<false, 2>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, x3, gout,
                           nullptr, nullptr, coef3, g.total4, C / 4, dx3, mask, g.div);
    } else {
        hipLaunchKernelGGL((rowbn_apply_bwd_kernel<false, 0>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, x3, gout,
                           nullptr, nullptr, coef3, g.total4, C / 4, dx3, nullptr, 1);
    }
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
