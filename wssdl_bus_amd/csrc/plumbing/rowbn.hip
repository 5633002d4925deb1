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
// LIVE-ROW MASK (the `mask` argument of the entry points).  The rows come in groups of `per` (the h*w positions of
// one RoI); `mask[roi]` = 0 marks a dead RoI -- a padding row of the fixed-shape RoI blob, or of a
// supervised image that ran short of candidates.  Dead rows are skipped by the column sums (not even
// loaded), the statistics are taken over the live rows (n = per * sum(mask), computed on the device:
// no host read-back), and the layer writes zeros for dead rows in both directions, so the live rows
// come out exactly as if the blob had been compacted first.
// With `pos_major` the same mask applies to POSITION-MAJOR rows (row r belongs to RoI r % n_rois: the
// head's 4x4 section, networks/roi_head.py); statistics and outputs are the same.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "bn_math.hip.h"

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
// The fused multiply-adds are written out (why: bn_math.hip.h, which holds y = x*scale + shift, bn_affine, for this
// file and the patch gather of taps.hip).
// dx = a*u - k0 - k1*x (coefficients of rowbn_bwd_finish_kernel)
__device__ __forceinline__ float bn_dx(float ka, float u, float k0, float k1, float x) {
    return __builtin_fmaf(-k1, x, __builtin_fmaf(ka, u, -k0));
}
// The f64 column sums of a thread: two rows per step, then a one-row tail.  Written out as well, in the form the
// compiler's contraction gave every slab kernel before (4 multiplies + 8 fused multiply-adds per float4 column):
//   two rows: q += fma(v0, w0, v1 * w1)        one row: q = fma(v, w, q)
// (The product of two f32 values is exact in f64, so either form rounds as the separate operations would; what is
// pinned is that every instantiation issues the same operations.)
__device__ __forceinline__ void dot_rows2(double &q, float v0, float w0, float v1, float w1) {
#pragma clang fp contract(off)
    const double p1 = (double)v1 * (double)w1;
    q += __builtin_fma((double)v0, (double)w0, p1);
}
__device__ __forceinline__ void dot_row(double &q, float v, float w) { q = __builtin_fma((double)v, (double)w, q); }
__device__ __forceinline__ void acc_rows2(double &s, double &q, float v0, float w0, float v1, float w1) {
    s += (double)v0 + (double)v1;
    dot_rows2(q, v0, w0, v1, w1);
}
__device__ __forceinline__ void acc_row(double &s, double &q, float v, float w) {
    s += (double)v;
    dot_row(q, v, w);
}

// ---- how a slab kernel reads and writes a row: float4 column c4 of row r ----
template <int MASK>
__device__ __forceinline__ bool row_live(const float *__restrict__ mask, long long r, int div) {
    return MASK ? mask[mask_roi<MASK>(r, div)] != 0.0f : true;
}

// zeros, and no load, unless `on`
__device__ __forceinline__ float4v load4(const float *__restrict__ p, long long r, int C, int c4, bool on) {
    const float4v zero4 = {0, 0, 0, 0};
    return on ? reinterpret_cast<const float4v *>(p + (size_t)r * C)[c4] : zero4;
}

__device__ __forceinline__ void store4(float *__restrict__ p, long long r, int C, int c4, float4v v) {
    reinterpret_cast<float4v *>(p + (size_t)r * C)[c4] = v;
}

// ---- block 1's entry gradient (networks/roi_head.py, _EntryNormFn) ----
// Block 1's pre-activation output y (roi-major rows, `per` positions per RoI) feeds conv1 at every position and
// the projection shortcut at the positions it samples.  Its gradient at row r = roi * per + p is
//   dy[r] + (possel[p] >= 0 ? dys[possel[p] * R + roi] + 0 : 0)
// with dy conv1's gradient, dys the shortcut's position-major gradient and possel[p] the shortcut's slot of
// position p (-1: not sampled).  The ENTRY variants of the two backward kernels form it in registers.  The
// "+ 0" is kept: the separate ops scatter dys into a zero tensor first, which turns a -0 into +0.
//
// ---- the head's exit gradient (networks/roi_head.py: the last _JoinFn in its exit form) ----
// The head's output is the mean over the slots of its final norm's position-major output y, so the gradient of y at
// row r is dfeat[r % R] * (1 / n_slots): DY_EXIT forms it in registers from dfeat [R, C] (passed as dy) instead of
// reading a [n_slots * R, C] expansion of it.  Same values, so whatever a kernel computes from them is the same.
enum DySrc { DY_PLAIN, DY_ENTRY, DY_EXIT };

struct EntryGrad {
    const float *dys;       // DY_ENTRY: [n_slots * R, C]
    const int *possel;      // DY_ENTRY: [per]
    int per, R;             // R also DY_EXIT
    float inv;              // DY_EXIT: slot_mean_scale(n_slots)
};

template <DySrc SRC>
__device__ __forceinline__ float4v load_dy(const float *__restrict__ dy, const EntryGrad &e, long long r, int C, int c4,
                                           bool on = true) {
    const float4v zero4 = {0, 0, 0, 0};
    if (!on) return zero4;
    if (SRC == DY_EXIT) {
        const unsigned roi = (unsigned)r % (unsigned)e.R;
        return reinterpret_cast<const float4v *>(dy + (size_t)roi * C)[c4] * e.inv;
    }
    const float4v g = reinterpret_cast<const float4v *>(dy + (size_t)r * C)[c4];
    if (SRC == DY_PLAIN) return g;
    const unsigned roi = (unsigned)r / (unsigned)e.per, p = (unsigned)r - roi * (unsigned)e.per;
    const int slot = e.possel[p];
    float4v d = zero4;
    if (slot >= 0) d = reinterpret_cast<const float4v *>(e.dys + ((size_t)slot * e.R + roi) * C)[c4] + zero4;
    return g + d;
}

// ---- row slabs ----
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

// What one row adds to the sums of its float4 column: s += v, q += v * w and, for a functor with TWO_Q, q2 += v * w2.
struct Term {
    float4v v, w, w2;
};

// THE walk of a row slab, shared by rowbn_partial_kernel and rowbn_join_bwd_kernel (rowbn_join_fwd_kernel keeps a
// hand-written copy of it, see there: a change to the walk has to be made in both): column chunk by column chunk,
// two rows in flight per step and a one-row tail, the f64 sums of the live rows in the one association of acc_rows2 /
// acc_row, then the fixed-order reduction into this block's partials (out; out2 takes (s, q2) with TWO_Q).  A kernel
// supplies its columns as a functor F:
//   f.setup(c4)                      per column chunk: its per-column constants
//   f.load(r, c4, live) -> F::Row    the row's loads, nothing else (a dead row loads nothing from a masked operand)
//   f.finish(row, r, c4, live)       the element arithmetic and any store; returns the row's Term
//   F::VISITS_DEAD                   false: the kernel writes nothing per row, dead rows are skipped unloaded (a pair
//                                    when both are dead); true: every row is finished, a dead row must still be stored
//   F::TWO_Q                         a second product sum over the same v (the dual backward join)
// Both rows of a pair are loaded before either is finished.  A dead row adds nothing: in a pair its term counts as
// v = w = 0 (so the pair's operations stay those of two rows), the tail leaves it out.  The kernels that go through
// here leave exactly the partials rowbn_partial_kernel would compute from the same v and w because they share this
// walk; the forward join's copy is held to it by the bit-for-bit join tests (tests/test_gpu_head_join.py).
template <int MASK, class F>
__device__ __forceinline__ void slab_walk(const Slab &b, int C, const float *__restrict__ mask, int div, F &f,
                                          double (*red)[8], double *__restrict__ out,
                                          double *__restrict__ out2 = nullptr) {
    const int RS = b.RS;
    for (int cc = 0; cc * b.L < b.C4; ++cc) {
        const int c4 = cc * b.L + b.lc;
        double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0}, q2[4] = {0, 0, 0, 0};
        f.setup(c4);
        if (b.lr < RS) {
            long long r = b.r0 + b.lr;
#pragma unroll 1
            for (; r + RS < b.r1; r += 2 * RS) {
                const bool live0 = row_live<MASK>(mask, r, div), live1 = row_live<MASK>(mask, r + RS, div);
                if (!F::VISITS_DEAD && !live0 && !live1) continue;
                const typename F::Row a0 = f.load(r, c4, live0), a1 = f.load(r + RS, c4, live1);
                const Term t0 = f.finish(a0, r, c4, live0), t1 = f.finish(a1, r + RS, c4, live1);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v0 = live0 ? t0.v[j] : 0.0f, v1 = live1 ? t1.v[j] : 0.0f;
                    acc_rows2(s[j], q[j], v0, live0 ? t0.w[j] : 0.0f, v1, live1 ? t1.w[j] : 0.0f);
                    if (F::TWO_Q) dot_rows2(q2[j], v0, live0 ? t0.w2[j] : 0.0f, v1, live1 ? t1.w2[j] : 0.0f);
                }
            }
            for (; r < b.r1; r += RS) {
                const bool live = row_live<MASK>(mask, r, div);
                if (!F::VISITS_DEAD && !live) continue;
                const Term t = f.finish(f.load(r, c4, live), r, c4, live);
                if (live) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc_row(s[j], q[j], t.v[j], t.w[j]);
                        if (F::TWO_Q) dot_row(q2[j], t.v[j], t.w2[j]);
                    }
                }
            }
        }
        slab_reduce(b, C, c4, s, q, red, out);
        if (F::TWO_Q) slab_reduce(b, C, c4, s, q2, red, out2);
    }
}

// Partial column sums of one row slab.
// MODE 0: s = sum x,  q = sum x*x
// MODE 1: s = sum g,  q = sum g*x   with g = dy, masked by (x*scale + shift > 0) when RELU
// SRC: where dy comes from (MODE 1, M < 2^31 unless DY_PLAIN): block 1's entry gradient (roi-major rows) or the
// head's exit gradient (position-major rows)
template <int MODE, bool RELU, DySrc SRC>
struct PartialCols {
    static constexpr bool VISITS_DEAD = false, TWO_Q = false;
    const float *x, *dy, *scale, *shift;
    int C;
    EntryGrad eg;
    float4v sc, sh;
    struct Row {
        float4v a, g;
    };
    __device__ __forceinline__ void setup(int c4) {
        if (MODE == 1 && RELU) {
            sc = reinterpret_cast<const float4v *>(scale)[c4];
            sh = reinterpret_cast<const float4v *>(shift)[c4];
        }
    }
    __device__ __forceinline__ Row load(long long r, int c4, bool live) const {
        Row w = {load4(x, r, C, c4, live), {0, 0, 0, 0}};
        if (MODE == 1) w.g = load_dy<SRC>(dy, eg, r, C, c4, live);
        return w;
    }
    __device__ __forceinline__ Term finish(const Row &w, long long, int, bool) const {
        Term t = {w.a, w.a, {0, 0, 0, 0}};
        if (MODE == 1) {
            t.v = w.g;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (RELU && !(bn_affine(w.a[j], sc[j], sh[j]) > 0.0f)) t.v[j] = 0.0f;
        }
        return t;
    }
};

template <int MODE, bool RELU, int MASK, DySrc SRC = DY_PLAIN>
__global__ __launch_bounds__(BLOCK) void rowbn_partial_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ scale,
    const float *__restrict__ shift, long long M, int C, long long rows_per_block,
    double *__restrict__ partial, const float *__restrict__ mask, int per, EntryGrad eg = EntryGrad()) {
    __shared__ double red[BLOCK][8];
    const Slab b(M, C, rows_per_block);
    PartialCols<MODE, RELU, SRC> f = {x, dy, scale, shift, C, eg};
    slab_walk<MASK>(b, C, mask, per, f, red, partial + (size_t)blockIdx.x * 2 * C);
}

// Sum of the per-workgroup partials of 16 columns, in a fixed order: 64 row groups of 16 lanes
// each add every 64th partial (in order), then lane-wise the 64 group sums are added in order.
// A thread owns the partials b = grp, grp + 64, ...: at most FIN_DEPTH of them.  All of its loads are issued before
// the first addition (a load per step and a wait for it made the kernel a chain of FIN_DEPTH trips to memory); the
// additions are those of the plain loop, in its order, from 0.0: a step past nblocks loads nothing and adds nothing.
constexpr int FIN_COLS = 16, FIN_GROUPS = 64, FIN_DEPTH = MAX_PARTIAL_BLOCKS / FIN_GROUPS, WAVE = 64;
static_assert(MAX_PARTIAL_BLOCKS == FIN_DEPTH * FIN_GROUPS && FIN_DEPTH == 16, "a finish thread owns at most 16 partials");
static_assert((FIN_COLS * FIN_GROUPS) % WAVE == 0 && FIN_COLS * FIN_GROUPS / WAVE <= WAVE, "live_rows: one LDS step");

__device__ __forceinline__ void finish_reduce(const double *__restrict__ partial, int nblocks, int C,
                                              int c, int grp, double (*red)[FIN_COLS][2], double &s,
                                              double &q) {
    double ps[FIN_DEPTH], pq[FIN_DEPTH];
#pragma unroll
    for (int k = FIN_DEPTH - 1; k >= 0; --k) {      // issue order only (last step first: the compiler keeps the first
        const int b = grp + k * FIN_GROUPS;         // addition next to the load of step 0, so that load goes out last)
        ps[k] = pq[k] = 0.0;
        if (c < C && b < nblocks) {
            ps[k] = partial[(size_t)b * 2 * C + c];
            pq[k] = partial[(size_t)b * 2 * C + C + c];
        }
    }
    double ss = 0.0, qq = 0.0;
#pragma unroll
    for (int k = 0; k < FIN_DEPTH; ++k)
        if (c < C && grp + k * FIN_GROUPS < nblocks) {
            ss += ps[k];
            qq += pq[k];
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
// Every thread of the workgroup returns the same value.  The live RoIs are counted as integers (a sum of 0 / 1
// values, exact in any order; n_rois < 2^31): LIVE_LOADS mask loads in flight per thread, a shuffle reduction within each
// wave, one LDS step across the waves, and one conversion to f64.
__device__ __forceinline__ double live_rows(const float *__restrict__ mask, int n_rois, int per, long long M,
                                            double *scratch /* [FIN_COLS * FIN_GROUPS] LDS */) {
    if (!mask) return (double)M;
    constexpr int T = FIN_COLS * FIN_GROUPS, NW = T / WAVE, LIVE_LOADS = 8;
    int n = 0;
    const unsigned last = (unsigned)n_rois - 1;     // a step past the end re-reads the last entry and does not count
    for (unsigned i0 = threadIdx.x; i0 <= last; i0 += LIVE_LOADS * T) {     // unsigned: n_rois + LIVE_LOADS * T < 2^32
        float m[LIVE_LOADS];
#pragma unroll
        for (int k = 0; k < LIVE_LOADS; ++k) {
            const unsigned i = i0 + k * T;
            m[k] = mask[i <= last ? i : last];
        }
#pragma unroll
        for (int k = 0; k < LIVE_LOADS; ++k) n += (i0 + k * T <= last && m[k] != 0.0f) ? 1 : 0;
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) n += __shfl_xor(n, d, WAVE);
    int *cnt = reinterpret_cast<int *>(scratch);
    __syncthreads();
    if (threadIdx.x % WAVE == 0) cnt[threadIdx.x / WAVE] = n;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) total += cnt[w];
    __syncthreads();
    const double t = (double)total * (double)per;
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

// Batch renormalisation (Ioffe 2017; tf.layers.batch_normalization(renorm=True), no clipping) of one norm: the
// layer's three state vectors, each f32 [C] and updated in place by the forward finish kernel, the moving-average
// factor rho of that update, and where the step's correction factors go (rows 5 and 6 of a [7, C] statistic block).
// The weight is kept per column (all entries equal): a column's thread reads and writes only its own entries, so no
// finish workgroup can see another's update.  mean == nullptr: a plain batch norm.
//   W, Rm, Rs = weight, mean, stddev BEFORE this step;  sigma = sqrt(v + eps)
//   mixed_mean = Rm + (1 - W) * mu;   mixed_std = Rs + (1 - W) * sigma
//   r = sigma / mixed_std;   d = (mu - mixed_mean) / mixed_std             (constants of the backward)
//   y = w * ((x - mu) / sigma * r + d) + b = x * scale + shift
// all of it in f64 from the f64 mu / v of the column sums and the f32 state, every operation rounded on its own; r, d
// and mixed_mean are rounded to f32 once, then in f32, as the plain layer forms them,
//   scale = (rstd * r) * w;   shift = fmaf(-scale, mixed_mean, b)          (w * d + b - scale * mu, regrouped)
// so that a fresh layer (W = Rm = Rs = 0: r = 1, d = 0, mixed_mean = mu exactly) writes the plain layer's bits.
// Then the state and, from the ROUNDED new state, the running statistics (no n / (n - 1) factor on this path):
//   Rm' = (float)(Rm + (mu - Rm) * (1 - rho));  Rs' = (float)(Rs + (sigma - Rs) * (1 - rho));
//   W'  = (float)(W + (1 - W) * (1 - rho))
//   running_mean += momentum * (Rm' / W' - running_mean);   running_var += momentum * ((Rs' / W')^2 - eps - running_var)
struct Renorm {
    float *mean, *stddev, *weight;
    double momentum;                // rho, a double: 1 - rho cancels, and f32(0.99) would put 1e-6 of error into every update
    float *r, *d;
};

// s + (x - s) * k, every f64 operation rounded on its own (the host restates it)
__device__ __forceinline__ double renorm_lerp(double s, double x, double k) {
#pragma clang fp contract(off)
    const double t = x - s;
    const double p = t * k;
    return s + p;
}

struct RenormFactors {
    float r, d, mixed_mean;
};

// the renorm part of the forward finish for column c: r, d and mixed_mean of this step, the state and the running
// statistics updated (struct Renorm above has the operation order)
__device__ __forceinline__ RenormFactors renorm_column(const Renorm &rn, const Running &run, int c, double mu, double v,
                                                       float eps) {
#pragma clang fp contract(off)
    const double sigma = sqrt(v + (double)eps);
    const double W = rn.weight[c], Rm = rn.mean[c], Rs = rn.stddev[c];
    const double omw = 1.0 - W;
    const double pm = omw * mu;
    const double mixed_mean = Rm + pm;
    const double ps = omw * sigma;
    const double mixed_std = Rs + ps;
    const double dm = mu - mixed_mean;
    const RenormFactors f = {(float)(sigma / mixed_std), (float)(dm / mixed_std), (float)mixed_mean};
    const double k = 1.0 - rn.momentum;
    const float Rm1 = (float)renorm_lerp(Rm, mu, k), Rs1 = (float)renorm_lerp(Rs, sigma, k);
    const float W1 = (float)renorm_lerp(W, 1.0, k);
    rn.mean[c] = Rm1;
    rn.stddev[c] = Rs1;
    rn.weight[c] = W1;
    const double mom = (double)run.momentum;
    if (run.mean) run.mean[c] = (float)renorm_lerp((double)run.mean[c], (double)Rm1 / (double)W1, mom);
    if (run.var) {
        const double q = (double)Rs1 / (double)W1;
        const double q2 = q * q;
        run.var[c] = (float)renorm_lerp((double)run.var[c], q2 - (double)eps, mom);
    }
    return f;
}

// forward finish: mean / biased var / scale / shift per column, and the running statistics; RENORM: the layer is a
// batch renormalisation (struct Renorm), which changes scale and shift and adds r, d and the state update
template <bool RENORM>
__device__ __forceinline__ void fwd_finish(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ bias, float eps,
    float *__restrict__ mean, float *__restrict__ var, float *__restrict__ rstd,
    float *__restrict__ scale, float *__restrict__ shift, const float *__restrict__ mask, int n_rois, int per,
    float *__restrict__ count, const Running &run, const Renorm &rn) {
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
    // The fused multiply-adds are written out, as the compiler's contraction always formed them (the host restates
    // these lines: tests/test_gpu_rowbn_finish.py): v = fma(-mu, mu, q / n), shift = fmaf(-scale, mean, bias).
    const double mu = s / Mn;
    double v = __builtin_fma(-mu, mu, q / Mn);
    if (v < 0.0) v = 0.0;
    const float rs = (float)(1.0 / sqrt(v + (double)eps));
    if (RENORM) {
        const RenormFactors f = renorm_column(rn, run, c, mu, v, eps);
        const float scl = (rs * f.r) * weight[c];
        mean[c] = (float)mu;
        var[c] = (float)v;
        rstd[c] = rs;
        scale[c] = scl;
        shift[c] = __builtin_fmaf(-scl, f.mixed_mean, bias[c]);
        rn.r[c] = f.r;
        rn.d[c] = f.d;
        return;
    }
    const float scl = rs * weight[c];
    mean[c] = (float)mu;
    var[c] = (float)v;
    rstd[c] = rs;
    scale[c] = scl;
    shift[c] = __builtin_fmaf(-scl, (float)mu, bias[c]);
    const double mom = (double)run.momentum;
    if (run.mean) run.mean[c] = running_update(run.mean[c], (float)mu, 1.0, mom);
    if (run.var) run.var[c] = running_update(run.var[c], (float)v, Mn / (Mn - 1.0 > 1.0 ? Mn - 1.0 : 1.0), mom);
}

__global__ __launch_bounds__(FIN_COLS * FIN_GROUPS) void rowbn_fwd_finish_kernel(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ bias, float eps,
    float *__restrict__ mean, float *__restrict__ var, float *__restrict__ rstd,
    float *__restrict__ scale, float *__restrict__ shift, const float *__restrict__ mask, int n_rois, int per,
    float *__restrict__ count, Running run) {
    fwd_finish<false>(partial, nblocks, C, M, weight, bias, eps, mean, var, rstd, scale, shift, mask, n_rois, per, count,
                      run, Renorm());
}

__global__ __launch_bounds__(FIN_COLS * FIN_GROUPS) void rowbn_fwd_finish_renorm_kernel(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ bias, float eps,
    float *__restrict__ mean, float *__restrict__ var, float *__restrict__ rstd,
    float *__restrict__ scale, float *__restrict__ shift, const float *__restrict__ mask, int n_rois, int per,
    float *__restrict__ count, Running run, Renorm rn) {
    fwd_finish<true>(partial, nblocks, C, M, weight, bias, eps, mean, var, rstd, scale, shift, mask, n_rois, per, count,
                     run, rn);
}

// backward finish: dweight, dbias and the three coefficients of dx = a*g - k0 - k1*x.  RENORM: the forward's r and d
// (constants: no gradient flows through them) enter as a = (w * r) * rstd and dweight = r * sum_g_xhat + d * sum_g,
// product, product and sum each rounded on its own in f64; k1 and k0 follow from that a.
template <bool RENORM>
__device__ __forceinline__ void bwd_finish(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ mean,
    const float *__restrict__ rstd, float *__restrict__ dweight, float *__restrict__ dbias,
    float *__restrict__ coef, const float *__restrict__ mask, int n_rois, int per,
    const float *__restrict__ rn_r, const float *__restrict__ rn_d) {
    __shared__ double red[FIN_GROUPS][FIN_COLS][2];
    const int grp = threadIdx.x / FIN_COLS;
    const int c = blockIdx.x * FIN_COLS + threadIdx.x % FIN_COLS;
    const double Mn = live_rows(mask, n_rois, per, M, &red[0][0][0]);
    double sg, sgx;
    finish_reduce(partial, nblocks, C, c, grp, red, sg, sgx);
    if (grp != 0 || c >= C) return;
    // fused multiply-adds written out as in the forward finish: fma(-mu, sg, sgx) and k0 = fma(-k1, mu, a * sg / n)
    const double mu = mean[c], rs = rstd[c], w = weight[c];
    const double sum_g_xhat = __builtin_fma(-mu, sg, sgx) * rs;
    double a = w * rs, dw = sum_g_xhat;
    if (RENORM) {
#pragma clang fp contract(off)
        const double r = rn_r[c], d = rn_d[c];
        const double wr = w * r;
        a = wr * rs;
        const double p0 = r * sum_g_xhat;
        const double p1 = d * sg;
        dw = p0 + p1;
    }
    const double k1 = a * rs * sum_g_xhat / Mn;
    const double k0 = __builtin_fma(-k1, mu, a * sg / Mn);
    dweight[c] = (float)dw;
    dbias[c] = (float)sg;
    coef[c] = (float)a;
    coef[C + c] = (float)k0;
    coef[2 * C + c] = (float)k1;
}

__global__ __launch_bounds__(FIN_COLS * FIN_GROUPS) void rowbn_bwd_finish_kernel(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ mean,
    const float *__restrict__ rstd, float *__restrict__ dweight, float *__restrict__ dbias,
    float *__restrict__ coef, const float *__restrict__ mask, int n_rois, int per) {
    bwd_finish<false>(partial, nblocks, C, M, weight, mean, rstd, dweight, dbias, coef, mask, n_rois, per, nullptr,
                      nullptr);
}

__global__ __launch_bounds__(FIN_COLS * FIN_GROUPS) void rowbn_bwd_finish_renorm_kernel(
    const double *__restrict__ partial, int nblocks, int C, long long M,
    const float *__restrict__ weight, const float *__restrict__ mean,
    const float *__restrict__ rstd, float *__restrict__ dweight, float *__restrict__ dbias,
    float *__restrict__ coef, const float *__restrict__ mask, int n_rois, int per,
    const float *__restrict__ rn_r, const float *__restrict__ rn_d) {
    bwd_finish<true>(partial, nblocks, C, M, weight, mean, rstd, dweight, dbias, coef, mask, n_rois, per, rn_r, rn_d);
}

// Block 1's entry (networks/roi_head.py, _EntryNormFn): besides y (roi-major rows, `per` positions per RoI), the
// forward apply pass writes the rows of the positions the projection shortcut samples a second time, position-major:
// ys[possel[p] * R + roi] = y[roi * per + p] where possel[p] >= 0 (the table of EntryGrad).  A copy of the float4 it
// has just stored, zeros for a dead RoI.
struct EntryRows {
    float *ys;              // [n_slots * R, C]
    const int *possel;      // [per]
    int per, R;
};

template <bool RELU, int MASK, bool ENTRY = false>
__global__ __launch_bounds__(BLOCK) void rowbn_apply_fwd_kernel(
    const float *__restrict__ x, const float *__restrict__ scale, const float *__restrict__ shift,
    long long total4, int C4, float *__restrict__ y, const float *__restrict__ mask, int per,
    EntryRows er = EntryRows()) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total4;
         i += (long long)gridDim.x * BLOCK) {
        const int c4 = (int)(i % C4);
        float4v *ys4 = nullptr;     // where this row goes in ys, if anywhere
        if (ENTRY) {
            const unsigned r = (unsigned)(i / C4), roi = r / (unsigned)er.per, p = r - roi * (unsigned)er.per;
            const int slot = er.possel[p];
            if (slot >= 0) ys4 = reinterpret_cast<float4v *>(er.ys) + ((size_t)slot * er.R + roi) * C4 + c4;
        }
        if (MASK && mask[mask_roi<MASK>(i / C4, per)] == 0.0f) {
            const float4v zero4 = {0, 0, 0, 0};
            reinterpret_cast<float4v *>(y)[i] = zero4;
            if (ENTRY && ys4) *ys4 = zero4;
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
        if (ENTRY && ys4) *ys4 = o;
    }
}

// The head's exit: feat[roi] = the mean over the slots (bn_math.hip.h: slot order, chunks of 16, a balanced tree per
// chunk) of the position-major rows x[slot * R + roi] -- with NORM of relu(x*scale + shift), the final norm's output
// as rowbn_apply_fwd_kernel<true> would write it, which is then never written.  A dead RoI's row of feat is zero and
// nothing of it is read.  One thread per (roi, float4 column), 16 loads in flight.  MASK is 0 or 2.
template <bool NORM, int MASK>
__global__ __launch_bounds__(BLOCK) void rowbn_slot_mean_kernel(
    const float *__restrict__ x, const float *__restrict__ scale, const float *__restrict__ shift, int n_slots, int R,
    int C4, float *__restrict__ feat, const float *__restrict__ mask) {
    const long long total4 = (long long)R * C4;
    const float inv = slot_mean_scale(n_slots);
    const float4v zero4 = {0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total4;
         i += (long long)gridDim.x * BLOCK) {
        const int c4 = (int)(i % C4);
        const long long roi = i / C4;
        float4v acc = zero4;
        if (!(MASK && mask[roi] == 0.0f)) {
            float4v sc = zero4, sh = zero4;
            if (NORM) {
                sc = reinterpret_cast<const float4v *>(scale)[c4];
                sh = reinterpret_cast<const float4v *>(shift)[c4];
            }
            for (int s0 = 0; s0 < n_slots; s0 += SLOT_CHUNK) {
                float4v v[SLOT_CHUNK];
                // a place past the last slot re-reads the last slot's row (no branch per load) and is set to +0
#pragma unroll
                for (int k = 0; k < SLOT_CHUNK; ++k) {
                    const int slot = s0 + k < n_slots ? s0 + k : n_slots - 1;
                    v[k] = reinterpret_cast<const float4v *>(x)[((size_t)slot * R + roi) * C4 + c4];
                }
#pragma unroll
                for (int k = 0; k < SLOT_CHUNK; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float t = NORM ? bn_affine_relu(v[k][j], sc[j], sh[j]) : v[k][j];
                        v[k][j] = s0 + k < n_slots ? t : 0.0f;
                    }
                const float4v cs = slot_chunk_sum(v);
                acc = s0 == 0 ? cs : acc + cs;
            }
            acc = acc * inv;
        }
        reinterpret_cast<float4v *>(feat)[i] = acc;
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
        const float4v g = ENTRY ? load_dy<DY_ENTRY>(dy, eg, i / C4, C, c4) : reinterpret_cast<const float4v *>(dy)[i];
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
// norm (or the head's final norm) then takes its statistics over out.  Both join kernels walk row slabs as
// rowbn_partial_kernel does (the backward join through slab_walk itself), so the f64 partials they leave are
// those that kernel would compute from the tensor they write.  Unlike it they store every row, dead ones too.
// MASK is 0 or 2 (the joins are position-major).

// Forward join: writes out = act_mask(x3*sc3 + sh3) + (DUAL ? act_mask(other*sco + sho) : other), act_mask
// being zero on dead rows, and the partials (sum, sum of squares over the live rows) of out.
// This kernel keeps a walk of its own, a copy of slab_walk's built from the same pieces (Slab, row_live, load4, store4,
// slab_reduce), and sums through acc_rows2_loose / acc_row_loose, the accumulation as it was before it was pinned:
// through the walker, and equally with the pinned sums in this loop, the <true, 2> instantiation waits for each of
// its conditional loads on its own (21 % slower).  The sums are the same bits either way (exact products).
// Change this loop and slab_walk together.
__device__ __forceinline__ void acc_rows2_loose(double &s, double &q, float v0, float w0, float v1, float w1) {
    s += (double)v0 + (double)v1;
    q += (double)v0 * (double)w0 + (double)v1 * (double)w1;
}
__device__ __forceinline__ void acc_row_loose(double &s, double &q, float v, float w) {
    s += (double)v;
    q += (double)v * (double)w;
}

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
                    acc_rows2_loose(s[j], q[j], v0, v0, v1, v1);
                }
                store4(out, r, C, c4, y0);
                store4(out, r + RS, C, c4, y1);
            }
            for (; r < b.r1; r += RS) {
                const bool live0 = row_live<MASK>(mask, r, div);
                const float4v a0 = load4(x3, r, C, c4, live0), o0 = load4(other, r, C, c4, !DUAL || live0);
                float4v y0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y0[j] = join(a0[j], o0[j], j, live0);
                    if (live0) acc_row_loose(s[j], q[j], y0[j], y0[j]);
                }
                store4(out, r, C, c4, y0);
            }
        }
        slab_reduce(b, C, c4, s, q, red, pout);
    }
}

// Backward join: writes g = (a*u - k0 - k1*xo) + d_res -- the dx of the norm that follows the join (its
// coefficients in coef, u = dy masked by the recomputed ReLU of xo*scn + shn; zero on dead rows) plus, with
// RES, the gradient arriving over the residual path -- and the partials bn3's backward takes over it:
// partial3 = (sum g, sum g*x3) and, with DUAL, partials = (sum g, sum g*xs), live rows only.
// SRC = DY_EXIT: dy is the head's exit gradient, formed from dfeat (the last join of the head; it has no dres).
template <bool DUAL, bool RES, DySrc SRC>
struct JoinBwdCols {
    static constexpr bool VISITS_DEAD = true, TWO_Q = DUAL;
    const float *xo, *dy, *scn, *shn, *coef, *dres, *x3, *xs;
    float *g;
    int C;
    EntryGrad eg;
    float4v sc, sh, ka, k0, k1;
    struct Row {
        float4v x, d, e, a, b;
    };
    __device__ __forceinline__ void setup(int c4) {
        sc = reinterpret_cast<const float4v *>(scn)[c4];
        sh = reinterpret_cast<const float4v *>(shn)[c4];
        ka = reinterpret_cast<const float4v *>(coef)[c4];
        k0 = reinterpret_cast<const float4v *>(coef + C)[c4];
        k1 = reinterpret_cast<const float4v *>(coef + 2 * C)[c4];
    }
    __device__ __forceinline__ Row load(long long r, int c4, bool live) const {
        const float4v a = load4(xo, r, C, c4, live);
        const float4v d = SRC == DY_PLAIN ? load4(dy, r, C, c4, live) : load_dy<SRC>(dy, eg, r, C, c4, live);
        return {a, d, load4(dres, r, C, c4, RES), load4(x3, r, C, c4, live),
                load4(xs, r, C, c4, DUAL && live)};
    }
    __device__ __forceinline__ Term finish(const Row &w, long long r, int c4, bool live) const {
        float4v o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float u = w.d[j];
            if (!(bn_affine(w.x[j], sc[j], sh[j]) > 0.0f)) u = 0.0f;
            const float dx = live ? bn_dx(ka[j], u, k0[j], k1[j], w.x[j]) : 0.0f;
            o[j] = RES ? dx + w.e[j] : dx;
        }
        store4(g, r, C, c4, o);
        return {o, w.a, w.b};
    }
};

template <bool DUAL, bool RES, int MASK, DySrc SRC = DY_PLAIN>
__global__ __launch_bounds__(BLOCK) void rowbn_join_bwd_kernel(
    const float *__restrict__ xo, const float *__restrict__ dy, const float *__restrict__ scn,
    const float *__restrict__ shn, const float *__restrict__ coef, const float *__restrict__ dres,
    const float *__restrict__ x3, const float *__restrict__ xs, long long M, int C, long long rows_per_block,
    float *__restrict__ g, double *__restrict__ partial3, double *__restrict__ partials,
    const float *__restrict__ mask, int div, EntryGrad eg = EntryGrad()) {
    __shared__ double red[BLOCK][8];
    const Slab b(M, C, rows_per_block);
    JoinBwdCols<DUAL, RES, SRC> f = {xo, dy, scn, shn, coef, dres, x3, xs, g, C, eg};
    slab_walk<MASK>(b, C, mask, div, f, red, partial3 + (size_t)blockIdx.x * 2 * C,
                    DUAL ? partials + (size_t)blockIdx.x * 2 * C : nullptr);
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

// bytes of scratch of one join call: two partial buffers
PLUMB_API size_t wsplumb_rowbn_join_workspace_bytes(long long M, int C) {
    return 2 * wsplumb_rowbn_workspace_bytes(M, C);
}

namespace {

// Everything a launch needs to know about one call's rows: filled, and the call's arguments checked, by make_geom.
struct Geom {
    hipStream_t st;
    long long M, rpb, total4;
    int C, nb;
    const float *mask;      // null: every row live
    int mode, div;          // mask mode and row -> RoI divisor of the kernels (mask_roi); 0, 1 without a mask
    int n_rois, per;
    double *p0, *p1;        // partial buffers in the workspace (p1 with n_partials = 2)
};

// THE argument check of every entry point; returns 0 and fills g when the call may launch.
//   n_partials   partial buffers the workspace must hold (0: an elementwise call, any C % 4 == 0)
//   grouped      the rows must come as n_rois groups of `per` even without a mask (the entry gradient)
//   args_ok      the entry point's own requirements on its optional pointers, evaluated by the caller
inline int make_geom(Geom &g, long long M, int C, const float *mask, int n_rois, int per, bool pos_major, bool grouped,
                     bool args_ok, void *workspace, size_t workspace_bytes, int n_partials, void *stream) {
    if (!args_ok || M < 1 || C < 4 || (C & 3)) return 1;
    if (n_partials && (!shape_ok(M, C) || workspace_bytes < n_partials * wsplumb_rowbn_workspace_bytes(M, C))) return 1;
    if (pos_major && !mask) return 1;
    if ((mask || grouped) && (per < 1 || n_rois < 1 || (long long)n_rois * per != M || M > 0x7fffffffLL)) return 1;
    g.st = static_cast<hipStream_t>(stream);
    g.M = M;
    g.C = C;
    g.nb = n_partials ? partial_blocks(M, C) : 0;
    g.rpb = n_partials ? (M + g.nb - 1) / g.nb : 0;
    g.total4 = M * (C / 4);
    g.mask = mask;
    g.mode = mask ? (pos_major ? 2 : 1) : 0;
    g.div = mask ? (pos_major ? n_rois : per) : 1;
    g.n_rois = n_rois;
    g.per = per;
    g.p0 = static_cast<double *>(workspace);
    g.p1 = g.p0 + (size_t)g.nb * 2 * C;
    return 0;
}

// THE place where a runtime flag becomes a template argument: f(std::integral_constant<.., V>) for the V equal to v.
template <auto... Vs, class T, class F>
inline void pick(T v, F &&f) {
    (void)((v == Vs && (f(std::integral_constant<decltype(Vs), Vs>{}), true)) || ...);
}

// column sums of x (MODE 0 of rowbn_partial_kernel)
inline void launch_sums(const Geom &g, const float *x, double *partial) {
    pick<0, 1, 2>(g.mode, [&](auto MASK) {
        hipLaunchKernelGGL((rowbn_partial_kernel<0, false, MASK>), dim3(g.nb), dim3(BLOCK), 0, g.st, x, nullptr, nullptr,
                           nullptr, g.M, g.C, g.rpb, partial, g.mask, g.div);
    });
}

// column sums of g and g*x (MODE 1); with eg, dy is given in the two parts of the entry gradient or, with `exit`, as
// the head's dfeat (relu in both)
inline void launch_grad_sums(const Geom &g, const float *x, const float *dy, const float *scale, const float *shift,
                             bool relu, const EntryGrad *eg, double *partial, bool exit = false) {
    if (eg && exit)
        pick<0, 2>(g.mode, [&](auto MASK) {
            hipLaunchKernelGGL((rowbn_partial_kernel<1, true, MASK, DY_EXIT>), dim3(g.nb), dim3(BLOCK), 0, g.st, x, dy,
                               scale, shift, g.M, g.C, g.rpb, partial, g.mask, g.div, *eg);
        });
    else if (eg)
        pick<0, 1>(g.mode, [&](auto MASK) {
            hipLaunchKernelGGL((rowbn_partial_kernel<1, true, MASK, DY_ENTRY>), dim3(g.nb), dim3(BLOCK), 0, g.st, x, dy,
                               scale, shift, g.M, g.C, g.rpb, partial, g.mask, g.div, *eg);
        });
    else
        pick<false, true>(relu, [&](auto RELU) {
            pick<0, 1, 2>(g.mode, [&](auto MASK) {
                hipLaunchKernelGGL((rowbn_partial_kernel<1, RELU, MASK>), dim3(g.nb), dim3(BLOCK), 0, g.st, x, dy, scale,
                                   shift, g.M, g.C, g.rpb, partial, g.mask, g.div);
            });
        });
}

// rn (null, or with a null mean: a plain norm): the norm's renorm state, the renorm form of the kernel
inline void launch_fwd_finish(const Geom &g, const double *partial, const float *weight, const float *bias, float eps,
                              float *mean, float *var, float *rstd, float *scale, float *shift, float *count,
                              Running run, const Renorm *rn = nullptr) {
    const dim3 grid((g.C + FIN_COLS - 1) / FIN_COLS), block(FIN_COLS * FIN_GROUPS);
    if (rn && rn->mean)
        hipLaunchKernelGGL(rowbn_fwd_finish_renorm_kernel, grid, block, 0, g.st, partial, g.nb, g.C, g.M, weight, bias, eps,
                           mean, var, rstd, scale, shift, g.mask, g.n_rois, g.per, g.mask ? count : nullptr, run, *rn);
    else
        hipLaunchKernelGGL(rowbn_fwd_finish_kernel, grid, block, 0, g.st, partial, g.nb, g.C, g.M, weight, bias, eps, mean,
                           var, rstd, scale, shift, g.mask, g.n_rois, g.per, g.mask ? count : nullptr, run);
}

// the same into a statistic block: [5, C] = mean, var, rstd, scale, shift (the layout of the Python binding), or with
// rn [7, C], r and d after them
inline void launch_fwd_finish(const Geom &g, const double *partial, const float *weight, const float *bias, float eps,
                              float *stats, float *count, Running run, const Renorm *rn = nullptr) {
    const int C = g.C;
    Renorm block;
    if (rn && rn->mean) {
        block = *rn;
        block.r = stats + 5 * C;
        block.d = stats + 6 * C;
        rn = &block;
    }
    launch_fwd_finish(g, partial, weight, bias, eps, stats, stats + C, stats + 2 * C, stats + 3 * C, stats + 4 * C, count,
                      run, rn);
}

// r, d (both or neither): the forward's renorm factors of the norm, the renorm form of the kernel
inline void launch_bwd_finish(const Geom &g, const double *partial, const float *weight, const float *mean,
                              const float *rstd, float *dweight, float *dbias, float *coef, const float *r = nullptr,
                              const float *d = nullptr) {
    const dim3 grid((g.C + FIN_COLS - 1) / FIN_COLS), block(FIN_COLS * FIN_GROUPS);
    if (r)
        hipLaunchKernelGGL(rowbn_bwd_finish_renorm_kernel, grid, block, 0, g.st, partial, g.nb, g.C, g.M, weight, mean, rstd,
                           dweight, dbias, coef, g.mask, g.n_rois, g.per, r, d);
    else
        hipLaunchKernelGGL(rowbn_bwd_finish_kernel, grid, block, 0, g.st, partial, g.nb, g.C, g.M, weight, mean, rstd,
                           dweight, dbias, coef, g.mask, g.n_rois, g.per);
}

// er: block 1's entry form (relu, roi-major rows): the sampled rows go to er->ys as well
inline void launch_apply_fwd(const Geom &g, const float *x, const float *scale, const float *shift, bool relu, float *y,
                             const EntryRows *er = nullptr) {
    if (er) {
        pick<0, 1>(g.mode, [&](auto MASK) {
            hipLaunchKernelGGL((rowbn_apply_fwd_kernel<true, MASK, true>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st,
                               x, scale, shift, g.total4, g.C / 4, y, g.mask, g.div, *er);
        });
        return;
    }
    pick<false, true>(relu, [&](auto RELU) {
        pick<0, 1, 2>(g.mode, [&](auto MASK) {
            hipLaunchKernelGGL((rowbn_apply_fwd_kernel<RELU, MASK>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, x,
                               scale, shift, g.total4, g.C / 4, y, g.mask, g.div);
        });
    });
}

inline void launch_apply_bwd(const Geom &g, const float *x, const float *dy, const float *scale, const float *shift,
                             const float *coef, bool relu, const EntryGrad *eg, float *dx) {
    if (eg)
        pick<0, 1>(g.mode, [&](auto MASK) {
            hipLaunchKernelGGL((rowbn_apply_bwd_kernel<true, MASK, true>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st,
                               x, dy, scale, shift, coef, g.total4, g.C / 4, dx, g.mask, g.div, *eg);
        });
    else
        pick<false, true>(relu, [&](auto RELU) {
            pick<0, 1, 2>(g.mode, [&](auto MASK) {
                hipLaunchKernelGGL((rowbn_apply_bwd_kernel<RELU, MASK>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st,
                                   x, dy, scale, shift, coef, g.total4, g.C / 4, dx, g.mask, g.div);
            });
        });
}

// feat [R, C] = the mean over the slots of x [n_slots * R, C], of relu(x*scale + shift) when scale is given; mask [R]
// or null
inline void launch_slot_mean(hipStream_t st, const float *x, const float *scale, const float *shift, int n_slots, int R,
                             int C, const float *mask, float *feat) {
    pick<false, true>(scale != nullptr, [&](auto NORM) {
        pick<false, true>(mask != nullptr, [&](auto MASKED) {
            hipLaunchKernelGGL((rowbn_slot_mean_kernel<NORM, MASKED ? 2 : 0>), dim3(apply_grid((long long)R * (C / 4))),
                               dim3(BLOCK), 0, st, x, scale, shift, n_slots, R, C / 4, feat, mask);
        });
    });
}

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : 3; }

// the backward of one layer; eg: dy comes in the two parts of block 1's entry gradient (relu, roi-major rows)
// r, d: the forward's renorm factors (both or neither)
int backward_impl(const Geom &g, const float *x, const float *dy, const EntryGrad *eg, const float *weight,
                  const float *mean, const float *rstd, const float *scale, const float *shift, bool relu, float *dx,
                  float *dweight, float *dbias, float *coef, const float *r = nullptr, const float *d = nullptr) {
    if ((r != nullptr) != (d != nullptr)) return 1;
    launch_grad_sums(g, x, dy, scale, shift, relu, eg, g.p0);
    launch_bwd_finish(g, g.p0, weight, mean, rstd, dweight, dbias, coef, r, d);
    launch_apply_bwd(g, x, dy, scale, shift, coef, relu, eg, dx);
    return launched();
}

// the renorm state of a single-norm entry point from its arguments; complete, or the call is rejected
struct RenormArgs {
    Renorm rn;
    bool ok;
    RenormArgs(float *mean, float *stddev, float *weight, double momentum, float *r, float *d)
        : rn{mean, stddev, weight, momentum, r, d}, ok(mean && stddev && weight && r && d) {}
};

// the forward of one layer: sums, finish and, with y, the apply pass (er: block 1's entry form).  rn: the layer's
// renorm state, or null for a plain norm.
int forward_impl(const Geom &g, const float *x, const float *weight, const float *bias, float eps, bool relu, float *y,
                 const EntryRows *er, float *mean, float *var, float *rstd, float *scale, float *shift, float *count,
                 Running run, const Renorm *rn = nullptr) {
    launch_sums(g, x, g.p0);
    launch_fwd_finish(g, g.p0, weight, bias, eps, mean, var, rstd, scale, shift, count, run, rn);
    if (y) launch_apply_fwd(g, x, scale, shift, relu, y, er);
    return launched();
}

}  // namespace

// y = act(batch_norm(x)); writes mean, var (biased), rstd, scale = rstd*weight, shift = bias - mean*scale (all [C]).
// Returns 0 on success, 1 for arguments it rejects (before any launch).
// mask (null: every row live): [n_rois] f32, 0 = dead; M = n_rois * per and row r belongs to RoI r / per or, with
// pos_major, r % n_rois (pos_major needs a mask).  Statistics are taken over the live rows, dead rows of y are
// written as zeros, and count[0] (required with a mask, untouched without) receives the number of live rows (>= 1)
// as a float.
// running_mean / running_var (f32 [C]) and num_batches_tracked (int64 [1]) are the layer's buffers, updated in place
// with `momentum` (struct Running); each may be null.
PLUMB_API int wsplumb_rowbn_forward(const float *x, long long M, int C, const float *weight, const float *bias,
                                    float eps, int relu, const float *mask, int n_rois, int per, int pos_major,
                                    float *y, float *mean, float *var, float *rstd, float *scale, float *shift,
                                    float *count, void *workspace, size_t workspace_bytes, void *stream,
                                    float *running_mean, float *running_var, float momentum,
                                    long long *num_batches_tracked) {
    Geom g;
    if (make_geom(g, M, C, mask, n_rois, per, pos_major != 0, false, !mask || count, workspace, workspace_bytes, 1,
                  stream))
        return 1;
    return forward_impl(g, x, weight, bias, eps, relu != 0, y, nullptr, mean, var, rstd, scale, shift, count,
                        Running{running_mean, running_var, momentum, num_batches_tracked});
}

// wsplumb_rowbn_forward of a batch renormalisation layer (struct Renorm): renorm_mean / renorm_stddev / renorm_weight
// (f32 [C], the layer's state, updated in place), renorm_momentum (a double: struct Renorm), and r, d (f32 [C], written: the step's correction
// factors, which the backward takes).  scale and shift are the renorm layer's; the running statistics follow the
// renorm state.  Everything else as wsplumb_rowbn_forward.
PLUMB_API int wsplumb_rowbn_forward_renorm(const float *x, long long M, int C, const float *weight, const float *bias,
                                           float eps, int relu, const float *mask, int n_rois, int per, int pos_major,
                                           float *y, float *mean, float *var, float *rstd, float *scale, float *shift,
                                           float *count, void *workspace, size_t workspace_bytes, void *stream,
                                           float *running_mean, float *running_var, float momentum,
                                           long long *num_batches_tracked, float *renorm_mean, float *renorm_stddev,
                                           float *renorm_weight, double renorm_momentum, float *r, float *d) {
    Geom g;
    const RenormArgs ra(renorm_mean, renorm_stddev, renorm_weight, renorm_momentum, r, d);
    if (make_geom(g, M, C, mask, n_rois, per, pos_major != 0, false, ra.ok && y && (!mask || count), workspace,
                  workspace_bytes, 1, stream))
        return 1;
    return forward_impl(g, x, weight, bias, eps, relu != 0, y, nullptr, mean, var, rstd, scale, shift, count,
                        Running{running_mean, running_var, momentum, num_batches_tracked}, &ra.rn);
}

// wsplumb_rowbn_forward without its apply pass: the statistics (and the running statistics) of the layer, for a
// consumer that applies scale / shift itself while it reads x (the patch gather of taps.hip).  Same arguments minus
// relu and y, same values.
PLUMB_API int wsplumb_rowbn_stats(const float *x, long long M, int C, const float *weight, const float *bias, float eps,
                                  const float *mask, int n_rois, int per, int pos_major, float *mean, float *var,
                                  float *rstd, float *scale, float *shift, float *count, void *workspace,
                                  size_t workspace_bytes, void *stream, float *running_mean, float *running_var,
                                  float momentum, long long *num_batches_tracked) {
    Geom g;
    if (make_geom(g, M, C, mask, n_rois, per, pos_major != 0, false, !mask || count, workspace, workspace_bytes, 1,
                  stream))
        return 1;
    return forward_impl(g, x, weight, bias, eps, false, nullptr, nullptr, mean, var, rstd, scale, shift, count,
                        Running{running_mean, running_var, momentum, num_batches_tracked});
}

// wsplumb_rowbn_stats of a batch renormalisation layer (the renorm arguments of wsplumb_rowbn_forward_renorm)
PLUMB_API int wsplumb_rowbn_stats_renorm(const float *x, long long M, int C, const float *weight, const float *bias,
                                         float eps, const float *mask, int n_rois, int per, int pos_major, float *mean,
                                         float *var, float *rstd, float *scale, float *shift, float *count,
                                         void *workspace, size_t workspace_bytes, void *stream, float *running_mean,
                                         float *running_var, float momentum, long long *num_batches_tracked,
                                         float *renorm_mean, float *renorm_stddev, float *renorm_weight,
                                         double renorm_momentum, float *r, float *d) {
    Geom g;
    const RenormArgs ra(renorm_mean, renorm_stddev, renorm_weight, renorm_momentum, r, d);
    if (make_geom(g, M, C, mask, n_rois, per, pos_major != 0, false, ra.ok && (!mask || count), workspace,
                  workspace_bytes, 1, stream))
        return 1;
    return forward_impl(g, x, weight, bias, eps, false, nullptr, nullptr, mean, var, rstd, scale, shift, count,
                        Running{running_mean, running_var, momentum, num_batches_tracked}, &ra.rn);
}

// wsplumb_rowbn_forward with ReLU for block 1's pre-activation norm (roi-major rows, n_rois groups of `per`; mask may
// be null): besides y it writes ys [n_slots * n_rois, C], the position-major rows of the positions the projection
// shortcut samples -- ys[possel[p] * n_rois + roi] = y[roi * per + p] for the p with possel[p] >= 0, possel [per]
// (device) being the table of wsplumb_rowbn_backward_entry, every slot 0 .. n_slots - 1 named by exactly one position.
// ys is a copy made in the apply pass, bit-identical to selecting the rows from y.
PLUMB_API int wsplumb_rowbn_forward_entry(const float *x, long long M, int C, const float *weight, const float *bias,
                                          float eps, const float *mask, int n_rois, int per, const int *possel,
                                          int n_slots, float *y, float *ys, float *mean, float *var, float *rstd,
                                          float *scale, float *shift, float *count, void *workspace,
                                          size_t workspace_bytes, void *stream, float *running_mean,
                                          float *running_var, float momentum, long long *num_batches_tracked) {
    Geom g;
    if (make_geom(g, M, C, mask, n_rois, per, false, true,
                  (!mask || count) && ys && possel && n_slots >= 1 && n_slots <= per, workspace, workspace_bytes, 1, stream))
        return 1;
    const EntryRows er = {ys, possel, per, n_rois};
    return forward_impl(g, x, weight, bias, eps, true, y, &er, mean, var, rstd, scale, shift, count,
                        Running{running_mean, running_var, momentum, num_batches_tracked});
}

// wsplumb_rowbn_forward_entry of a batch renormalisation layer (the renorm arguments of wsplumb_rowbn_forward_renorm)
PLUMB_API int wsplumb_rowbn_forward_entry_renorm(const float *x, long long M, int C, const float *weight,
                                                 const float *bias, float eps, const float *mask, int n_rois, int per,
                                                 const int *possel, int n_slots, float *y, float *ys, float *mean,
                                                 float *var, float *rstd, float *scale, float *shift, float *count,
                                                 void *workspace, size_t workspace_bytes, void *stream,
                                                 float *running_mean, float *running_var, float momentum,
                                                 long long *num_batches_tracked, float *renorm_mean,
                                                 float *renorm_stddev, float *renorm_weight, double renorm_momentum,
                                                 float *r, float *d) {
    Geom g;
    const RenormArgs ra(renorm_mean, renorm_stddev, renorm_weight, renorm_momentum, r, d);
    if (make_geom(g, M, C, mask, n_rois, per, false, true,
                  ra.ok && y && (!mask || count) && ys && possel && n_slots >= 1 && n_slots <= per, workspace,
                  workspace_bytes, 1, stream))
        return 1;
    const EntryRows er = {ys, possel, per, n_rois};
    return forward_impl(g, x, weight, bias, eps, true, y, &er, mean, var, rstd, scale, shift, count,
                        Running{running_mean, running_var, momentum, num_batches_tracked}, &ra.rn);
}

// feat [R, C] = the mean over the slots of the position-major rows x [n_slots * R, C] (row slot * R + roi), in the one
// order of bn_math.hip.h that the exit form of wsplumb_rowbn_join_forward uses as well.
PLUMB_API int wsplumb_slot_mean(const float *x, int n_slots, int R, int C, float *feat, void *stream) {
    if (n_slots < 1 || R < 1 || C < 4 || (C & 3) || (long long)n_slots * R > 0x7fffffffLL) return 1;
    launch_slot_mean(static_cast<hipStream_t>(stream), x, nullptr, nullptr, n_slots, R, C, nullptr, feat);
    return launched();
}

// y = act(x*scale + shift) with given per-column scale / shift (inference statistics)
PLUMB_API int wsplumb_rowbn_apply(const float *x, long long M, int C, const float *scale,
                                  const float *shift, int relu, float *y, void *stream) {
    Geom g;
    if (make_geom(g, M, C, nullptr, 0, 1, false, false, true, nullptr, 0, 0, stream)) return 1;
    launch_apply_fwd(g, x, scale, shift, relu != 0, y);
    return launched();
}

// gradients of wsplumb_rowbn_forward (same mask arguments; dead rows: dy ignored, dx = 0): dx [M,C], dweight [C],
// dbias [C]; coef is [3*C] scratch
PLUMB_API int wsplumb_rowbn_backward(const float *x, const float *dy, long long M, int C, const float *weight,
                                     const float *mean, const float *rstd, const float *scale, const float *shift,
                                     int relu, const float *mask, int n_rois, int per, int pos_major, float *dx,
                                     float *dweight, float *dbias, float *coef, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    Geom g;
    if (make_geom(g, M, C, mask, n_rois, per, pos_major != 0, false, true, workspace, workspace_bytes, 1, stream))
        return 1;
    return backward_impl(g, x, dy, nullptr, weight, mean, rstd, scale, shift, relu != 0, dx, dweight, dbias, coef);
}

// gradients of wsplumb_rowbn_forward_renorm: r, d (f32 [C]) are the factors that call wrote, constants of the
// backward (bwd_finish); scale and shift are the renorm layer's.  Everything else as wsplumb_rowbn_backward.
PLUMB_API int wsplumb_rowbn_backward_renorm(const float *x, const float *dy, long long M, int C, const float *weight,
                                            const float *mean, const float *rstd, const float *scale,
                                            const float *shift, int relu, const float *mask, int n_rois, int per,
                                            int pos_major, float *dx, float *dweight, float *dbias, float *coef,
                                            void *workspace, size_t workspace_bytes, void *stream, const float *r,
                                            const float *d) {
    Geom g;
    if (make_geom(g, M, C, mask, n_rois, per, pos_major != 0, false, r && d, workspace, workspace_bytes, 1, stream))
        return 1;
    return backward_impl(g, x, dy, nullptr, weight, mean, rstd, scale, shift, relu != 0, dx, dweight, dbias, coef, r, d);
}

// gradients of wsplumb_rowbn_forward with ReLU for block 1's pre-activation norm (roi-major rows), the output's
// gradient given in its two parts (EntryGrad above): dy [n_rois * per, C] roi-major from conv1, dys
// [n_slots * n_rois, C] position-major from the projection shortcut, possel [per] (device) the slot of each position
// or -1.  mask may be null.  Bit-identical to wsplumb_rowbn_backward on dy + scatter(dys).
PLUMB_API int wsplumb_rowbn_backward_entry(const float *x, const float *dy, const float *dys, const int *possel,
                                           int n_slots, long long M, int C, const float *weight, const float *mean,
                                           const float *rstd, const float *scale, const float *shift,
                                           const float *mask, int n_rois, int per, float *dx, float *dweight,
                                           float *dbias, float *coef, void *workspace, size_t workspace_bytes,
                                           void *stream) {
    Geom g;
    if (make_geom(g, M, C, mask, n_rois, per, false, true, dys && possel && n_slots >= 1 && n_slots <= per, workspace,
                  workspace_bytes, 1, stream))
        return 1;
    const EntryGrad eg = {dys, possel, per, n_rois, 0.0f};
    return backward_impl(g, x, dy, &eg, weight, mean, rstd, scale, shift, true, dx, dweight, dbias, coef);
}

// gradients of wsplumb_rowbn_forward_entry_renorm (r, d as in wsplumb_rowbn_backward_renorm)
PLUMB_API int wsplumb_rowbn_backward_entry_renorm(const float *x, const float *dy, const float *dys, const int *possel,
                                                  int n_slots, long long M, int C, const float *weight,
                                                  const float *mean, const float *rstd, const float *scale,
                                                  const float *shift, const float *mask, int n_rois, int per,
                                                  float *dx, float *dweight, float *dbias, float *coef, void *workspace,
                                                  size_t workspace_bytes, void *stream, const float *r, const float *d) {
    Geom g;
    if (make_geom(g, M, C, mask, n_rois, per, false, true, r && d && dys && possel && n_slots >= 1 && n_slots <= per,
                  workspace, workspace_bytes, 1, stream))
        return 1;
    const EntryGrad eg = {dys, possel, per, n_rois, 0.0f};
    return backward_impl(g, x, dy, &eg, weight, mean, rstd, scale, shift, true, dx, dweight, dbias, coef, r, d);
}

// ---- residual joins (position-major rows; mask may be null: every row live) ----
// Statistic blocks are [5, C] f32: mean, var, rstd, scale, shift (the layout of the Python binding).

namespace {

// exit_slots = 0: y [M, C] is written.  exit_slots = n_slots > 0 (the head's exit): y is feat [M / n_slots, C], the
// mean over the slots of what y would hold, which is then never written.
int join_forward_impl(const float *x3, const float *other, long long M, int C, const float *weight3, const float *bias3,
                      float eps3, const float *weight_s, const float *bias_s, float eps_s, const float *weight_n,
                      const float *bias_n, float eps_n, const float *mask, int n_rois, int per, float *out, float *y,
                      float *stats3, float *stats_s, float *stats_n, float *count, void *workspace,
                      size_t workspace_bytes, void *stream, float *const *running, const float *momentum,
                      long long *const *batches, int exit_slots, float *const *renorm = nullptr,
                      const double *renorm_momentum = nullptr) {
    const bool dual = weight_s != nullptr;
    Geom g;
    const bool exit_ok = exit_slots == 0 || (exit_slots > 0 && M % exit_slots == 0 && M <= 0x7fffffffLL &&
                                             (!mask || (per == exit_slots && (long long)n_rois * per == M)));
    if (make_geom(g, M, C, mask, n_rois, per, mask != nullptr, false,
                  exit_ok && (!mask || count) && (!dual || (bias_s && stats_s)), workspace, workspace_bytes, 2, stream))
        return 1;
    Running run[3] = {};
    Renorm rn[3] = {};          // per norm: its renorm state, or none (mean null: a plain norm, a [5, C] block)
    for (int k = 0; k < 3; ++k) {
        if (running) { run[k].mean = running[2 * k]; run[k].var = running[2 * k + 1]; }
        if (momentum) run[k].momentum = momentum[k];
        if (batches) run[k].batches = batches[k];
        if (renorm && renorm[3 * k]) {
            if (!renorm[3 * k + 1] || !renorm[3 * k + 2] || !renorm_momentum) return 1;
            rn[k] = Renorm{renorm[3 * k], renorm[3 * k + 1], renorm[3 * k + 2], renorm_momentum[k], nullptr, nullptr};
        }
    }
    launch_sums(g, x3, g.p0);
    launch_fwd_finish(g, g.p0, weight3, bias3, eps3, stats3, nullptr, run[0], &rn[0]);
    if (dual) {
        launch_sums(g, other, g.p0);
        launch_fwd_finish(g, g.p0, weight_s, bias_s, eps_s, stats_s, nullptr, run[1], &rn[1]);
    }
    const float *sco = dual ? stats_s + 3 * C : nullptr, *sho = dual ? stats_s + 4 * C : nullptr;
    pick<false, true>(dual, [&](auto DUAL) {
        pick<0, 2>(g.mode, [&](auto MASK) {
            hipLaunchKernelGGL((rowbn_join_fwd_kernel<DUAL, MASK>), dim3(g.nb), dim3(BLOCK), 0, g.st, x3, stats3 + 3 * C,
                               stats3 + 4 * C, other, sco, sho, M, C, g.rpb, out, g.p0, mask, g.div);
        });
    });
    launch_fwd_finish(g, g.p0, weight_n, bias_n, eps_n, stats_n, count, run[2], &rn[2]);
    if (exit_slots)
        launch_slot_mean(g.st, out, stats_n + 3 * C, stats_n + 4 * C, exit_slots, (int)(M / exit_slots), C, mask, y);
    else
        launch_apply_fwd(g, out, stats_n + 3 * C, stats_n + 4 * C, true, y);
    return launched();
}

}  // namespace

// out = bn3(x3) + other, y = relu(bn_n(out)), all in training mode over the live rows:
//   other is the identity shortcut when weight_s is null, else the input xs of the shortcut's own norm
//   (out = bn3(x3) + bn_s(xs); stats_s is written only then);
//   stats3 / stats_s / stats_n [5, C] and count [1] are what wsplumb_rowbn_forward (pos_major) writes for the
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
    return join_forward_impl(x3, other, M, C, weight3, bias3, eps3, weight_s, bias_s, eps_s, weight_n, bias_n, eps_n, mask,
                             n_rois, per, out, y, stats3, stats_s, stats_n, count, workspace, workspace_bytes, stream,
                             running, momentum, batches, 0);
}

// The exit form of wsplumb_rowbn_join_forward, for the last join of the head, whose y = relu(bn_n(out)) is only ever
// averaged over the n_slots positions of each RoI (M = n_slots * R rows, row slot * R + roi; with a mask n_rois = R and
// per = n_slots): instead of y it writes feat [R, C], feat[roi] = mean over the slots of y[slot * R + roi] in the order
// of bn_math.hip.h (wsplumb_slot_mean of the y the plain form writes, bit for bit), zero for a dead RoI.  Everything
// else as the plain form.
PLUMB_API int wsplumb_rowbn_join_forward_exit(const float *x3, const float *other, long long M, int C,
                                              const float *weight3, const float *bias3, float eps3,
                                              const float *weight_s, const float *bias_s, float eps_s,
                                              const float *weight_n, const float *bias_n, float eps_n,
                                              const float *mask, int n_rois, int per, float *out, float *feat,
                                              float *stats3, float *stats_s, float *stats_n, float *count,
                                              void *workspace, size_t workspace_bytes, void *stream,
                                              float *const *running, const float *momentum,
                                              long long *const *batches, int n_slots) {
    if (n_slots < 1) return 1;
    return join_forward_impl(x3, other, M, C, weight3, bias3, eps3, weight_s, bias_s, eps_s, weight_n, bias_n, eps_n, mask,
                             n_rois, per, out, feat, stats3, stats_s, stats_n, count, workspace, workspace_bytes, stream,
                             running, momentum, batches, n_slots);
}

// wsplumb_rowbn_join_forward (n_slots = 0) or its exit form (n_slots >= 1) with batch renormalisation layers:
// renorm [9] (host array) holds the renorm_mean, renorm_stddev, renorm_weight pointers of bn3, bn_s, bn_n in that
// order and renorm_momentum [3] their factors (struct Renorm); a norm whose first pointer is null is a plain norm.
// The statistic block of a renorm norm is [7, C]: r and d after the five rows (wsplumb_rowbn_join_backward_renorm
// reads them); scale and shift are the renorm layer's, so the join, apply and exit kernels run unchanged.
PLUMB_API int wsplumb_rowbn_join_forward_renorm(const float *x3, const float *other, long long M, int C,
                                                const float *weight3, const float *bias3, float eps3,
                                                const float *weight_s, const float *bias_s, float eps_s,
                                                const float *weight_n, const float *bias_n, float eps_n,
                                                const float *mask, int n_rois, int per, float *out, float *y,
                                                float *stats3, float *stats_s, float *stats_n, float *count,
                                                void *workspace, size_t workspace_bytes, void *stream,
                                                float *const *running, const float *momentum,
                                                long long *const *batches, int n_slots, float *const *renorm,
                                                const double *renorm_momentum) {
    if (n_slots < 0 || !renorm) return 1;
    return join_forward_impl(x3, other, M, C, weight3, bias3, eps3, weight_s, bias_s, eps_s, weight_n, bias_n, eps_n, mask,
                             n_rois, per, out, y, stats3, stats_s, stats_n, count, workspace, workspace_bytes, stream,
                             running, momentum, batches, n_slots, renorm, renorm_momentum);
}

namespace {

// exit_slots = n_slots > 0: dy is dfeat [M / n_slots, C] of the forward's exit form, and there is no dres
int join_backward_impl(const float *out, const float *dy, const float *dres, const float *x3, const float *xs, long long M,
                       int C, const float *weight_n, const float *stats_n, const float *weight3, const float *stats3,
                       const float *weight_s, const float *stats_s, const float *mask, int n_rois, int per, float *gout,
                       float *dx3, float *dxs, float *dwb_n, float *dwb3, float *dwb_s, float *coef, void *workspace,
                       size_t workspace_bytes, void *stream, int exit_slots, int renorm = 0) {
    const bool dual = xs != nullptr;
    Geom g;
    const bool exit_ok = exit_slots == 0 || (exit_slots > 0 && !dres && M % exit_slots == 0 && M <= 0x7fffffffLL &&
                                             (!mask || (per == exit_slots && (long long)n_rois * per == M)));
    if (make_geom(g, M, C, mask, n_rois, per, mask != nullptr, false,
                  exit_ok && (!dual || (weight_s && stats_s && dxs && dwb_s)), workspace, workspace_bytes, 2, stream))
        return 1;
    float *coef_n = coef, *coef3 = coef + 3 * C, *coefs = coef + 6 * C;
    const float *scn = stats_n + 3 * C, *shn = stats_n + 4 * C;
    // r, d of a norm the renorm bits name (1: bn3, 2: bn_s, 4: bn_n), rows 5 and 6 of its [7, C] block
    auto rd = [&](int bit, const float *stats, int row) { return (renorm & bit) ? stats + row * C : nullptr; };
    if (exit_slots) {
        const EntryGrad eg = {nullptr, nullptr, exit_slots, (int)(M / exit_slots), slot_mean_scale(exit_slots)};
        launch_grad_sums(g, out, dy, scn, shn, true, &eg, g.p0, true);
        launch_bwd_finish(g, g.p0, weight_n, stats_n, stats_n + 2 * C, dwb_n, dwb_n + C, coef_n, rd(4, stats_n, 5),
                          rd(4, stats_n, 6));
        pick<false, true>(dual, [&](auto DUAL) {
            pick<0, 2>(g.mode, [&](auto MASK) {
                hipLaunchKernelGGL((rowbn_join_bwd_kernel<DUAL, false, MASK, DY_EXIT>), dim3(g.nb), dim3(BLOCK), 0, g.st, out,
                                   dy, scn, shn, coef_n, nullptr, x3, xs, M, C, g.rpb, gout, g.p0, g.p1, mask, g.div, eg);
            });
        });
    } else {
        launch_grad_sums(g, out, dy, scn, shn, true, nullptr, g.p0);
        launch_bwd_finish(g, g.p0, weight_n, stats_n, stats_n + 2 * C, dwb_n, dwb_n + C, coef_n, rd(4, stats_n, 5),
                          rd(4, stats_n, 6));
        pick<false, true>(dual, [&](auto DUAL) {
            pick<false, true>(dres != nullptr, [&](auto RES) {
                pick<0, 2>(g.mode, [&](auto MASK) {
                    hipLaunchKernelGGL((rowbn_join_bwd_kernel<DUAL, RES, MASK>), dim3(g.nb), dim3(BLOCK), 0, g.st, out, dy,
                                       scn, shn, coef_n, dres, x3, xs, M, C, g.rpb, gout, g.p0, g.p1, mask, g.div);
                });
            });
        });
    }
    launch_bwd_finish(g, g.p0, weight3, stats3, stats3 + 2 * C, dwb3, dwb3 + C, coef3, rd(1, stats3, 5), rd(1, stats3, 6));
    if (dual) {
        launch_bwd_finish(g, g.p1, weight_s, stats_s, stats_s + 2 * C, dwb_s, dwb_s + C, coefs, rd(2, stats_s, 5),
                          rd(2, stats_s, 6));
        pick<0, 2>(g.mode, [&](auto MASK) {
            hipLaunchKernelGGL((rowbn_apply_bwd_dual_kernel<MASK>), dim3(apply_grid(g.total4)), dim3(BLOCK), 0, g.st, x3, xs,
                               gout, coef3, coefs, g.total4, C / 4, dx3, dxs, mask, g.div);
        });
    } else {
        launch_apply_bwd(g, x3, gout, nullptr, nullptr, coef3, false, nullptr, dx3);
    }
    return launched();
}

}  // namespace

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
    return join_backward_impl(out, dy, dres, x3, xs, M, C, weight_n, stats_n, weight3, stats3, weight_s, stats_s, mask,
                              n_rois, per, gout, dx3, dxs, dwb_n, dwb3, dwb_s, coef, workspace, workspace_bytes, stream, 0);
}

// gradients of wsplumb_rowbn_join_forward_exit: dfeat [M / n_slots, C] is the gradient of feat; the gradient of the y
// that was never written, dfeat[r % R] * (1 / n_slots), is formed in registers by the two kernels that read it (DY_EXIT).
// There is no dres.  Everything else as wsplumb_rowbn_join_backward, and bit-identical to it fed with that gradient
// expanded to [M, C] (1 / n_slots is exact for a power of two, which makes it torch's mean backward as well).
PLUMB_API int wsplumb_rowbn_join_backward_exit(const float *out, const float *dfeat, int n_slots, const float *x3,
                                               const float *xs, long long M, int C, const float *weight_n,
                                               const float *stats_n, const float *weight3, const float *stats3,
                                               const float *weight_s, const float *stats_s, const float *mask,
                                               int n_rois, int per, float *gout, float *dx3, float *dxs, float *dwb_n,
                                               float *dwb3, float *dwb_s, float *coef, void *workspace,
                                               size_t workspace_bytes, void *stream) {
    if (n_slots < 1) return 1;
    return join_backward_impl(out, dfeat, nullptr, x3, xs, M, C, weight_n, stats_n, weight3, stats3, weight_s, stats_s,
                              mask, n_rois, per, gout, dx3, dxs, dwb_n, dwb3, dwb_s, coef, workspace, workspace_bytes,
                              stream, n_slots);
}

// gradients of wsplumb_rowbn_join_forward_renorm (n_slots = 0: dy is y's gradient; n_slots >= 1, the exit form: dy is
// dfeat and there is no dres).  renorm: bit 0 / 1 / 2 set when bn3 / bn_s / bn_n is a renorm norm, whose [7, C]
// statistic block then carries the forward's r and d in rows 5 and 6.
PLUMB_API int wsplumb_rowbn_join_backward_renorm(const float *out, const float *dy, const float *dres, int n_slots,
                                                 const float *x3, const float *xs, long long M, int C,
                                                 const float *weight_n, const float *stats_n, const float *weight3,
                                                 const float *stats3, const float *weight_s, const float *stats_s,
                                                 const float *mask, int n_rois, int per, float *gout, float *dx3,
                                                 float *dxs, float *dwb_n, float *dwb3, float *dwb_s, float *coef,
                                                 void *workspace, size_t workspace_bytes, void *stream, int renorm) {
    if (n_slots < 0 || renorm < 0 || renorm > 7) return 1;
    return join_backward_impl(out, dy, dres, x3, xs, M, C, weight_n, stats_n, weight3, stats3, weight_s, stats_s, mask,
                              n_rois, per, gout, dx3, dxs, dwb_n, dwb3, dwb_s, coef, workspace, workspace_bytes, stream,
                              n_slots, renorm);
}
