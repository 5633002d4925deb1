// Group normalisation (+ReLU) over the row-matrix view both networks use: x is [M, C] f32 with M = S * P, S samples
// of P rows each (the trunk: a sample is an image, P = H*W; the per-RoI head: a sample is one RoI, P = 49 or 16).
// Part of the plumbing library, like rowbn.hip; reached through networks/_plumbing.py (groupnorm_forward / _backward).
//
// WHAT IS COMPUTED (the reference project's group_norm, not torch.nn.GroupNorm): G = 8 INTERLEAVED groups -- channel
// c belongs to group c % G -- and per (sample, group) one mean and one biased variance over its P * C/G values;
//   y  = act((x - mean) * rstd * gamma[c] + beta[c]),   rstd = 1 / sqrt(var + eps)
//   g  = dy * gate (gate = y > 0, recomputed from x),   xhat = (x - mean) * rstd
//   A  = mean(g * gamma), B = mean(g * gamma * xhat)    per (sample, group)
//   dx = rstd * (g * gamma - A - xhat * B),   dgamma[c] = sum g * xhat,   dbeta[c] = sum g   over all live samples
// Every sum is f64 and taken in a fixed order (no atomics): two runs give the same bits.
//
// ROWS.  Row (s, p) is row s * ss + p * ps of the matrix: sample-major (ss = P, ps = 1: the trunk's [N*H*W, C] view,
// the head's roi-major rows) or position-major (ss = 1, ps = S: the head's 4x4 section).  One kernel set takes both.
//
// LIVE-SAMPLE MASK ([S] f32, the head's RoI mask).  A dead sample's rows are not read, its y / dx rows are written as
// zeros, it adds nothing to dgamma / dbeta, and its mean / rstd come out as 0.
//
// LOADS AND GROUPS.  Threads read float4 columns.  With G = 8 the four channels of float4 column j are groups
// (j & 1) * 4 + 0..3, so a thread keeps four (sum, sum of squares) pairs and the block reduces across the threads of
// equal column parity.  A thread's columns are j = lc + cc * L with L even, so its parity never changes.
//
// TWO REGIMES, by the floats of one sample (GN_SMALL_MAX_FLOATS):
//  small  one workgroup of 512 threads owns a whole sample and loops over samples.  It sums the sample while keeping up
//         to GN_CACHE float4 per thread in registers, reduces, and applies from the registers; what does not fit (a
//         49 x 1024 sample is 200 KB) is read a second time, from cache.  In the backward the workgroup carries its
//         dgamma / dbeta sums in registers across all its samples and writes ONE [2, C] f64 partial at the end.
//  large  many workgroups per sample: f64 partial sums per (sample, chunk of rows, group), a finish kernel that forms
//         mean / rstd (backward: A / B), then an apply pass -- the partial / finish / apply of rowbn.hip with the
//         reduction running over a sample's rows and C/G channels.  The backward's partial pass also leaves a [2, C]
//         f64 partial per (sample, chunk).
// Either way one finish kernel reduces the [2, C] partials in slot order into dgamma / dbeta.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn_math.hip.h"

#define PLUMB_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int GN_G = 8;                             // the only group count of the fused kernels
constexpr int GN_MAX_C = 2048;                      // C/4 <= BLOCK_SMALL, and <= 2 column passes of BLOCK_LARGE
constexpr long long GN_SMALL_MAX_FLOATS = 65536;    // THE REGIME SWITCH: samples of up to 256 KB are 'small'
constexpr int GN_BLOCK_SMALL = 512;
constexpr int GN_BLOCK_LARGE = 256;
constexpr int GN_SMALL_MAX_WG = 1024;               // small regime: workgroups looping over the samples
constexpr int GN_CACHE = 16;                        // small forward: float4 kept per thread between the two sweeps
constexpr int GN_CACHE_BWD = 8;                     // small backward: float4 of x and of dy kept per thread
constexpr int GN_CHUNK_STEPS = 8;                   // large regime: row steps of a thread per chunk ...
constexpr int GN_MAX_CHUNKS = 128;                  // ... until the chunks of a sample hit this cap
constexpr int FIN_COLS = 32, FIN_SLICES = 8;        // the column finish: 32 columns x 8 slices of slots per block
constexpr int GFIN_SLICES = 16;                     // the group finish: 16 values x 16 slices of chunks per block

typedef float float4v __attribute__((ext_vector_type(4)));

// Thread t owns float4 columns lc + cc * L and the rows lr + k * RS of a sample (or of a chunk of its rows).
template <int BS>
struct Map {
    int C4, L, RS, lc, lr;
    bool on;
    __device__ __forceinline__ explicit Map(int C) {
        C4 = C >> 2;
        L = C4 < BS ? C4 : BS;
        RS = BS / L;
        lc = threadIdx.x % L;
        lr = threadIdx.x / L;
        on = lr < RS;
    }
};

struct Rows {
    long long ss, ps;       // row of (sample s, position p) = s * ss + p * ps
    int C;
    __device__ __forceinline__ size_t at(long long s, long long p) const { return (size_t)(s * ss + p * ps) * (size_t)C; }
};

__device__ __forceinline__ float4v ld4(const float *__restrict__ base, size_t row_off, int c4) {
    return reinterpret_cast<const float4v *>(base + row_off)[c4];
}
__device__ __forceinline__ void st4(float *__restrict__ base, size_t row_off, int c4, float4v v) {
    reinterpret_cast<float4v *>(base + row_off)[c4] = v;
}

// ---- the element arithmetic, one form for both regimes ----
// scale = rstd * gamma, shift = beta - mean * scale (one fused rounding), y = fma(x, scale, shift) (bn_affine)
__device__ __forceinline__ void gn_coef(float mean, float rstd, float ga, float be, float &sc, float &sh) {
    sc = rstd * ga;
    sh = __builtin_fmaf(-mean, sc, be);
}
// xhat = (x - mean) * rstd: two roundings
__device__ __forceinline__ float gn_xhat(float x, float mean, float rstd) {
    const float xc = x - mean;
    return xc * rstd;
}
// dx = rstd * (g * gamma - A - xhat * B): three roundings
__device__ __forceinline__ float gn_dx(float g, float ga, float A, float B, float xhat, float rstd) {
    const float t = __builtin_fmaf(g, ga, -A);
    return rstd * __builtin_fmaf(-xhat, B, t);
}
template <bool RELU>
__device__ __forceinline__ float gn_gated(float dy, float x, float sc, float sh) {
    return (!RELU || bn_affine(x, sc, sh) > 0.0f) ? dy : 0.0f;
}
__device__ __forceinline__ void acc_sq(double &s, double &q, float v) {
    s += (double)v;
    q = __builtin_fma((double)v, (double)v, q);
}

// a[0..3] / a[4..7]: this thread's two sums for the groups par * 4 + 0..3.  On return every thread holds the block's
// totals for its parity: a butterfly over the lanes of equal parity (lane distances 2 .. 32), then the waves in
// order.  red: [BS / 64][2][8].
template <int BS>
__device__ __forceinline__ void group_reduce(double (&a)[8], double (*red)[2][8]) {
    constexpr int NW = BS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off >= 2; off >>= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] += __shfl_xor(a[i], off, 64);
    __syncthreads();                                 // the previous use of red is over
    if (lane < 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[wave][lane][i] = a[i];
    }
    __syncthreads();
    const int par = lane & 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double t = red[0][par][i];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += red[w][par][i];
        a[i] = t;
    }
}

// mean / rstd of a group from its f64 sums: mean = s / n, var = max(q / n - mean^2, 0), each rounded to f32 once
__device__ __forceinline__ void gn_stats(double s, double q, double inv_n, double eps, float &mean, float &rstd) {
    const double mu = s * inv_n;
    double var = q * inv_n - mu * mu;
    var = var > 0.0 ? var : 0.0;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + eps));
}

// fixed-order sum over the RS row phases of this thread's column, through red [BS] doubles; the lr == 0 thread of
// the column returns the total
template <int BS>
__device__ __forceinline__ double col_reduce(const Map<BS> &m, double v, double *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    double t = 0.0;
    if (m.lr == 0)
        for (int k = 0; k < m.RS; ++k) t += red[k * m.L + m.lc];
    return t;
}

// ================================================================ small samples
template <bool RELU>
__global__ __launch_bounds__(GN_BLOCK_SMALL) void gn_small_fwd_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ mask, float *__restrict__ y, float *__restrict__ mean, float *__restrict__ rstd,
    long long S, int P, Rows R, float eps) {
    __shared__ double red[GN_BLOCK_SMALL / 64][2][8];
    const Map<GN_BLOCK_SMALL> m(R.C);
    const int par = m.lc & 1, RS = m.RS;
    const float4v zero4 = {0, 0, 0, 0};
    float4v ga = zero4, be = zero4;
    if (m.on) {
        ga = reinterpret_cast<const float4v *>(gamma)[m.lc];
        be = reinterpret_cast<const float4v *>(beta)[m.lc];
    }
    const double inv_n = 1.0 / ((double)P * (double)(R.C / GN_G));
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        if (mask && mask[s] == 0.0f) {               // block-uniform
            if (m.on)
                for (int p = m.lr; p < P; p += RS) st4(y, R.at(s, p), m.lc, zero4);
            if (threadIdx.x < GN_G) { mean[s * GN_G + threadIdx.x] = 0.0f; rstd[s * GN_G + threadIdx.x] = 0.0f; }
            continue;
        }
        float4v cache[GN_CACHE];
        double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const size_t base = R.at(s, m.lr), step = (size_t)(RS * R.ps) * (size_t)R.C;   // row lr + k * RS: base + k * step
        if (m.on) {
#pragma unroll
            for (int k = 0; k < GN_CACHE; ++k) {
                const int p = m.lr + k * RS;
                cache[k] = p < P ? ld4(x, base + k * step, m.lc) : zero4;
            }
#pragma unroll
            for (int k = 0; k < GN_CACHE; ++k) {
                if (m.lr + k * RS < P) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc_sq(a[j], a[4 + j], cache[k][j]);
                }
            }
            for (int p = m.lr + GN_CACHE * RS; p < P; p += RS) {
                const float4v v = ld4(x, R.at(s, p), m.lc);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc_sq(a[j], a[4 + j], v[j]);
            }
        }
        group_reduce<GN_BLOCK_SMALL>(a, red);
        float4v sc, sh;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mu, rs, c0, c1;
            gn_stats(a[j], a[4 + j], inv_n, (double)eps, mu, rs);
            if (threadIdx.x < 2) { mean[s * GN_G + par * 4 + j] = mu; rstd[s * GN_G + par * 4 + j] = rs; }
            gn_coef(mu, rs, ga[j], be[j], c0, c1);
            sc[j] = c0;
            sh[j] = c1;
        }
        if (m.on) {
#pragma unroll
            for (int k = 0; k < GN_CACHE; ++k) {
                const int p = m.lr + k * RS;
                if (p < P) {
                    float4v o;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        o[j] = RELU ? bn_affine_relu(cache[k][j], sc[j], sh[j]) : bn_affine(cache[k][j], sc[j], sh[j]);
                    st4(y, base + k * step, m.lc, o);
                }
            }
            for (int p = m.lr + GN_CACHE * RS; p < P; p += RS) {
                const size_t off = R.at(s, p);
                const float4v v = ld4(x, off, m.lc);
                float4v o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = RELU ? bn_affine_relu(v[j], sc[j], sh[j]) : bn_affine(v[j], sc[j], sh[j]);
                st4(y, off, m.lc, o);
            }
        }
    }
}

// part: [gridDim.x][2][C] f64, (sum g * xhat, sum g) of the samples this workgroup handled
template <bool RELU>
__global__ __launch_bounds__(GN_BLOCK_SMALL) void gn_small_bwd_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ rstd,
    const float *__restrict__ mask, float *__restrict__ dx, double *__restrict__ part, long long S, int P, Rows R) {
    __shared__ double red[GN_BLOCK_SMALL / 64][2][8];
    __shared__ double cred[GN_BLOCK_SMALL];
    const Map<GN_BLOCK_SMALL> m(R.C);
    const int par = m.lc & 1, RS = m.RS;
    const float4v zero4 = {0, 0, 0, 0};
    float4v ga = zero4, be = zero4;
    if (m.on) {
        ga = reinterpret_cast<const float4v *>(gamma)[m.lc];
        be = reinterpret_cast<const float4v *>(beta)[m.lc];
    }
    const double inv_n = 1.0 / ((double)P * (double)(R.C / GN_G));
    double dg[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0};       // carried across the samples
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        if (mask && mask[s] == 0.0f) {
            if (m.on)
                for (int p = m.lr; p < P; p += RS) st4(dx, R.at(s, p), m.lc, zero4);
            continue;
        }
        float4v mu, rs, sc, sh;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float c0, c1;
            mu[j] = mean[s * GN_G + par * 4 + j];
            rs[j] = rstd[s * GN_G + par * 4 + j];
            gn_coef(mu[j], rs[j], ga[j], be[j], c0, c1);
            sc[j] = c0;
            sh[j] = c1;
        }
        float4v cx[GN_CACHE_BWD], cg[GN_CACHE_BWD];
        double sg[4] = {0, 0, 0, 0}, sgx[4] = {0, 0, 0, 0};
        if (m.on) {
#pragma unroll
            for (int k = 0; k < GN_CACHE_BWD; ++k) {
                const int p = m.lr + k * RS;
                const bool in = p < P;
                const size_t off = in ? R.at(s, p) : 0;
                cx[k] = in ? ld4(x, off, m.lc) : zero4;
                cg[k] = in ? ld4(dy, off, m.lc) : zero4;
            }
#pragma unroll
            for (int k = 0; k < GN_CACHE_BWD; ++k) {
                if (m.lr + k * RS < P) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float g = gn_gated<RELU>(cg[k][j], cx[k][j], sc[j], sh[j]);
                        cg[k][j] = g;
                        sg[j] += (double)g;
                        sgx[j] = __builtin_fma((double)g, (double)gn_xhat(cx[k][j], mu[j], rs[j]), sgx[j]);
                    }
                }
            }
            for (int p = m.lr + GN_CACHE_BWD * RS; p < P; p += RS) {
                const size_t off = R.at(s, p);
                const float4v xv = ld4(x, off, m.lc), dv = ld4(dy, off, m.lc);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g = gn_gated<RELU>(dv[j], xv[j], sc[j], sh[j]);
                    sg[j] += (double)g;
                    sgx[j] = __builtin_fma((double)g, (double)gn_xhat(xv[j], mu[j], rs[j]), sgx[j]);
                }
            }
        }
        double a[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = (double)ga[j] * sg[j];
            a[4 + j] = (double)ga[j] * sgx[j];
            dg[j] += sgx[j];
            db[j] += sg[j];
        }
        group_reduce<GN_BLOCK_SMALL>(a, red);
        float4v A, B;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            A[j] = (float)(a[j] * inv_n);
            B[j] = (float)(a[4 + j] * inv_n);
        }
        if (m.on) {
#pragma unroll
            for (int k = 0; k < GN_CACHE_BWD; ++k) {
                const int p = m.lr + k * RS;
                if (p < P) {
                    float4v o;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        o[j] = gn_dx(cg[k][j], ga[j], A[j], B[j], gn_xhat(cx[k][j], mu[j], rs[j]), rs[j]);
                    st4(dx, R.at(s, p), m.lc, o);
                }
            }
            for (int p = m.lr + GN_CACHE_BWD * RS; p < P; p += RS) {
                const size_t off = R.at(s, p);
                const float4v xv = ld4(x, off, m.lc), dv = ld4(dy, off, m.lc);
                float4v o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g = gn_gated<RELU>(dv[j], xv[j], sc[j], sh[j]);
                    o[j] = gn_dx(g, ga[j], A[j], B[j], gn_xhat(xv[j], mu[j], rs[j]), rs[j]);
                }
                st4(dx, off, m.lc, o);
            }
        }
    }
    double *out = part + (size_t)blockIdx.x * 2 * R.C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double tg = col_reduce(m, m.on ? dg[j] : 0.0, cred);
        const double tb = col_reduce(m, m.on ? db[j] : 0.0, cred);
        if (m.lr == 0) {
            out[m.lc * 4 + j] = tg;
            out[R.C + m.lc * 4 + j] = tb;
        }
    }
}

// ================================================================ large samples
// Block b = s * nchunk + chunk takes the rows [chunk * rpc, min(P, (chunk + 1) * rpc)) of sample s.
struct Chunks {
    int nchunk;
    long long rpc;
};

// gpart: [S * nchunk][16] f64 -- sums for groups 0..7, then sums of squares
__global__ __launch_bounds__(GN_BLOCK_LARGE) void gn_large_fwd_partial_kernel(
    const float *__restrict__ x, const float *__restrict__ mask, double *__restrict__ gpart, long long P, Rows R,
    Chunks ch) {
    __shared__ double red[GN_BLOCK_LARGE / 64][2][8];
    const long long s = blockIdx.x / ch.nchunk;
    if (mask && mask[s] == 0.0f) return;             // its partials are never read (gn_group_finish_kernel)
    const int chunk = blockIdx.x % ch.nchunk;
    const Map<GN_BLOCK_LARGE> m(R.C);
    const long long p0 = chunk * ch.rpc, p1 = p0 + ch.rpc < P ? p0 + ch.rpc : P;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (m.on) {
        for (int c4 = m.lc; c4 < m.C4; c4 += m.L) {
            long long p = p0 + m.lr;
            for (; p + m.RS < p1; p += 2 * m.RS) {   // two rows in flight
                const float4v v0 = ld4(x, R.at(s, p), c4), v1 = ld4(x, R.at(s, p + m.RS), c4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc_sq(a[j], a[4 + j], v0[j]); acc_sq(a[j], a[4 + j], v1[j]); }
            }
            for (; p < p1; p += m.RS) {
                const float4v v = ld4(x, R.at(s, p), c4);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc_sq(a[j], a[4 + j], v[j]);
            }
        }
    }
    group_reduce<GN_BLOCK_LARGE>(a, red);
    if (threadIdx.x < 2) {
        double *o = gpart + (size_t)blockIdx.x * 16;
        const int par = threadIdx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[par * 4 + j] = a[j]; o[8 + par * 4 + j] = a[4 + j]; }
    }
}

// One block per sample: the 16 sums of its chunks in chunk order (16 slices, then the slices in order), then
// MODE 0: o0 = mean, o1 = rstd;  MODE 1: o0 = A = s / n, o1 = B = q / n.  A dead sample: zeros.
template <int MODE>
__global__ __launch_bounds__(256) void gn_group_finish_kernel(const double *__restrict__ gpart,
                                                              const float *__restrict__ mask, int nchunk, double inv_n,
                                                              double eps, float *__restrict__ o0, float *__restrict__ o1) {
    __shared__ double sl[GFIN_SLICES][16];
    __shared__ double tot[16];
    const long long s = blockIdx.x;
    const int i = threadIdx.x & 15, slice = threadIdx.x >> 4;
    if (mask && mask[s] == 0.0f) {
        if (threadIdx.x < GN_G) { o0[s * GN_G + threadIdx.x] = 0.0f; o1[s * GN_G + threadIdx.x] = 0.0f; }
        return;
    }
    const int per = (nchunk + GFIN_SLICES - 1) / GFIN_SLICES;
    const int c0 = slice * per, c1 = c0 + per < nchunk ? c0 + per : nchunk;
    double t = 0.0;
    for (int c = c0; c < c1; ++c) t += gpart[((size_t)s * nchunk + c) * 16 + i];
    sl[slice][i] = t;
    __syncthreads();
    if (threadIdx.x < 16) {
        double u = 0.0;
        for (int k = 0; k < GFIN_SLICES; ++k) u += sl[k][i];
        tot[i] = u;
    }
    __syncthreads();
    if (threadIdx.x < GN_G) {
        const int g = threadIdx.x;
        if (MODE == 0) {
            float mu, rs;
            gn_stats(tot[g], tot[8 + g], inv_n, eps, mu, rs);
            o0[s * GN_G + g] = mu;
            o1[s * GN_G + g] = rs;
        } else {
            o0[s * GN_G + g] = (float)(tot[g] * inv_n);
            o1[s * GN_G + g] = (float)(tot[8 + g] * inv_n);
        }
    }
}

template <bool RELU>
__global__ __launch_bounds__(GN_BLOCK_LARGE) void gn_large_fwd_apply_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ mask, const float *__restrict__ mean, const float *__restrict__ rstd,
    float *__restrict__ y, long long P, Rows R, Chunks ch) {
    const long long s = blockIdx.x / ch.nchunk;
    const int chunk = blockIdx.x % ch.nchunk;
    const Map<GN_BLOCK_LARGE> m(R.C);
    if (!m.on) return;
    const bool dead = mask && mask[s] == 0.0f;
    const long long p0 = chunk * ch.rpc, p1 = p0 + ch.rpc < P ? p0 + ch.rpc : P;
    const int par = m.lc & 1;
    const float4v zero4 = {0, 0, 0, 0};
    for (int c4 = m.lc; c4 < m.C4; c4 += m.L) {
        if (dead) {
            for (long long p = p0 + m.lr; p < p1; p += m.RS) st4(y, R.at(s, p), c4, zero4);
            continue;
        }
        const float4v ga = reinterpret_cast<const float4v *>(gamma)[c4], be = reinterpret_cast<const float4v *>(beta)[c4];
        float4v sc, sh;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float c0, c1;
            gn_coef(mean[s * GN_G + par * 4 + j], rstd[s * GN_G + par * 4 + j], ga[j], be[j], c0, c1);
            sc[j] = c0;
            sh[j] = c1;
        }
        long long p = p0 + m.lr;
        for (; p + m.RS < p1; p += 2 * m.RS) {
            const size_t o0 = R.at(s, p), o1 = R.at(s, p + m.RS);
            const float4v v0 = ld4(x, o0, c4), v1 = ld4(x, o1, c4);
            float4v r0, r1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r0[j] = RELU ? bn_affine_relu(v0[j], sc[j], sh[j]) : bn_affine(v0[j], sc[j], sh[j]);
                r1[j] = RELU ? bn_affine_relu(v1[j], sc[j], sh[j]) : bn_affine(v1[j], sc[j], sh[j]);
            }
            st4(y, o0, c4, r0);
            st4(y, o1, c4, r1);
        }
        for (; p < p1; p += m.RS) {
            const size_t o0 = R.at(s, p);
            const float4v v0 = ld4(x, o0, c4);
            float4v r0;
#pragma unroll
            for (int j = 0; j < 4; ++j) r0[j] = RELU ? bn_affine_relu(v0[j], sc[j], sh[j]) : bn_affine(v0[j], sc[j], sh[j]);
            st4(y, o0, c4, r0);
        }
    }
}

// gpart as in the forward, holding (sum g * gamma, sum g * gamma * xhat) per group; cpart: [S * nchunk][2][C] f64,
// (sum g * xhat, sum g) per channel over the chunk's rows -- zeros from a dead sample's blocks
template <bool RELU>
__global__ __launch_bounds__(GN_BLOCK_LARGE) void gn_large_bwd_partial_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ rstd,
    const float *__restrict__ mask, double *__restrict__ gpart, double *__restrict__ cpart, long long P, Rows R,
    Chunks ch) {
    __shared__ double red[GN_BLOCK_LARGE / 64][2][8];
    __shared__ double cred[GN_BLOCK_LARGE];
    const long long s = blockIdx.x / ch.nchunk;
    const int chunk = blockIdx.x % ch.nchunk;
    const Map<GN_BLOCK_LARGE> m(R.C);
    double *cout = cpart + (size_t)blockIdx.x * 2 * R.C;
    if (mask && mask[s] == 0.0f) {
        for (int c = threadIdx.x; c < 2 * R.C; c += GN_BLOCK_LARGE) cout[c] = 0.0;
        return;
    }
    const long long p0 = chunk * ch.rpc, p1 = p0 + ch.rpc < P ? p0 + ch.rpc : P;
    const int par = m.lc & 1;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int cc = 0; cc * m.L < m.C4; ++cc) {        // block-uniform trip count (col_reduce synchronises)
        const int c4 = cc * m.L + m.lc;
        const bool on = m.on && c4 < m.C4;
        double sg[4] = {0, 0, 0, 0}, sgx[4] = {0, 0, 0, 0};
        if (on) {
            const float4v ga = reinterpret_cast<const float4v *>(gamma)[c4],
                          be = reinterpret_cast<const float4v *>(beta)[c4];
            float4v mu, rs, sc, sh;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float c0, c1;
                mu[j] = mean[s * GN_G + par * 4 + j];
                rs[j] = rstd[s * GN_G + par * 4 + j];
                gn_coef(mu[j], rs[j], ga[j], be[j], c0, c1);
                sc[j] = c0;
                sh[j] = c1;
            }
            long long p = p0 + m.lr;
            for (; p + m.RS < p1; p += 2 * m.RS) {
                const size_t o0 = R.at(s, p), o1 = R.at(s, p + m.RS);
                const float4v x0 = ld4(x, o0, c4), d0 = ld4(dy, o0, c4), x1 = ld4(x, o1, c4), d1 = ld4(dy, o1, c4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g0 = gn_gated<RELU>(d0[j], x0[j], sc[j], sh[j]);
                    const float g1 = gn_gated<RELU>(d1[j], x1[j], sc[j], sh[j]);
                    sg[j] += (double)g0;
                    sgx[j] = __builtin_fma((double)g0, (double)gn_xhat(x0[j], mu[j], rs[j]), sgx[j]);
                    sg[j] += (double)g1;
                    sgx[j] = __builtin_fma((double)g1, (double)gn_xhat(x1[j], mu[j], rs[j]), sgx[j]);
                }
            }
            for (; p < p1; p += m.RS) {
                const size_t o0 = R.at(s, p);
                const float4v x0 = ld4(x, o0, c4), d0 = ld4(dy, o0, c4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g0 = gn_gated<RELU>(d0[j], x0[j], sc[j], sh[j]);
                    sg[j] += (double)g0;
                    sgx[j] = __builtin_fma((double)g0, (double)gn_xhat(x0[j], mu[j], rs[j]), sgx[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] += (double)ga[j] * sg[j];
                a[4 + j] += (double)ga[j] * sgx[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double tg = col_reduce(m, sgx[j], cred);
            const double tb = col_reduce(m, sg[j], cred);
            if (m.lr == 0 && c4 < m.C4) {
                cout[c4 * 4 + j] = tg;
                cout[R.C + c4 * 4 + j] = tb;
            }
        }
    }
    group_reduce<GN_BLOCK_LARGE>(a, red);
    if (threadIdx.x < 2) {
        double *o = gpart + (size_t)blockIdx.x * 16;
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[threadIdx.x * 4 + j] = a[j]; o[8 + threadIdx.x * 4 + j] = a[4 + j]; }
    }
}

template <bool RELU>
__global__ __launch_bounds__(GN_BLOCK_LARGE) void gn_large_bwd_apply_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ rstd,
    const float *__restrict__ mask, const float *__restrict__ Ag, const float *__restrict__ Bg, float *__restrict__ dx,
    long long P, Rows R, Chunks ch) {
    const long long s = blockIdx.x / ch.nchunk;
    const int chunk = blockIdx.x % ch.nchunk;
    const Map<GN_BLOCK_LARGE> m(R.C);
    if (!m.on) return;
    const bool dead = mask && mask[s] == 0.0f;
    const long long p0 = chunk * ch.rpc, p1 = p0 + ch.rpc < P ? p0 + ch.rpc : P;
    const int par = m.lc & 1;
    const float4v zero4 = {0, 0, 0, 0};
    for (int c4 = m.lc; c4 < m.C4; c4 += m.L) {
        if (dead) {
            for (long long p = p0 + m.lr; p < p1; p += m.RS) st4(dx, R.at(s, p), c4, zero4);
            continue;
        }
        const float4v ga = reinterpret_cast<const float4v *>(gamma)[c4], be = reinterpret_cast<const float4v *>(beta)[c4];
        float4v mu, rs, sc, sh, A, B;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float c0, c1;
            mu[j] = mean[s * GN_G + par * 4 + j];
            rs[j] = rstd[s * GN_G + par * 4 + j];
            A[j] = Ag[s * GN_G + par * 4 + j];
            B[j] = Bg[s * GN_G + par * 4 + j];
            gn_coef(mu[j], rs[j], ga[j], be[j], c0, c1);
            sc[j] = c0;
            sh[j] = c1;
        }
        long long p = p0 + m.lr;
        for (; p + m.RS < p1; p += 2 * m.RS) {
            const size_t o0 = R.at(s, p), o1 = R.at(s, p + m.RS);
            const float4v x0 = ld4(x, o0, c4), d0 = ld4(dy, o0, c4), x1 = ld4(x, o1, c4), d1 = ld4(dy, o1, c4);
            float4v r0, r1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r0[j] = gn_dx(gn_gated<RELU>(d0[j], x0[j], sc[j], sh[j]), ga[j], A[j], B[j], gn_xhat(x0[j], mu[j], rs[j]),
                              rs[j]);
                r1[j] = gn_dx(gn_gated<RELU>(d1[j], x1[j], sc[j], sh[j]), ga[j], A[j], B[j], gn_xhat(x1[j], mu[j], rs[j]),
                              rs[j]);
            }
            st4(dx, o0, c4, r0);
            st4(dx, o1, c4, r1);
        }
        for (; p < p1; p += m.RS) {
            const size_t o0 = R.at(s, p);
            const float4v x0 = ld4(x, o0, c4), d0 = ld4(dy, o0, c4);
            float4v r0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                r0[j] = gn_dx(gn_gated<RELU>(d0[j], x0[j], sc[j], sh[j]), ga[j], A[j], B[j], gn_xhat(x0[j], mu[j], rs[j]),
                              rs[j]);
            st4(dx, o0, c4, r0);
        }
    }
}

// ================================================================ the column finish of both regimes
// cpart: [nslots][2 * C] f64.  Column col < C is dgamma[col], else dbeta[col - C]: the slots summed in slot order
// (8 slices of consecutive slots, then the slices in order), rounded to f32 once.
__global__ __launch_bounds__(FIN_COLS *FIN_SLICES) void gn_cols_finish_kernel(const double *__restrict__ cpart,
                                                                               long long nslots, int C,
                                                                               float *__restrict__ dgamma,
                                                                               float *__restrict__ dbeta) {
    __shared__ double sl[FIN_SLICES][FIN_COLS];
    const int lc = threadIdx.x % FIN_COLS, slice = threadIdx.x / FIN_COLS;
    const int col = blockIdx.x * FIN_COLS + lc;
    const long long per = (nslots + FIN_SLICES - 1) / FIN_SLICES;
    const long long k0 = slice * per, k1 = k0 + per < nslots ? k0 + per : nslots;
    double t = 0.0;
    if (col < 2 * C)
        for (long long k = k0; k < k1; ++k) t += cpart[(size_t)k * 2 * C + col];
    sl[slice][lc] = t;
    __syncthreads();
    if (slice == 0 && col < 2 * C) {
        double u = 0.0;
        for (int k = 0; k < FIN_SLICES; ++k) u += sl[k][lc];
        if (col < C) dgamma[col] = (float)u;
        else dbeta[col - C] = (float)u;
    }
}

// ================================================================ host side
struct Plan {
    bool small;
    int grid_small;
    Chunks ch;
    long long nslots;           // [2, C] partials of the backward
    size_t off_c, off_ab, bytes;
};

bool shape_ok(long long S, long long P, int C, int G) {
    return G == GN_G && C >= GN_G && C % GN_G == 0 && C <= GN_MAX_C && S >= 1 && P >= 1 && P < (1LL << 31) &&
           S < (1LL << 31) && S * P < (1LL << 40);
}

Plan make_plan(long long S, long long P, int C) {
    Plan pl;
    pl.small = P * C <= GN_SMALL_MAX_FLOATS;
    pl.grid_small = (int)(S < GN_SMALL_MAX_WG ? S : GN_SMALL_MAX_WG);
    const int C4 = C / 4, L = C4 < GN_BLOCK_LARGE ? C4 : GN_BLOCK_LARGE, RS = GN_BLOCK_LARGE / L;
    const long long step = (long long)RS * GN_CHUNK_STEPS;
    long long want = (P + step - 1) / step;
    pl.ch.nchunk = (int)(want < 1 ? 1 : (want > GN_MAX_CHUNKS ? GN_MAX_CHUNKS : want));
    pl.ch.rpc = (P + pl.ch.nchunk - 1) / pl.ch.nchunk;
    pl.nslots = pl.small ? pl.grid_small : S * pl.ch.nchunk;
    const size_t gbytes = pl.small ? 0 : (size_t)S * pl.ch.nchunk * 16 * sizeof(double);
    pl.off_c = gbytes;
    pl.off_ab = pl.off_c + (size_t)pl.nslots * 2 * C * sizeof(double);
    pl.bytes = pl.off_ab + (size_t)S * GN_G * 2 * sizeof(float) + 16;
    return pl;
}

// the two layouts the kernels are given: sample-major (ss = P, ps = 1) and position-major (ss = 1, ps = S); nothing
// else is accepted, so that row s * ss + p * ps < S * P always
bool layout_ok(long long S, long long P, long long ss, long long ps) {
    return (ss == P && ps == 1) || (ss == 1 && ps == S);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// 1 when the fused kernels take S samples of P rows of C channels in G groups (f32, contiguous, 16-byte aligned)
PLUMB_API int wsplumb_groupnorm_supported(long long S, long long P, int C, int G) {
    if (!shape_ok(S, P, C, G)) return 0;
    const Plan pl = make_plan(S, P, C);
    return pl.small || S * pl.ch.nchunk < (1LL << 31);
}

// bytes of scratch a forward or backward call over that shape needs
PLUMB_API size_t wsplumb_groupnorm_workspace_bytes(long long S, long long P, int C) {
    if (!shape_ok(S, P, C, GN_G)) return 0;
    return make_plan(S, P, C).bytes;
}

// what[0]: 1 = small regime; what[1]: workgroups (small) or chunks per sample (large); what[2]: rows per chunk
PLUMB_API int wsplumb_groupnorm_plan(long long S, long long P, int C, long long *what) {
    if (!shape_ok(S, P, C, GN_G)) return 1;
    const Plan pl = make_plan(S, P, C);
    what[0] = pl.small;
    what[1] = pl.small ? pl.grid_small : pl.ch.nchunk;
    what[2] = pl.small ? P : pl.ch.rpc;
    return 0;
}

// y [S*P, C], mean / rstd [S, G].  mask: [S] f32 or null.  Returns 0, 1 for arguments it rejects (before any launch),
// 3 for a launch error.
PLUMB_API int wsplumb_groupnorm_forward(const float *x, long long S, long long P, int C, int G, long long ss, long long ps,
                                        const float *gamma, const float *beta, float eps, int relu, const float *mask,
                                        float *y, float *mean, float *rstd, void *ws, size_t ws_bytes, void *stream) {
    if (!wsplumb_groupnorm_supported(S, P, C, G) || !layout_ok(S, P, ss, ps) || !x || !gamma || !beta || !y || !mean ||
        !rstd || !aligned16(x) || !aligned16(y) || !aligned16(gamma) || !aligned16(beta))
        return 1;
    const Plan pl = make_plan(S, P, C);
    if (!pl.small && (!ws || ws_bytes < pl.bytes || !aligned16(ws))) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Rows R = {ss, ps, C};
    if (pl.small) {
        auto k = relu ? gn_small_fwd_kernel<true> : gn_small_fwd_kernel<false>;
        hipLaunchKernelGGL(k, dim3(pl.grid_small), dim3(GN_BLOCK_SMALL), 0, st, x, gamma, beta, mask, y, mean, rstd, S,
                           (int)P, R, eps);
    } else {
        double *gpart = static_cast<double *>(ws);
        const dim3 grid((unsigned)(S * pl.ch.nchunk));
        const double inv_n = 1.0 / ((double)P * (double)(C / GN_G));
        hipLaunchKernelGGL(gn_large_fwd_partial_kernel, grid, dim3(GN_BLOCK_LARGE), 0, st, x, mask, gpart, P, R, pl.ch);
        hipLaunchKernelGGL(gn_group_finish_kernel<0>, dim3((unsigned)S), dim3(256), 0, st, gpart, mask, pl.ch.nchunk,
                           inv_n, (double)eps, mean, rstd);
        auto k = relu ? gn_large_fwd_apply_kernel<true> : gn_large_fwd_apply_kernel<false>;
        hipLaunchKernelGGL(k, grid, dim3(GN_BLOCK_LARGE), 0, st, x, gamma, beta, mask, mean, rstd, y, P, R, pl.ch);
    }
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// dx [S*P, C], dgamma / dbeta [C] from x, dy and the forward's mean / rstd; beta only forms the ReLU gate.
PLUMB_API int wsplumb_groupnorm_backward(const float *x, const float *dy, long long S, long long P, int C, int G,
                                         long long ss, long long ps, const float *gamma, const float *beta,
                                         const float *mean, const float *rstd, int relu, const float *mask, float *dx,
                                         float *dgamma, float *dbeta, void *ws, size_t ws_bytes, void *stream) {
    if (!wsplumb_groupnorm_supported(S, P, C, G) || !layout_ok(S, P, ss, ps) || !x || !dy || !gamma || !beta || !mean ||
        !rstd || !dx || !dgamma || !dbeta || !aligned16(x) || !aligned16(dy) || !aligned16(dx) || !aligned16(gamma) ||
        !aligned16(beta))
        return 1;
    const Plan pl = make_plan(S, P, C);
    if (!ws || ws_bytes < pl.bytes || !aligned16(ws)) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Rows R = {ss, ps, C};
    char *base = static_cast<char *>(ws);
    double *cpart = reinterpret_cast<double *>(base + pl.off_c);
    if (pl.small) {
        auto k = relu ? gn_small_bwd_kernel<true> : gn_small_bwd_kernel<false>;
        hipLaunchKernelGGL(k, dim3(pl.grid_small), dim3(GN_BLOCK_SMALL), 0, st, x, dy, gamma, beta, mean, rstd, mask, dx,
                           cpart, S, (int)P, R);
    } else {
        double *gpart = reinterpret_cast<double *>(base);
        float *A = reinterpret_cast<float *>(base + pl.off_ab), *B = A + S * GN_G;
        const dim3 grid((unsigned)(S * pl.ch.nchunk));
        const double inv_n = 1.0 / ((double)P * (double)(C / GN_G));
        auto kp = relu ? gn_large_bwd_partial_kernel<true> : gn_large_bwd_partial_kernel<false>;
        hipLaunchKernelGGL(kp, grid, dim3(GN_BLOCK_LARGE), 0, st, x, dy, gamma, beta, mean, rstd, mask, gpart, cpart, P,
                           R, pl.ch);
        hipLaunchKernelGGL(gn_group_finish_kernel<1>, dim3((unsigned)S), dim3(256), 0, st, gpart, mask, pl.ch.nchunk,
                           inv_n, 0.0, A, B);
        auto ka = relu ? gn_large_bwd_apply_kernel<true> : gn_large_bwd_apply_kernel<false>;
        hipLaunchKernelGGL(ka, grid, dim3(GN_BLOCK_LARGE), 0, st, x, dy, gamma, beta, mean, rstd, mask, A, B, dx, P, R,
                           pl.ch);
    }
    hipLaunchKernelGGL(gn_cols_finish_kernel, dim3((unsigned)((2 * C + FIN_COLS - 1) / FIN_COLS)),
                       dim3(FIN_COLS * FIN_SLICES), 0, st, cpart, pl.nslots, C, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
