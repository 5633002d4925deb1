// Class-packed 3x3 patch gather for the per-RoI head's 3x3 convolutions (networks/roi_head.py,
// networks/_plumbing.py: TapConv3x3Fn).  With TF 'SAME' padding, the output positions whose
// patch reaches into the padding fall into a few POSITION CLASSES (centre, edges, corners of the
// 4x4 map); every position of a class has the same set of valid taps.  The dense route
// (im2col.hip) multiplies the padding taps' zeros as well: 44 of the 144 (position, tap) pairs of
// a 4x4 output.  Here each class is its own GEMM over only its valid taps, so the patch matrix,
// the weight and the gradients are packed class by class:
//   cols  class k: [npos_k][R][ntaps_k][C]  at float offset cum_k  * R   * C
//   W     class k: [c_o][ntaps_k][C]        at float offset wcum_k * c_o * C
// and the GEMM output of class k is rows slot_base_k*R .. (slot_base_k + npos_k)*R of the
// POSITION-MAJOR output, row = slot * R + roi.  Plumbing library, not the drop-in C ABI.
//
// The class table (int32, built by networks/_plumbing.py:tap_plan, layout TAB_* below) holds the
// geometry; R and C are call arguments.  The input is roi-major [R, H, W, C] or, when in_pm is
// set, position-major [H*W slots][R][C] in the table's own slot order (then H = OH, W = OW).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn_math.hip.h"

#define PLUMB_API extern "C" __attribute__((visibility("default")))

namespace {

// table layout (keep in sync with networks/_plumbing.py)
constexpr int TAB_NCLS = 0, TAB_H = 1, TAB_W = 2, TAB_OH = 3, TAB_OW = 4, TAB_S = 5, TAB_PT = 6, TAB_PL = 7,
              TAB_UNITS = 8, TAB_WUNITS = 9;
constexpr int TAB_CLS = 16, CLS_STRIDE = 24, MAX_CLS = 9;                 // per class:
constexpr int C_NPOS = 0, C_NTAPS = 1, C_SLOT = 2, C_CUM = 3, C_WCUM = 4,  // scalars
              C_TAPS = 6,                                                  // [9] tap ky*3+kx, in order
              C_TAPIDX = 15;                                               // [9] index of tap in class, -1
constexpr int MAX_POS = 64;
constexpr int TAB_SLOTPOS = TAB_CLS + CLS_STRIDE * MAX_CLS;  // [MAX_POS] slot -> position oy*OW+ox
constexpr int TAB_POSSLOT = TAB_SLOTPOS + MAX_POS;           // [MAX_POS] position -> slot
constexpr int TAB_SLOTCLS = TAB_POSSLOT + MAX_POS;           // [MAX_POS] slot -> class
constexpr int TAB_INTS = TAB_SLOTCLS + MAX_POS;

typedef float float4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ const int *cls_of(const int *T, int k) { return T + TAB_CLS + CLS_STRIDE * k; }

// class whose [cum, cum + size) range (field F of the class table) holds unit q
template <int F>
__device__ __forceinline__ int find_class(const int *__restrict__ T, unsigned q) {
    const int n = T[TAB_NCLS];
    int k = 0;
    while (k + 1 < n && (unsigned)cls_of(T, k + 1)[F] <= q) ++k;
    return k;
}

// Thread mapping of the two patch kernels: a workgroup owns one (position, tap) unit of the table (gather) or
// one input position (adjoint) and a chunk of RoIs, so the class, the tap, the source position and every
// table entry are the same for all its threads and come from scalar loads, once.  Thread t then walks
// float4 column(s) t % L (+ L ...) of RoIs roi0 + t / L (+ RS ...): L = C/4 and RS = 256 / L rows per pass when
// C/4 divides 256, else L = 256 columns of one row.  Per element: a float4 load, a float4 store, an add.
struct RoiWalk {
    unsigned L, RS, lc, lr, roi0, roi1;
    __device__ __forceinline__ RoiWalk(unsigned R, unsigned C4, unsigned chunk) {
        L = (C4 <= 256u && 256u % C4 == 0u) ? C4 : 256u;
        RS = 256u / L;
        lc = threadIdx.x % L;
        lr = threadIdx.x / L;
        roi0 = blockIdx.x * chunk;
        roi1 = roi0 + chunk < R ? roi0 + chunk : R;
    }
};

constexpr unsigned GATHER_CHUNK = 32, COL2IM_CHUNK = 16;    // RoIs per workgroup

// blockIdx.y = unit q of the packed patch matrix (class k, position p of the class, tap tl of the class),
// blockIdx.x = RoI chunk.  32-bit index math (total4 < 2^31, checked by the entry point).
// NORM: x is the raw output of the convolution in front (the bottleneck's conv1) and the copy applies that layer's
// norm and ReLU on the way, relu(x * scale + shift) with the arithmetic of rowbn_apply_fwd_kernel (bn_math.hip.h);
// the RoIs with mask[roi] == 0 (mask may be null) are not loaded and give zeros, as the layer writes them.  The
// thread's scale / shift float4 is loaded once per column pass.
template <bool NORM>
__global__ __launch_bounds__(256) void tap_gather_kernel(const float *__restrict__ x, const int *__restrict__ T,
                                                        int in_pm, unsigned R, unsigned C4,
                                                        float *__restrict__ cols, const float *__restrict__ scale,
                                                        const float *__restrict__ shift,
                                                        const float *__restrict__ mask) {
    const int H = T[TAB_H], W = T[TAB_W], OW = T[TAB_OW], S = T[TAB_S], PT = T[TAB_PT], PL = T[TAB_PL];
    const unsigned q = blockIdx.y;
    const int *cl = cls_of(T, find_class<C_CUM>(T, q));
    const unsigned ntaps = cl[C_NTAPS], local = q - (unsigned)cl[C_CUM];
    const unsigned p = local / ntaps, tl = local - p * ntaps;
    const int pos = T[TAB_SLOTPOS + cl[C_SLOT] + p];
    const int tap = cl[C_TAPS + tl];
    const int y = (pos / OW) * S + tap / 3 - PT, xx = (pos % OW) * S + tap % 3 - PL;
    const bool inside = y >= 0 && y < H && xx >= 0 && xx < W;   // always true by construction of the classes
    // source float4 of (roi, c4) = sbase + roi * sstride + c4, destination = dbase + roi * dstride + c4
    const unsigned sbase = !inside ? 0u : in_pm ? (unsigned)T[TAB_POSSLOT + y * W + xx] * R * C4 : (unsigned)(y * W + xx) * C4;
    const unsigned sstride = in_pm ? C4 : (unsigned)(H * W) * C4;
    const unsigned dstride = ntaps * C4;
    const unsigned dbase = (unsigned)cl[C_CUM] * R * C4 + p * R * dstride + tl * C4;
    const float4v *__restrict__ src = reinterpret_cast<const float4v *>(x) + sbase;
    float4v *__restrict__ dst = reinterpret_cast<float4v *>(cols) + dbase;
    const RoiWalk w(R, C4, GATHER_CHUNK);
    const float4v zero4 = {0.f, 0.f, 0.f, 0.f};
    for (unsigned c4 = w.lc; c4 < C4; c4 += w.L) {
        float4v sc = zero4, sh = zero4;
        if (NORM) {
            sc = reinterpret_cast<const float4v *>(scale)[c4];
            sh = reinterpret_cast<const float4v *>(shift)[c4];
        }
        // the (roi, c4) element: a copy, or the layer's output for a live RoI
        auto fetch = [&](unsigned roi) -> float4v {
            if (!NORM) return inside ? src[roi * sstride + c4] : zero4;
            if (!inside || (mask && mask[roi] == 0.0f)) return zero4;
            const float4v a = src[roi * sstride + c4];
            float4v o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = bn_affine_relu(a[j], sc[j], sh[j]);
            return o;
        };
        unsigned roi = w.roi0 + w.lr;
        for (; roi + 3u * w.RS < w.roi1; roi += 4u * w.RS) {          // four rows in flight
            float4v v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fetch(roi + k * w.RS);
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[(roi + k * w.RS) * dstride + c4] = v[k];
        }
        for (; roi < w.roi1; roi += w.RS) dst[roi * dstride + c4] = fetch(roi);
    }
}

// adjoint: blockIdx.y = input position (row-major y*W+x of the roi-major layout, or the slot with in_pm),
// blockIdx.x = RoI chunk.  The (at most 9) packed units that copied the position are resolved once, in the
// (ky, kx) order of col2im3x3_kernel (im2col.hip), and every element adds them in that order starting from
// +0, so that it is bit-equal to the dense adjoint given the same values in the valid columns.
__global__ __launch_bounds__(256) void tap_col2im_kernel(const float *__restrict__ dcols, const int *__restrict__ T,
                                                        int in_pm, unsigned R, unsigned C4,
                                                        float *__restrict__ dx) {
    const int H = T[TAB_H], W = T[TAB_W], OH = T[TAB_OH], OW = T[TAB_OW], S = T[TAB_S], PT = T[TAB_PT],
              PL = T[TAB_PL];
    const int pos = in_pm ? T[TAB_SLOTPOS + blockIdx.y] : (int)blockIdx.y;
    const int y = pos / W, xx = pos % W;
    unsigned base[9], stride[9], valid = 0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int j = ky * 3 + kx;
            base[j] = stride[j] = 0;
            const int ny = y + PT - ky, nx = xx + PL - kx;
            if (ny < 0 || ny % S != 0 || nx < 0 || nx % S != 0) continue;
            const int oy = ny / S, ox = nx / S;
            if (oy >= OH || ox >= OW) continue;
            const int slot = T[TAB_POSSLOT + oy * OW + ox];
            const int *cl = cls_of(T, T[TAB_SLOTCLS + slot]);
            const int tl = cl[C_TAPIDX + j];
            if (tl < 0) continue;                      // never: an in-bounds input is a valid tap
            stride[j] = (unsigned)cl[C_NTAPS] * C4;
            base[j] = (unsigned)cl[C_CUM] * R * C4 + (unsigned)(slot - cl[C_SLOT]) * R * stride[j] + (unsigned)tl * C4;
            valid |= 1u << j;
        }
    }
    const float4v *__restrict__ src = reinterpret_cast<const float4v *>(dcols);
    // destination float4 of (roi, c4) = dbase + roi * dstride + c4
    const unsigned dbase = in_pm ? blockIdx.y * R * C4 : (unsigned)pos * C4;
    const unsigned dstride = in_pm ? C4 : (unsigned)(H * W) * C4;
    float4v *__restrict__ dst = reinterpret_cast<float4v *>(dx) + dbase;
    const RoiWalk w(R, C4, COL2IM_CHUNK);
    for (unsigned c4 = w.lc; c4 < C4; c4 += w.L) {
        for (unsigned roi = w.roi0 + w.lr; roi < w.roi1; roi += w.RS) {
            float4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 9; ++j)
                if (valid & (1u << j)) acc += src[base[j] + roi * stride[j] + c4];
            dst[roi * dstride + c4] = acc;
        }
    }
}

// weight [c_o][9][C] -> class-packed [c_o][ntaps_k][C] per class (a copy)
__global__ __launch_bounds__(256) void tap_weight_gather_kernel(const float *__restrict__ w, const int *__restrict__ T,
                                                               unsigned CO, unsigned C4, unsigned total4,
                                                               float *__restrict__ wp) {
    const unsigned unit4 = CO * C4;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total4; i += gridDim.x * 256u) {
        const int k = find_class<C_WCUM>(T, i / unit4);
        const int *cl = cls_of(T, k);
        const unsigned ntaps = cl[C_NTAPS];
        const unsigned local = i - (unsigned)cl[C_WCUM] * unit4;
        const unsigned c4 = local % C4, t = local / C4;
        const unsigned tl = t % ntaps, o = t / ntaps;
        reinterpret_cast<float4v *>(wp)[i] =
            reinterpret_cast<const float4v *>(w)[((size_t)o * 9 + cl[C_TAPS + tl]) * C4 + c4];
    }
}

// adjoint of the weight gather: dW[o][tap][c] = sum over the classes that hold the tap, in class order
// (no atomics: deterministic).  Taps no class holds get 0.
__global__ __launch_bounds__(256) void tap_weight_scatter_kernel(const float *__restrict__ dwp, const int *__restrict__ T,
                                                                unsigned CO, unsigned C4, unsigned total4,
                                                                float *__restrict__ dw) {
    const int n = T[TAB_NCLS];
    const unsigned unit4 = CO * C4;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total4; i += gridDim.x * 256u) {
        const unsigned c4 = i % C4, t = i / C4;
        const unsigned tap = t % 9u, o = t / 9u;
        float4v acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < n; ++k) {
            const int *cl = cls_of(T, k);
            const int tl = cl[C_TAPIDX + tap];
            if (tl < 0) continue;
            acc += reinterpret_cast<const float4v *>(dwp)[(size_t)cl[C_WCUM] * unit4 +
                                                           ((size_t)o * cl[C_NTAPS] + tl) * C4 + c4];
        }
        reinterpret_cast<float4v *>(dw)[i] = acc;
    }
}

inline int grid_for(unsigned total4) {
    unsigned b = (total4 + 255u) / 256u;
    return (int)(b < 262144u ? b : 262144u);
}

// workgroups along x of the patch kernels: RoI chunks (R < 2^31 by dims_ok)
inline unsigned roi_chunks(long long R, unsigned chunk) { return (unsigned)((R + chunk - 1) / chunk); }

// R, C and the products the kernels index with 32-bit math
inline bool dims_ok(long long R, int C, long long total4) {
    return R >= 1 && C >= 4 && !(C & 3) && total4 >= 1 && total4 <= 0x7fffffffLL;
}

}  // namespace

// int32 count of a class table
PLUMB_API int wsplumb_tap_table_ints() { return TAB_INTS; }

namespace {

// the shape checks and the launch of both gather exports
template <bool NORM>
int gather_impl(const float *x, long long R, int C, const int *tab, const int *hnum, int in_pm, float *cols,
                const float *scale, const float *shift, const float *mask, void *stream) {
    const long long total4 = (long long)hnum[TAB_UNITS] * R * (C / 4);
    if (R < 1 || C < 4 || (C & 3)) return 1;
    if (!dims_ok(R, C, total4) || (long long)hnum[TAB_H] * hnum[TAB_W] * R * (C / 4) > 0x7fffffffLL) return 2;
    if (hnum[TAB_UNITS] < 1 || hnum[TAB_UNITS] > 65535) return 1;
    hipLaunchKernelGGL(tap_gather_kernel<NORM>, dim3(roi_chunks(R, GATHER_CHUNK), hnum[TAB_UNITS]), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, tab, in_pm, (unsigned)R, (unsigned)(C / 4), cols, scale, shift,
                       mask);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

// cols (class-packed, TAB_UNITS * R * C floats) <- x.  tab: device copy of the class table; hnum: host copy
// (the shape checks read it).  Returns 0 on success, 1 on a bad shape, 2 when the indices exceed 32 bits.
PLUMB_API int wsplumb_tap_gather(const float *x, long long R, int C, const int *tab, const int *hnum, int in_pm,
                                 float *cols, void *stream) {
    return gather_impl<false>(x, R, C, tab, hnum, in_pm, cols, nullptr, nullptr, nullptr, stream);
}

// cols <- relu(x * scale + shift), zeros for the RoIs with mask[roi] == 0: the gather of the output of a row batch
// norm + ReLU over x given that layer's scale / shift [C] (wsplumb_rowbn_stats); mask [R] f32 or null.
PLUMB_API int wsplumb_tap_gather_norm(const float *x, long long R, int C, const int *tab, const int *hnum, int in_pm,
                                      const float *scale, const float *shift, const float *mask, float *cols,
                                      void *stream) {
    if (!scale || !shift) return 1;
    return gather_impl<true>(x, R, C, tab, hnum, in_pm, cols, scale, shift, mask, stream);
}

// dx (roi-major [R, H, W, C] or position-major) <- class-packed dcols
PLUMB_API int wsplumb_tap_col2im(const float *dcols, long long R, int C, const int *tab, const int *hnum, int in_pm,
                                 float *dx, void *stream) {
    const long long total4 = (long long)hnum[TAB_H] * hnum[TAB_W] * R * (C / 4);
    if (R < 1 || C < 4 || (C & 3)) return 1;
    if (!dims_ok(R, C, total4) || (long long)hnum[TAB_UNITS] * R * (C / 4) > 0x7fffffffLL) return 2;
    if (hnum[TAB_H] * hnum[TAB_W] < 1 || hnum[TAB_H] * hnum[TAB_W] > MAX_POS) return 1;
    hipLaunchKernelGGL(tap_col2im_kernel, dim3(roi_chunks(R, COL2IM_CHUNK), hnum[TAB_H] * hnum[TAB_W]), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dcols, tab, in_pm, (unsigned)R, (unsigned)(C / 4), dx);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// wp (TAB_WUNITS * c_o * C floats) <- weight [c_o, 9*C]
PLUMB_API int wsplumb_tap_weight_gather(const float *w, int CO, int C, const int *tab, const int *hnum, float *wp,
                                        void *stream) {
    const long long total4 = (long long)hnum[TAB_WUNITS] * CO * (C / 4);
    if (CO < 1 || !dims_ok(CO, C, total4) || 9LL * CO * (C / 4) > 0x7fffffffLL) return 1;
    hipLaunchKernelGGL(tap_weight_gather_kernel, dim3(grid_for((unsigned)total4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), w, tab, (unsigned)CO, (unsigned)(C / 4), (unsigned)total4, wp);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// dweight [c_o, 9*C] <- class-packed dwp (overwritten, not accumulated)
PLUMB_API int wsplumb_tap_weight_scatter(const float *dwp, int CO, int C, const int *tab, const int *hnum, float *dw,
                                         void *stream) {
    const long long total4 = 9LL * CO * (C / 4);
    if (CO < 1 || !dims_ok(CO, C, total4) || (long long)hnum[TAB_WUNITS] * CO * (C / 4) > 0x7fffffffLL) return 1;
    hipLaunchKernelGGL(tap_weight_scatter_kernel, dim3(grid_for((unsigned)total4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dwp, tab, (unsigned)CO, (unsigned)(C / 4), (unsigned)total4, dw);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
