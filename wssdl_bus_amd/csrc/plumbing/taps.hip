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

// one thread = one float4 of the packed patch matrix; consecutive threads walk c, then the tap,
// then the RoI: coalesced writes, reads coalesced per tap.  32-bit index math (total4 < 2^31).
__global__ __launch_bounds__(256) void tap_gather_kernel(const float *__restrict__ x, const int *__restrict__ T,
                                                        int in_pm, unsigned R, unsigned C4, unsigned total4,
                                                        float *__restrict__ cols) {
    const int H = T[TAB_H], W = T[TAB_W], OW = T[TAB_OW], S = T[TAB_S], PT = T[TAB_PT], PL = T[TAB_PL];
    const unsigned unit4 = R * C4;                       // float4s of one (position, tap) unit
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total4; i += gridDim.x * 256u) {
        const int k = find_class<C_CUM>(T, i / unit4);
        const int *cl = cls_of(T, k);
        const unsigned ntaps = cl[C_NTAPS];
        const unsigned local = i - (unsigned)cl[C_CUM] * unit4;
        const unsigned c4 = local % C4, t = local / C4;
        const unsigned tl = t % ntaps, row = t / ntaps;
        const unsigned roi = row % R, p = row / R;
        const int pos = T[TAB_SLOTPOS + cl[C_SLOT] + p];
        const int tap = cl[C_TAPS + tl];
        const int y = (pos / OW) * S + tap / 3 - PT, xx = (pos % OW) * S + tap % 3 - PL;
        float4v v = {0.f, 0.f, 0.f, 0.f};
        if (y >= 0 && y < H && xx >= 0 && xx < W) {     // always true by construction of the classes
            const size_t src = in_pm ? (size_t)T[TAB_POSSLOT + y * W + xx] * R + roi
                                     : ((size_t)roi * H + y) * W + xx;
            v = reinterpret_cast<const float4v *>(x)[src * C4 + c4];
        }
        reinterpret_cast<float4v *>(cols)[i] = v;
    }
}

// adjoint: one thread = one float4 of dx; adds the (at most 9) packed entries that copied it in the
// (ky, kx) order of col2im3x3_kernel (im2col.hip), so that it is bit-equal to the dense adjoint given the
// same values in the valid columns
__global__ __launch_bounds__(256) void tap_col2im_kernel(const float *__restrict__ dcols, const int *__restrict__ T,
                                                        int in_pm, unsigned R, unsigned C4, unsigned total4,
                                                        float *__restrict__ dx) {
    const int H = T[TAB_H], W = T[TAB_W], OH = T[TAB_OH], OW = T[TAB_OW], S = T[TAB_S], PT = T[TAB_PT],
              PL = T[TAB_PL];
    const unsigned unit4 = R * C4;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total4; i += gridDim.x * 256u) {
        const unsigned c4 = i % C4, row = i / C4;
        unsigned roi;
        int y, xx;
        if (in_pm) {
            roi = row % R;
            const int pos = T[TAB_SLOTPOS + row / R];
            y = pos / W;
            xx = pos % W;
        } else {
            xx = (int)(row % (unsigned)W);
            const unsigned t = row / (unsigned)W;
            y = (int)(t % (unsigned)H);
            roi = t / (unsigned)H;
        }
        float4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ny = y + PT - ky;
            if (ny < 0 || ny % S != 0) continue;
            const int oy = ny / S;
            if (oy >= OH) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int nx = xx + PL - kx;
                if (nx < 0 || nx % S != 0) continue;
                const int ox = nx / S;
                if (ox >= OW) continue;
                const int slot = T[TAB_POSSLOT + oy * OW + ox];
                const int *cl = cls_of(T, T[TAB_SLOTCLS + slot]);
                const int tl = cl[C_TAPIDX + ky * 3 + kx];
                if (tl < 0) continue;                  // never: an in-bounds input is a valid tap
                const size_t u = (size_t)cl[C_CUM] * unit4 +
                                 (((size_t)(slot - cl[C_SLOT]) * R + roi) * cl[C_NTAPS] + tl) * C4 + c4;
                acc += reinterpret_cast<const float4v *>(dcols)[u];
            }
        }
        reinterpret_cast<float4v *>(dx)[i] = acc;
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

// R, C and the products the kernels index with 32-bit math
inline bool dims_ok(long long R, int C, long long total4) {
    return R >= 1 && C >= 4 && !(C & 3) && total4 >= 1 && total4 <= 0x7fffffffLL;
}

}  // namespace

// int32 count of a class table
PLUMB_API int wsplumb_tap_table_ints() { return TAB_INTS; }

// cols (class-packed, TAB_UNITS * R * C floats) <- x.  tab: device copy of the class table; hnum: host copy
// (the shape checks read it).  Returns 0 on success, 1 on a bad shape, 2 when the indices exceed 32 bits.
PLUMB_API int wsplumb_tap_gather(const float *x, long long R, int C, const int *tab, const int *hnum, int in_pm,
                                 float *cols, void *stream) {
    const long long total4 = (long long)hnum[TAB_UNITS] * R * (C / 4);
    if (R < 1 || C < 4 || (C & 3)) return 1;
    if (!dims_ok(R, C, total4) || (long long)hnum[TAB_H] * hnum[TAB_W] * R * (C / 4) > 0x7fffffffLL) return 2;
    hipLaunchKernelGGL(tap_gather_kernel, dim3(grid_for((unsigned)total4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, tab, in_pm, (unsigned)R, (unsigned)(C / 4),
                       (unsigned)total4, cols);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// dx (roi-major [R, H, W, C] or position-major) <- class-packed dcols
PLUMB_API int wsplumb_tap_col2im(const float *dcols, long long R, int C, const int *tab, const int *hnum, int in_pm,
                                 float *dx, void *stream) {
    const long long total4 = (long long)hnum[TAB_H] * hnum[TAB_W] * R * (C / 4);
    if (R < 1 || C < 4 || (C & 3)) return 1;
    if (!dims_ok(R, C, total4) || (long long)hnum[TAB_UNITS] * R * (C / 4) > 0x7fffffffLL) return 2;
    hipLaunchKernelGGL(tap_col2im_kernel, dim3(grid_for((unsigned)total4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dcols, tab, in_pm, (unsigned)R, (unsigned)(C / 4),
                       (unsigned)total4, dx);
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
