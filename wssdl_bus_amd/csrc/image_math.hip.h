// The image path's arithmetic, one definition per statement (image.hip: one image per launch chain;
// image_batch.hip: a whole mini-batch per op).  The two are bit for bit the same because they include this file.
//
// Reference: code/lib/utils/blob.py:49-60 (brightness, contrast, mean subtraction of prep_im_for_blob) and the
// bilinear cell of skimage.transform.warp, order 1 (skimage/transform/_warps_cy.pyx `_warp_fast`,
// interpolation.pxd `bilinear_interpolation`).  Every operation is rounded on its own (-ffp-contract=off).
#pragma once

#include "common.hip.h"

namespace wssdl {

// partial results per reduction (sum of the contrast step's mean, min / max of a warp's clip range): block b of
// IMG_PARTS takes elements b * 256 + t with stride IMG_PARTS * 256, and the partials meet in the trees below.
// The order is part of the result.
constexpr int IMG_PARTS = 256;

// ---- blob.py:49-60 on the u8 grey plane, f32 (the random draws are Python floats: weak scalars) -------------------
__device__ __forceinline__ float u8_unit(unsigned char u) { return (float)u / 255.0f; }

// / 255 and the brightness step: what the contrast step's mean is taken over
__device__ __forceinline__ float prep_value(unsigned char u, int use_b, float delta) {
    float v = u8_unit(u);
    if (use_b) {
        v = v + delta;
        v = fminf(fmaxf(v, 0.0f), 1.0f);
    }
    return v;
}

// the whole map of one u8 value: brightness, contrast about the mean mm, im -= pixel_means / 255. (f64, rounded once)
__device__ __forceinline__ float prep_pixel(unsigned char u, int use_b, float delta, int use_c, float factor, float mm,
                                            double mean_sub) {
    float v = prep_value(u, use_b, delta);
    if (use_c) {
        v = v - mm;
        v = v * factor;
        v = v + mm;
        v = fminf(fmaxf(v, 0.0f), 1.0f);
    }
    return (float)((double)v - mean_sub);
}

// ---- the same steps on the float64 image skimage.transform.rotate returns (weak images, blob.py:39-41), all f64 ----
__device__ __forceinline__ double adjust_value(double v, int use_b, double delta) {
    if (use_b) {
        v = v + delta;
        v = fmin(fmax(v, 0.0), 1.0);
    }
    return v;
}

__device__ __forceinline__ double adjust_pixel(double v, int use_b, double delta, int use_c, double factor, double mm,
                                               double mean_sub) {
    v = adjust_value(v, use_b, delta);
    if (use_c) {
        v = v - mm;
        v = v * factor;
        v = v + mm;
        v = fmin(fmax(v, 0.0), 1.0);
    }
    return v - mean_sub;
}

// ---- bilinear cell of the input coordinate (c, r): the four neighbours and the two weights ------------------------
struct Cell { long long minr, minc, maxr, maxc; double dr, dc; };

__device__ __forceinline__ Cell warp_cell(double c, double r) {
    Cell q;
    const double fr = floor(r), fc = floor(c);
    // (a coordinate far outside any image: every neighbour is outside, clamp before the integer cast)
    const double big = 4.0e9;
    q.minr = (long long)fmax(fmin(fr, big), -big);
    q.minc = (long long)fmax(fmin(fc, big), -big);
    q.maxr = (long long)fmax(fmin(ceil(r), big), -big);
    q.maxc = (long long)fmax(fmin(ceil(c), big), -big);
    q.dr = r - fr;
    q.dc = c - fc;
    return q;
}

__device__ __forceinline__ double warp_mix(const Cell &q, double p00, double p01, double p10, double p11) {
    double top = (1.0 - q.dc) * p00;  top = top + q.dc * p01;
    double bot = (1.0 - q.dc) * p10;  bot = bot + q.dc * p11;
    double v = (1.0 - q.dr) * top;  v = v + q.dr * bot;
    return v;
}

// ---- fixed-order trees over the 256 LDS slots of a 256-thread block -----------------------------------------------
// join(a, b) folds slot b into slot a.  The slots must have been published by a barrier; the result is in slot 0,
// visible to every thread on return.
template <typename Join>
__device__ __forceinline__ void tree256(Join join) {
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) join((int)threadIdx.x, (int)threadIdx.x + st);
        __syncthreads();
    }
}

__device__ __forceinline__ double tree_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double tree_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ int tree_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ int tree_max(int a, int b) { return max(a, b); }

__device__ __forceinline__ void tree_sum256(double *s) {
    tree256([=](int a, int b) { s[a] += s[b]; });
}

template <typename T>
__device__ __forceinline__ void tree_minmax256(T *lo, T *hi) {
    tree256([=](int a, int b) {
        lo[a] = tree_min(lo[a], lo[b]);
        hi[a] = tree_max(hi[a], hi[b]);
    });
}

// the sum and the extremes in one walk (the same levels, one barrier each)
template <typename T>
__device__ __forceinline__ void tree_sum_minmax256(double *s, T *lo, T *hi) {
    tree256([=](int a, int b) {
        s[a] += s[b];
        lo[a] = tree_min(lo[a], lo[b]);
        hi[a] = tree_max(hi[a], hi[b]);
    });
}

}  // namespace wssdl
