// Arithmetic that more than one file of the plumbing library must round alike (rowbn.hip, taps.hip).
// The fused multiply-adds are written out: left to the compiler's contraction, the same expression came out
// fused in one kernel and as separate multiplies and subtractions in another (even lane by lane within one
// kernel), and a kernel that stands for a layer must round exactly as the layer it replaces.
#pragma once
#include <hip/hip_runtime.h>

// y = x*scale + shift
static __device__ __forceinline__ float bn_affine(float x, float sc, float sh) { return __builtin_fmaf(x, sc, sh); }
// relu(x*scale + shift) as the apply kernels form it (a NaN becomes 0)
static __device__ __forceinline__ float bn_affine_relu(float x, float sc, float sh) {
    const float v = bn_affine(x, sc, sh);
    return v > 0.0f ? v : 0.0f;
}
