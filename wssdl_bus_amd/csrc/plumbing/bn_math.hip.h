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

// THE mean over the slots of a position-major [n_slots * R, C] matrix (row slot * R + roi), the head's exit: one
// order of additions for every route that forms it (rowbn.hip: rowbn_slot_mean_kernel, with or without the final norm
// applied to what it reads).  The slots are taken in slot order in chunks of SLOT_CHUNK = 16.  A chunk is summed by a
// balanced binary tree over its 16 places,
//   (((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7))) + (((v8 + v9) + (v10 + v11)) + ((v12 + v13) + (v14 + v15)))
// with +0 in a place past the last slot; the chunk sums are added in chunk order (the first one as it is), and the
// total is multiplied by 1.0f / n_slots, formed as that f32 quotient (exact for a power of two).  With 16 (4) slots
// this is the balanced tree of depth 4 (2): every addend goes through log2(n_slots) additions, each rounded once.
// The padding zeros cannot change a bit of a sum of values >= +0 -- what the head feeds, ReLU outputs: x + 0 = x,
// and 0 + 0 = 0 -- so the value is that of the tree over the slots alone; for other inputs they can only turn a sum
// that is -0 into +0.
constexpr int SLOT_CHUNK = 16;

template <class V>
static __device__ __forceinline__ V slot_chunk_sum(V (&v)[SLOT_CHUNK]) {
#pragma unroll
    for (int w = 1; w < SLOT_CHUNK; w *= 2)
#pragma unroll
        for (int i = 0; i < SLOT_CHUNK; i += 2 * w) v[i] = v[i] + v[i + w];
    return v[0];
}

// the factor of the mean, and of its gradient dfeat * (1 / n_slots)
static __host__ __device__ __forceinline__ float slot_mean_scale(int n_slots) { return 1.0f / (float)n_slots; }
