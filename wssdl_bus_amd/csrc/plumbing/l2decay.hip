// L2 weight decay of the training step (fast_rcnn/train_bus.py: l2_weight_decay) as one device op over ALL the
// decayed parameters:  value = f32(sum over every weight of w*w) * k,  gradient of weight w = 2 * w * (gout * k).
// With stock ops this is a multiply, a reduction and, in the backward, three more launches PER PARAMETER (about 230
// launches of 5-9 us per step for ~58 weights); here it is two launches forward and one backward.  Plumbing library,
// not the drop-in C ABI.
//
// The parameters are separate allocations, so the kernels run over a flat CHUNK space: chunk i covers up to CHUNK
// consecutive floats of one parameter's storage (parameters are walked in storage order, whatever their strides:
// they are dense), and a device table (built by networks/_plumbing.py, cached while the parameters stay where they
// are) gives its first float, its element offset in the flat gradient buffer and its length.
//
// Sums are f64 (the product of two f32 values is exact in f64) and every order is fixed: a thread adds its elements
// in index order, a workgroup adds its threads by a fixed tree, and the finish kernel adds the chunk partials in
// index order (64 consecutive runs, then the runs in order).  The value does not depend on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLUMB_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int BLOCK = 256;
constexpr int CHUNK = 4096;          // floats per chunk (keep in sync with networks/_plumbing.py: _L2_CHUNK)
constexpr int FIN_LANES = 64;

typedef float float4v __attribute__((ext_vector_type(4)));

// one row of the chunk table: three int64 (the layout of the Python binding)
struct Chunk {
    const float *w;         // first float of the chunk
    long long off;          // its element offset in the flat gradient buffer
    long long n;            // 1 .. CHUNK floats
};

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// partial[chunk] = sum of w*w over the chunk
__global__ __launch_bounds__(BLOCK) void l2decay_sumsq_kernel(const Chunk *__restrict__ tab, double *__restrict__ partial) {
    __shared__ double red[BLOCK];
    const Chunk ch = tab[blockIdx.x];
    const int n = (int)ch.n;
    double s = 0.0;
    int done = 0;
    if (aligned16(ch.w)) {                                   // workgroup-uniform
        const int n4 = n / 4;
        for (int i = threadIdx.x; i < n4; i += BLOCK) {
            const float4v v = reinterpret_cast<const float4v *>(ch.w)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) s = __builtin_fma((double)v[j], (double)v[j], s);
        }
        done = n4 * 4;
    }
    for (int i = done + threadIdx.x; i < n; i += BLOCK) {
        const float v = ch.w[i];
        s = __builtin_fma((double)v, (double)v, s);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// out[0] = f32(sum of the partials) * k: one wave, lane l adds its run of consecutive partials in index order,
// lane 0 then adds the runs in order; one rounding to f32, one f32 multiply.
__global__ __launch_bounds__(FIN_LANES) void l2decay_finish_kernel(const double *__restrict__ partial, int n, float k,
                                                                   float *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[FIN_LANES];
    const int per = (n + FIN_LANES - 1) / FIN_LANES;
    const int b = (int)threadIdx.x * per;
    const int e = b + per < n ? b + per : n;
    double s = 0.0;
    for (int i = b; i < e; ++i) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int l = 0; l < FIN_LANES; ++l) t += red[l];
        out[0] = (float)t * k;
    }
}

// flat[off + i] = (w[i] * c) + (w[i] * c), c = gout[0] * k: the roundings of the stock chain (the scalar multiply's
// backward, then the two equal products of d(w*w) summed), no contraction.
__device__ __forceinline__ float decay_grad(float w, float c) {
#pragma clang fp contract(off)
    const float t = w * c;
    return t + t;
}

__global__ __launch_bounds__(BLOCK) void l2decay_grad_kernel(const Chunk *__restrict__ tab, const float *__restrict__ gout,
                                                             float k, float *__restrict__ flat) {
#pragma clang fp contract(off)
    const Chunk ch = tab[blockIdx.x];
    const int n = (int)ch.n;
    const float c = gout[0] * k;
    float *__restrict__ dst = flat + ch.off;
    int done = 0;
    if (aligned16(ch.w) && aligned16(dst)) {                 // workgroup-uniform
        const int n4 = n / 4;
        for (int i = threadIdx.x; i < n4; i += BLOCK) {
            const float4v v = reinterpret_cast<const float4v *>(ch.w)[i];
            float4v o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = decay_grad(v[j], c);
            reinterpret_cast<float4v *>(dst)[i] = o;
        }
        done = n4 * 4;
    }
    for (int i = done + threadIdx.x; i < n; i += BLOCK) dst[i] = decay_grad(ch.w[i], c);
}

inline bool chunks_ok(const void *tab, int n_chunks) { return tab && n_chunks >= 1; }

}  // namespace

// floats per chunk of the table
PLUMB_API int wsplumb_l2decay_chunk() { return CHUNK; }

// out[0] = f32(sum of w*w over every chunk of tab) * k.  tab: device table of n_chunks rows (struct Chunk), every
// n in 1 .. wsplumb_l2decay_chunk(); partial: n_chunks doubles of scratch.  Returns 0 on success, 1 for arguments it
// rejects (before any launch).
PLUMB_API int wsplumb_l2decay_forward(const void *tab, int n_chunks, double *partial, float k, float *out, void *stream) {
    if (!chunks_ok(tab, n_chunks) || !partial || !out) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(l2decay_sumsq_kernel, dim3(n_chunks), dim3(BLOCK), 0, st, static_cast<const Chunk *>(tab), partial);
    hipLaunchKernelGGL(l2decay_finish_kernel, dim3(1), dim3(FIN_LANES), 0, st, partial, n_chunks, k, out);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// every chunk's gradient into the flat buffer: flat[off + i] = 2 * w[i] * (gout[0] * k), gout read on the device
PLUMB_API int wsplumb_l2decay_backward(const void *tab, int n_chunks, const float *gout, float k, float *flat,
                                       void *stream) {
    if (!chunks_ok(tab, n_chunks) || !gout || !flat) return 1;
    hipLaunchKernelGGL(l2decay_grad_kernel, dim3(n_chunks), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                       static_cast<const Chunk *>(tab), gout, k, flat);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
