// The reference's optimisers (code/lib/fast_rcnn/train_bus.py:286-294, :694-697) as ONE launch over all the
// parameters: TensorFlow 1.x Adam in its "epsilon-hat" form, AMSGrad in the same form, and Nesterov momentum
// (ApplyMomentum with use_nesterov).  With stock ops each is about ten small launches for each of ~160 parameters
// per step.  Plumbing library, not the drop-in C ABI; the host side is fast_rcnn/optim.py.
//
//   Adam      m += (g - m) * (1 - b1);  v += (g * g - v) * (1 - b2);  p -= (m * alpha_t) / (sqrt(v) + eps)
//             alpha_t = lr * sqrt(1 - b2^t) / (1 - b1^t): computed by the host in f64, rounded once, passed by value
//   AMSGrad   Adam's m and v, then  vhat = max(vhat, v);  p -= (m * alpha_t) / (sqrt(vhat) + eps)
//   Nesterov  accum = accum * mu + g;  p -= g * lr + (accum * mu) * lr
//
// f32 throughout, every operation rounded on its own in exactly the order written (no contraction, no fast-math;
// sqrt and the division are the compiler's default, correctly rounded, forms).
//
// The parameters are separate allocations, so the kernel runs over the flat CHUNK space of l2decay.hip: chunk i
// covers up to CHUNK consecutive floats of one parameter's storage (storage order, whatever the strides: the
// parameters are dense).  A static table (built once per parameter list) gives each chunk's parameter, its first
// float inside that parameter, its length and its offset in the flat state buffers; a second static table holds the
// parameters' addresses.  Gradients are re-allocated every step, so their addresses come in a small per-step table,
// one int64 per parameter; 0 there means "no gradient" and the workgroups of that parameter return without touching
// the parameter or its state (apply_gradients with a None gradient).  A gradient has its parameter's layout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLUMB_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int BLOCK = 256;
constexpr int CHUNK = 4096;          // floats per chunk (keep in sync with fast_rcnn/optim.py: CHUNK)

typedef float float4v __attribute__((ext_vector_type(4)));

// one row of the static chunk table: four int64 (the layout of the Python binding)
struct Chunk {
    long long param;        // index into the two per-parameter tables
    long long first;        // first float of the chunk inside that parameter's storage
    long long n;            // 1 .. CHUNK floats
    long long off;          // the chunk's element offset in the flat state buffers (a multiple of 4)
};

enum Kind { ADAM = 0, AMSGRAD = 1, NESTEROV = 2 };

// lr and mu: Nesterov; alpha, eps, omb1 = 1 - b1, omb2 = 1 - b2: the two Adam forms
struct Scalars {
    float lr, mu, alpha, eps, omb1, omb2;
};

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// one element: p, g and the state words a, b, c (Adam: m, v; AMSGrad: m, v, vhat; Nesterov: accum)
template <int KIND>
__device__ __forceinline__ void update(float &p, float g, float &a, float &b, float &c, const Scalars &k) {
#pragma clang fp contract(off)
    if (KIND == NESTEROV) {
        const float acc = a * k.mu + g;
        a = acc;
        const float t0 = g * k.lr;
        const float t1 = acc * k.mu;
        const float t2 = t1 * k.lr;
        p = p - (t0 + t2);
    } else {
        const float d1 = g - a;
        const float m = a + d1 * k.omb1;
        const float gg = g * g;
        const float d2 = gg - b;
        const float v = b + d2 * k.omb2;
        a = m;
        b = v;
        float den = v;
        if (KIND == AMSGRAD) {
            den = c > v ? c : v;                             // max(vhat, v)
            c = den;
        }
        const float num = m * k.alpha;
        p = p - num / (__builtin_sqrtf(den) + k.eps);
    }
}

template <int KIND>
__global__ __launch_bounds__(BLOCK) void optim_kernel(const Chunk *__restrict__ tab, const long long *__restrict__ params,
                                                      const long long *__restrict__ grads, float *__restrict__ s0,
                                                      float *__restrict__ s1, float *__restrict__ s2, Scalars k) {
    const Chunk ch = tab[blockIdx.x];
    const long long gaddr = grads[ch.param];
    if (gaddr == 0) return;                                  // no gradient: parameter and state stay as they are
    float *__restrict__ p = reinterpret_cast<float *>(params[ch.param]) + ch.first;
    const float *__restrict__ g = reinterpret_cast<const float *>(gaddr) + ch.first;
    float *__restrict__ a = s0 + ch.off;
    float *__restrict__ b = KIND == NESTEROV ? nullptr : s1 + ch.off;
    float *__restrict__ c = KIND == AMSGRAD ? s2 + ch.off : nullptr;
    const int n = (int)ch.n;
    int done = 0;
    if (aligned16(p) && aligned16(g) && aligned16(a) && aligned16(b) && aligned16(c)) {      // workgroup-uniform
        const int n4 = n / 4;
        for (int i = threadIdx.x; i < n4; i += BLOCK) {
            float4v vp = reinterpret_cast<float4v *>(p)[i];
            const float4v vg = reinterpret_cast<const float4v *>(g)[i];
            float4v va = reinterpret_cast<float4v *>(a)[i];
            float4v vb = {0.f, 0.f, 0.f, 0.f}, vc = {0.f, 0.f, 0.f, 0.f};
            if (KIND != NESTEROV) vb = reinterpret_cast<float4v *>(b)[i];
            if (KIND == AMSGRAD) vc = reinterpret_cast<float4v *>(c)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float ep = vp[j], ea = va[j], eb = vb[j], ec = vc[j];
                update<KIND>(ep, vg[j], ea, eb, ec, k);
                vp[j] = ep, va[j] = ea, vb[j] = eb, vc[j] = ec;
            }
            reinterpret_cast<float4v *>(p)[i] = vp;
            reinterpret_cast<float4v *>(a)[i] = va;
            if (KIND != NESTEROV) reinterpret_cast<float4v *>(b)[i] = vb;
            if (KIND == AMSGRAD) reinterpret_cast<float4v *>(c)[i] = vc;
        }
        done = n4 * 4;
    }
    for (int i = done + threadIdx.x; i < n; i += BLOCK) {
        float ep = p[i], ea = a[i], eb = 0.f, ec = 0.f;
        if (KIND != NESTEROV) eb = b[i];
        if (KIND == AMSGRAD) ec = c[i];
        update<KIND>(ep, g[i], ea, eb, ec, k);
        p[i] = ep;
        a[i] = ea;
        if (KIND != NESTEROV) b[i] = eb;
        if (KIND == AMSGRAD) c[i] = ec;
    }
}

}  // namespace

// floats per chunk of the table
PLUMB_API int wsplumb_optim_chunk() { return CHUNK; }

// One step of optimiser `kind` (0 Adam, 1 AMSGrad, 2 Nesterov momentum) over every chunk of `tab`.
// tab: device table of n_chunks rows (struct Chunk), every n in 1 .. wsplumb_optim_chunk(); params, grads: device
// tables of n_params addresses (a 0 in grads: that parameter is skipped); s0, s1, s2: the flat state buffers (Adam:
// m, v; AMSGrad: m, v, vhat; Nesterov: accum -- the unused ones may be null).  lr and mu are Nesterov's, alpha_t, eps,
// b1 and b2 the Adam forms'.  Returns 0 on success, 1 for arguments it rejects (before any launch).
PLUMB_API int wsplumb_optim_step(int kind, const void *tab, int n_chunks, const void *params, const void *grads,
                                 int n_params, float *s0, float *s1, float *s2, float lr, float alpha_t, float eps,
                                 float mu, float b1, float b2, void *stream) {
    if (kind < ADAM || kind > NESTEROV || !tab || n_chunks < 1 || !params || !grads || n_params < 1 || !s0) return 1;
    if (kind != NESTEROV && !s1) return 1;
    if (kind == AMSGRAD && !s2) return 1;
    const Scalars k = {lr, mu, alpha_t, eps, 1.0f - b1, 1.0f - b2};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Chunk *t = static_cast<const Chunk *>(tab);
    const long long *pp = static_cast<const long long *>(params), *gp = static_cast<const long long *>(grads);
    if (kind == ADAM)
        hipLaunchKernelGGL(optim_kernel<ADAM>, dim3(n_chunks), dim3(BLOCK), 0, st, t, pp, gp, s0, s1, s2, k);
    else if (kind == AMSGRAD)
        hipLaunchKernelGGL(optim_kernel<AMSGRAD>, dim3(n_chunks), dim3(BLOCK), 0, st, t, pp, gp, s0, s1, s2, k);
    else
        hipLaunchKernelGGL(optim_kernel<NESTEROV>, dim3(n_chunks), dim3(BLOCK), 0, st, t, pp, gp, s0, s1, s2, k);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
