// The image blob of a whole mini-batch in one op (roi_data_layer/minibatch_bus.py:259-318), gfx950.
//
// image.hip builds one image with a chain of single-image launches and full-size temporaries (u8 -> f32 x3 ->
// [rotate: f64 x3 -> adjust: f64 x3] -> resize: f64 x3 -> blob).  Here the batch is
//   LAUNCHES PER BATCH: 3 (2 when no item is rotated), whatever the number of images
//     1. image_batch_stats_kernel    grid (256, N): the partial sums of the contrast step's mean and the u8 extremes
//     2. image_batch_rotate_kernel   grid (256, N), rotated items only: rotate() at every pixel of the crop -> one f64
//                                    channel in the workspace, the partial sums of ITS mean, its extremes
//     3. image_batch_blob_kernel     grid (blocks, N): the resize as a gather from the u8 plane (through a 256-entry
//                                    table of the whole pre-resize map, built per block in LDS) or from the rotated
//                                    plane, scale, 12 B per pixel staged in LDS and streamed out element-contiguous,
//                                    zero padding included
// and the result is bit for bit image.hip's: both take the value maps, the bilinear cell and the reduction trees from
// image_math.hip.h (-ffp-contract=off).
//   * The mean's reduction order is image.hip's: IMG_PARTS partials, block b takes elements b*256 + t with stride
//     65536, then the LDS tree; blockIdx.x plays the part of the single-image launch's block index.  For a rotated item the
//     index space is h' * w' * 3 with the channel innermost, as wssdl_image_adjust_f64 sees it.
//   * min / max are exact in any order.  The clip range of a warp is the min / max of its input; every step from the
//     u8 value (or from the rotated value) to the resize's input is monotone -- /255, +delta, clip, -mean, *factor
//     (non-increasing for a factor < 0), +mean, clip, -pixel_mean/255, each rounding included -- so the extremes of the
//     resize's input are the images of the extremes of the plane, whichever way round.
//   * Every gather is bounded: a tap outside the view takes cval (get_pixel2d, mode 'constant'; the taps here read
//     u8 or the rotated plane, so they are not image.hip's warp_pixel).
#include "image_math.hip.h"

namespace wssdl {

constexpr int IB_CHUNK_PIXELS = 86;            // pixels that 256 consecutive channel-innermost elements can touch
constexpr size_t IB_STATS1 = IMG_PARTS * (sizeof(double) + 2 * sizeof(int));      // per image: sums, (min, max) u8
constexpr size_t IB_STATS2 = IMG_PARTS * 3 * sizeof(double);                      // per image: sums, min, max f64

typedef wssdl_image_batch_item Item;

struct View { const unsigned char *p; int h, w; };

// the pixels the UNROTATED path works on: the crop of the flipped image as a view of the unflipped plane
__device__ __forceinline__ View crop_view(const unsigned char *arena, const Item &it) {
    View v;
    v.p = arena + it.offset;  v.h = it.h;  v.w = it.w;
    if (it.use_crop && !it.use_rotation) {
        v.p += (size_t)it.crop_u * it.row_stride + (it.flipped ? it.crop_r : it.crop_l);
        v.h = it.h - it.crop_u - it.crop_d;
        v.w = it.w - it.crop_l - it.crop_r;
    }
    return v;
}

// image_prep_kernel's map of one u8 value, as the double the resize reads
__device__ __forceinline__ double pre_u8(int u, const Item &it, float mm, double mean_sub) {
    return (double)prep_pixel((unsigned char)u, it.use_brightness, (float)it.brightness_delta, it.use_contrast,
                              (float)it.contrast_factor, mm, mean_sub);
}

// image_adjust_f64_kernel's map of one rotated value
__device__ __forceinline__ double pre_f64(double v, const Item &it, double mm, double mean_sub) {
    return adjust_pixel(v, it.use_brightness, it.brightness_delta, it.use_contrast, it.contrast_factor, mm, mean_sub);
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_batch_stats_kernel(const unsigned char *__restrict__ arena,
                                                                const Item *__restrict__ items,
                                                                double *__restrict__ sums, int *__restrict__ ext) {
    __shared__ double s[256];
    __shared__ int lo_s[256], hi_s[256];
    const Item it = items[blockIdx.y];
    const View v = crop_view(arena, it);                        // a rotated item: the whole plane (rotate()'s range)
    const int use_b = it.use_brightness;
    const float delta = (float)it.brightness_delta;
    const long long n = (long long)v.h * v.w;
    double acc = 0.0;
    int lo = 255, hi = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)IMG_PARTS * 256) {
        const int y = (int)(i / v.w), x = (int)(i - (long long)y * v.w);
        const unsigned char u = v.p[(size_t)y * it.row_stride + x];
        acc += (double)prep_value(u, use_b, delta);
        lo = min(lo, (int)u);
        hi = max(hi, (int)u);
    }
    s[threadIdx.x] = acc;  lo_s[threadIdx.x] = lo;  hi_s[threadIdx.x] = hi;
    __syncthreads();
    tree_sum_minmax256(s, lo_s, hi_s);
    if (threadIdx.x == 0) {
        const size_t k = (size_t)blockIdx.y * IMG_PARTS + blockIdx.x;
        sums[k] = s[0];
        ext[2 * k] = lo_s[0];
        ext[2 * k + 1] = hi_s[0];
    }
}

// the u8 extremes of image `img` from pass 1's partials (every thread gets them)
__device__ __forceinline__ void reduce_ext(const int *__restrict__ ext, int img, int *lo_s, int *hi_s, int &lo, int &hi) {
    const size_t k = (size_t)img * IMG_PARTS + threadIdx.x;
    lo_s[threadIdx.x] = ext[2 * k];
    hi_s[threadIdx.x] = ext[2 * k + 1];
    __syncthreads();
    tree_minmax256(lo_s, hi_s);
    lo = lo_s[0];  hi = hi_s[0];
    __syncthreads();
}

// ---- pass 2: rotated items ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_batch_rotate_kernel(const unsigned char *__restrict__ arena,
                                                                 const Item *__restrict__ items,
                                                                 const int *__restrict__ ext,
                                                                 double *__restrict__ sums2, double *__restrict__ planes) {
    __shared__ double s[256], dlo_s[256], dhi_s[256], pix_s[IB_CHUNK_PIXELS];
    __shared__ int lo_s[256], hi_s[256];
    const Item it = items[blockIdx.y];
    if (!it.use_rotation) return;
    int ulo, uhi;
    reduce_ext(ext, blockIdx.y, lo_s, hi_s, ulo, uhi);
    // rotate()'s clip range: the extremes of the f32 plane u / 255
    const double clo = (double)u8_unit((unsigned char)ulo), chi = (double)u8_unit((unsigned char)uhi);
    const double cval = it.cval;
    const bool keep_cval = !(clo <= cval && cval <= chi);
    const unsigned char *g = arena + it.offset;
    const int H0 = it.h, W0 = it.w;
    const int cu = it.use_crop ? it.crop_u : 0, cl = it.use_crop ? it.crop_l : 0;
    const int vh = it.use_crop ? H0 - it.crop_u - it.crop_d : H0, vw = it.use_crop ? W0 - it.crop_l - it.crop_r : W0;
    const int wc = vw * 3;
    const long long n = (long long)vh * wc;
    double *plane = planes + it.rot_offset;
    const long long npix = (long long)vh * vw;
    double acc = 0.0, lo = INFINITY, hi = -INFINITY;
    // block b owns elements e0 + t of adjust's index space (e0 = b*256, stride 65536), channel innermost: element e
    // belongs to pixel e / 3.  The <= 86 pixels of a chunk are rotated ONCE each (threads 0 .. 85) and handed to the
    // threads that own their elements through LDS, so every thread adds the addends image_sum_f64_kernel gives it, in
    // its order.
    for (long long e0 = (long long)blockIdx.x * 256; e0 < n; e0 += (long long)IMG_PARTS * 256) {
        const long long P0 = e0 / 3, P = P0 + threadIdx.x;
        if (threadIdx.x < IB_CHUNK_PIXELS && P < npix) {
            const int y = (int)(P / vw), px = (int)(P - (long long)y * vw);
            const double x = (double)(cl + px), yy0 = (double)(cu + y);
            double xx = it.inv_map[0] * x;  xx = xx + it.inv_map[1] * yy0;  xx = xx + it.inv_map[2];
            double yy = it.inv_map[3] * x;  yy = yy + it.inv_map[4] * yy0;  yy = yy + it.inv_map[5];
            double zz = it.inv_map[6] * x;  zz = zz + it.inv_map[7] * yy0;  zz = zz + it.inv_map[8];
            const Cell q = warp_cell(xx / zz, yy / zz);
            double p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long r = (k & 2) ? q.maxr : q.minr, c = (k & 1) ? q.maxc : q.minc;
                double tv = cval;
                if (r >= 0 && r < H0 && c >= 0 && c < W0) {
                    const int sx = it.flipped ? W0 - 1 - (int)c : (int)c;
                    tv = (double)u8_unit(g[(size_t)r * it.row_stride + sx]);
                }
                p[k] = tv;
            }
            double v = warp_mix(q, p[0], p[1], p[2], p[3]);
            if (!(keep_cval && v == cval)) v = fmin(fmax(v, clo), chi);
            pix_s[threadIdx.x] = v;
            if (3 * P >= e0) plane[P] = v;                      // a pixel cut by the chunk's start belongs to the chunk before
        }
        __syncthreads();
        const long long i = e0 + threadIdx.x;
        if (i < n) {
            const double v = pix_s[(int)(i / 3 - P0)];
            acc += adjust_value(v, it.use_brightness, it.brightness_delta);
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
        __syncthreads();
    }
    s[threadIdx.x] = acc;  dlo_s[threadIdx.x] = lo;  dhi_s[threadIdx.x] = hi;
    __syncthreads();
    tree_sum_minmax256(s, dlo_s, dhi_s);
    if (threadIdx.x == 0) {
        double *o = sums2 + (size_t)blockIdx.y * 3 * IMG_PARTS;
        o[blockIdx.x] = s[0];
        o[IMG_PARTS + blockIdx.x] = dlo_s[0];
        o[2 * IMG_PARTS + blockIdx.x] = dhi_s[0];
    }
}

// ---- pass 3 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_batch_blob_kernel(const unsigned char *__restrict__ arena,
                                                               const Item *__restrict__ items,
                                                               const double *__restrict__ sums,
                                                               const int *__restrict__ ext,
                                                               const double *__restrict__ sums2,
                                                               const double *__restrict__ planes, int Hmax, int Wmax,
                                                               float *__restrict__ blob) {
    __shared__ double s[256], dlo_s[256], dhi_s[256];
    __shared__ int lo_s[256], hi_s[256];
    __shared__ double table[256];
    __shared__ float out_s[256];
    const Item it = items[blockIdx.y];
    const double mean_sub = it.pixel_mean / 255.0;
    const int rot = it.use_rotation;
    const View v = crop_view(arena, it);
    const int vh = rot && it.use_crop ? it.h - it.crop_u - it.crop_d : v.h;
    const int vw = rot && it.use_crop ? it.w - it.crop_l - it.crop_r : v.w;
    const double *plane = planes + (rot ? it.rot_offset : 0);
    double lo, hi, mm64 = 0.0;
    if (!rot) {
        // every block re-reduces the partials in image.hip's order, then tabulates the pre-resize map of a u8 value
        s[threadIdx.x] = sums[(size_t)blockIdx.y * IMG_PARTS + threadIdx.x];
        int ulo, uhi;
        reduce_ext(ext, blockIdx.y, lo_s, hi_s, ulo, uhi);      // (its first barrier publishes s[] too)
        tree_sum256(s);
        const float mm = it.use_contrast ? (float)(s[0] / (double)((long long)vh * vw)) : 0.0f;
        table[threadIdx.x] = pre_u8((int)threadIdx.x, it, mm, mean_sub);
        __syncthreads();
        const double a = table[ulo], b = table[uhi];
        lo = fmin(a, b);  hi = fmax(a, b);
    } else {
        const double *p2 = sums2 + (size_t)blockIdx.y * 3 * IMG_PARTS;
        s[threadIdx.x] = p2[threadIdx.x];
        dlo_s[threadIdx.x] = p2[IMG_PARTS + threadIdx.x];
        dhi_s[threadIdx.x] = p2[2 * IMG_PARTS + threadIdx.x];
        __syncthreads();
        tree_sum_minmax256(s, dlo_s, dhi_s);
        if (it.use_contrast) mm64 = s[0] / (double)((long long)vh * (vw * 3));
        const double a = pre_f64(dlo_s[0], it, mm64, mean_sub), b = pre_f64(dhi_s[0], it, mm64, mean_sub);
        lo = fmin(a, b);  hi = fmax(a, b);
    }
    const bool keep_cval = !(lo <= 0.0 && 0.0 <= hi);            // resize(): mode 'constant', cval 0
    // wssdl_image_resize's inverse map (zz == 1: the division is exact)
    const int rows = it.rows, cols = it.cols;
    double m0 = 1.0, m2 = 0.0, m4 = 1.0, m5 = 0.0;
    if (rows == 1 && cols == 1) {
        m2 = (double)vw / 2.0 - 0.5;
        m5 = (double)vh / 2.0 - 0.5;
    } else {
        const double rs = (double)vh / (double)rows, cs = (double)vw / (double)cols;
        m0 = cs;  m2 = cs * 0.5 - 0.5;
        m4 = rs;  m5 = rs * 0.5 - 0.5;
    }
    const double scale = it.scale;
    const int divide = it.divide, flipped = it.flipped, stride = it.row_stride;
    float *out = blob + (size_t)blockIdx.y * Hmax * Wmax * 3;
    const long long n = (long long)Hmax * Wmax;
    // a block computes 256 consecutive pixels, one per thread, and streams their 768 floats out element-contiguous
    // (lane l of a store writes float l: whole 256-byte lines per wave instead of one float in three)
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        const int y = (int)(i / Wmax), x = (int)(i - (long long)y * Wmax);
        float o = 0.0f;
        if (i < n && y < rows && x < cols) {
            double xx = m0 * (double)x;  xx = xx + m2;
            double yy = m4 * (double)y;  yy = yy + m5;
            const Cell q = warp_cell(xx, yy);
            double p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long r = (k & 2) ? q.maxr : q.minr, c = (k & 1) ? q.maxc : q.minc;
                double t = 0.0;
                if (r >= 0 && r < vh && c >= 0 && c < vw) {
                    if (rot) {
                        t = pre_f64(plane[(size_t)r * vw + (size_t)c], it, mm64, mean_sub);
                    } else {
                        const int sx = flipped ? vw - 1 - (int)c : (int)c;
                        t = table[v.p[(size_t)r * stride + sx]];
                    }
                }
                p[k] = t;
            }
            double val = warp_mix(q, p[0], p[1], p[2], p[3]);
            if (!(keep_cval && val == 0.0)) val = fmin(fmax(val, lo), hi);
            o = (float)(divide ? val / scale : val * scale);
        }
        out_s[threadIdx.x] = o;
        __syncthreads();
        const long long left = (n - base) * 3;                   // floats of this chunk inside the image
        float *dst = out + (size_t)base * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = k * 256 + (int)threadIdx.x;
            if (e < left) dst[e] = out_s[e / 3];
        }
        __syncthreads();
    }
}

static bool finite_all(const double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.0)) return false;
    return true;
}

}  // namespace wssdl

using namespace wssdl;

extern "C" size_t wssdl_image_batch_workspace_bytes(int n_images, int64_t rotated_pixels) {
    if (n_images < 1 || rotated_pixels < 0) return 0;
    return (size_t)n_images * (IB_STATS1 + IB_STATS2) + (size_t)rotated_pixels * sizeof(double);
}

extern "C" int wssdl_image_batch_blob(const uint8_t *arena, size_t arena_bytes, const wssdl_image_batch_item *items_host,
                                      const wssdl_image_batch_item *items_dev, int n_images, int Hmax, int Wmax,
                                      float *blob, void *workspace, size_t workspace_bytes, wssdl_stream_t stream) {
    if (n_images < 1 || n_images > 65535 || Hmax < 1 || Wmax < 1) return WSSDL_ERR_INVALID_ARGUMENT;
    if (!arena || !items_host || !items_dev || !blob) return WSSDL_ERR_INVALID_ARGUMENT;
    int64_t rotated = 0;
    for (int i = 0; i < n_images; ++i) {
        const wssdl_image_batch_item &it = items_host[i];
        if (it.h < 1 || it.w < 1 || it.row_stride < it.w || it.rows < 1 || it.cols < 1) return WSSDL_ERR_INVALID_ARGUMENT;
        if (it.rows > Hmax || it.cols > Wmax || it.scale == 0.0) return WSSDL_ERR_INVALID_ARGUMENT;
        if (it.offset < 0 || (uint64_t)it.offset > arena_bytes) return WSSDL_ERR_INVALID_ARGUMENT;
        const uint64_t extent = (uint64_t)(it.h - 1) * (uint64_t)it.row_stride + (uint64_t)it.w;
        if (extent > arena_bytes - (uint64_t)it.offset) return WSSDL_ERR_INVALID_ARGUMENT;
        int64_t vh = it.h, vw = it.w;
        if (it.use_crop) {
            if (it.crop_u < 0 || it.crop_d < 0 || it.crop_l < 0 || it.crop_r < 0) return WSSDL_ERR_INVALID_ARGUMENT;
            vh -= (int64_t)it.crop_u + it.crop_d;
            vw -= (int64_t)it.crop_l + it.crop_r;
            if (vh < 1 || vw < 1) return WSSDL_ERR_INVALID_ARGUMENT;
        }
        const double scalars[5] = {it.brightness_delta, it.contrast_factor, it.pixel_mean, it.scale, it.cval};
        if (!finite_all(scalars, 5)) return WSSDL_ERR_INVALID_ARGUMENT;
        if (it.use_rotation) {
            if (!finite_all(it.inv_map, 9) || it.rot_offset != rotated) return WSSDL_ERR_INVALID_ARGUMENT;
            rotated += vh * vw;
        }
    }
    const size_t need = wssdl_image_batch_workspace_bytes(n_images, rotated);
    if (!workspace || workspace_bytes < need) return WSSDL_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    double *sums = reinterpret_cast<double *>(ws);
    int *ext = reinterpret_cast<int *>(ws + (size_t)n_images * IMG_PARTS * sizeof(double));
    double *sums2 = reinterpret_cast<double *>(ws + (size_t)n_images * IB_STATS1);
    double *planes = reinterpret_cast<double *>(ws + (size_t)n_images * (IB_STATS1 + IB_STATS2));
    hipLaunchKernelGGL(image_batch_stats_kernel, dim3(IMG_PARTS, n_images), dim3(256), 0, st, arena, items_dev, sums, ext);
    if (rotated > 0)
        hipLaunchKernelGGL(image_batch_rotate_kernel, dim3(IMG_PARTS, n_images), dim3(256), 0, st, arena, items_dev, ext,
                           sums2, planes);
    const long long n = (long long)Hmax * Wmax;
    const int blocks = (int)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
    hipLaunchKernelGGL(image_batch_blob_kernel, dim3(blocks, n_images), dim3(256), 0, st, arena, items_dev, sums, ext,
                       sums2, planes, Hmax, Wmax, blob);
    return check_launch();
}
