// What the test-path ops over the views of an image share (post_detect.hip: wssdl_post_detections_views; soft_nms.hip:
// wssdl_post_detections_soft): the run of every output image in the RoI blob, the output image of a row, the
// un-mirror step and the limits of the batched form.  One definition each: both files include this one.
#pragma once
#include "common.hip.h"

namespace wssdl {

constexpr int POST_MAX_VIEWS = 8;

// Limits of the batched form: the segments' rows are 32-bit item numbers of one select (<= 2^24), and the ranking
// and mask grids put the segments on a grid dimension of at most 65535 blocks.
constexpr long long POST_MAX_ITEMS = 1LL << 24;
constexpr long long POST_MAX_SEGMENTS = 65535;

// (start, count) of image img's rows: its run [lo, hi] in the blob, or rows 0 .. R-1 without a blob (lo == NULL)
__device__ __forceinline__ void image_rows(const int *__restrict__ lo, const int *__restrict__ hi, int img, int R,
                                           int &start, int &count) {
    if (!lo) {
        start = 0;
        count = R;
        return;
    }
    const int l = lo[img], h = hi[img];
    start = h >= 0 ? l : 0;
    count = h >= 0 ? h - l + 1 : 0;
}

// output image of RoI row r and its source image: the batch index b in [0, n_images * views) -> b / views, src = b;
// -1 otherwise (dead padding rows, NaN, foreign images)
__device__ __forceinline__ int roi_view_image(const float *__restrict__ rois, int r, int n_images, int views, int &src) {
    const float b = rois[(size_t)r * 5];
    if (!(b >= 0.0f && b < (float)(n_images * views))) {
        src = -1;
        return -1;
    }
    src = (int)b;
    return src / views;
}

// a box of a mirrored source of original width w >= 0 in the image's own frame:
//   x1' = max((w - x2) - 1, 0),  x2' = (w - x1) - 1     (wssdl_flip_boxes's two f32 steps, then the clamp)
__device__ __forceinline__ void unmirror_x(float w, float &x1, float &x2) {
    if (w >= 0.0f) {
        float a = w - x2;  a = a - 1.0f;
        float e = w - x1;  e = e - 1.0f;
        x1 = fmaxf(a, 0.0f);
        x2 = e;
    }
}

// one workgroup: lo / hi [n_images] = the first and last row of every output image's run (INT_MAX / -1 without rows);
// post_detect.hip
int launch_post_view_segments(const float *rois, int R, int n_images, int views, int *lo, int *hi, hipStream_t st);

}  // namespace wssdl
