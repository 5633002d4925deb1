// Decode and clip of the head's class-wise boxes for gfx950 (MI355X): the step between a forward's layers and the
// post-detection op, for all images of a batch in one launch.
//
// Reference: code/lib/fast_rcnn/train_bus.py:456-457 / :821-822 (the validation loop: rois[:, 1:5] / scale,
// clip_boxes(bbox_transform_inv(boxes, bbox_pred), im.shape)), fast_rcnn/bbox_transform.py:30-61
// (bbox_transform_inv), :63-77 (clip_boxes).
//
// One lane per (row, class) pair, grid-stride: lane p reads the 16 bytes deltas[4p .. 4p+3] -- a coalesced dwordx4
// stream, like the proposal decode -- and the five floats of its RoI row (K neighbouring lanes share them: one cache
// line), and writes the 16 bytes boxes[4p .. 4p+3].  At most a few thousand pairs: the launch is latency-bound, so
// there is no LDS, no knob and no second form.
//
// All arithmetic is f32 in NumPy's operation order, every operation rounded on its own (-ffp-contract=off): a true
// IEEE division by the scale (the reference divides; PyTorch's GPU division by a scalar multiplies by a reciprocal),
// separate multiply and add, and exp evaluated in f64 and rounded once to f32 -- the decode and the clip are
// box_code.hip.h's, the proposal layer's own.  That makes the output derivable bit for bit from the inputs (tests/decode_reference.py) wherever the f64 exp is not
// within a few ulps of an f32 rounding boundary.
#include "box_code.hip.h"

namespace wssdl {

constexpr int DECODE_BLOCK = 256;
constexpr int DECODE_MAX_BLOCKS = 1024;        // 4 blocks per CU; beyond that the lanes stride

__global__ __launch_bounds__(DECODE_BLOCK) void decode_detections_kernel(
        const float *__restrict__ rois, const float *__restrict__ deltas, long long pairs, int K,
        const float *__restrict__ im_info, int info_stride, int n_images, const float *__restrict__ bounds,
        float *__restrict__ boxes) {
    const long long step = (long long)gridDim.x * DECODE_BLOCK;
    for (long long p = (long long)blockIdx.x * DECODE_BLOCK + threadIdx.x; p < pairs; p += step) {
        const long long r = p / K;
        const float *roi = rois + (size_t)r * 5;
        const float fi = roi[0];
        float4v out = {0.0f, 0.0f, 0.0f, 0.0f};
        // (int)fi in [0, n_images), tested before the conversion: NaN and values no int holds are dead rows too
        if ((double)fi > -1.0 && (double)fi < (double)n_images) {
            const int i = (int)fi;
            const float *info = im_info + (size_t)i * info_stride;
            const float s = info[2];
            const float bx1 = roi[1] / s, by1 = roi[2] / s, bx2 = roi[3] / s, by2 = roi[4] / s;
            float xmax, ymax;
            if (bounds) {
                xmax = bounds[(size_t)i * 2];
                ymax = bounds[(size_t)i * 2 + 1];
            } else {
                xmax = (float)((double)info[1] / (double)s - 1.0);
                ymax = (float)((double)info[0] / (double)s - 1.0);
            }
            const float4v d = *reinterpret_cast<const float4v *>(deltas + (size_t)p * 4);
            // bbox_transform_inv + clip_boxes (box_code.hip.h)
            out = clip_box_f32(decode_box_f32(bx1, by1, bx2, by2, d), xmax, ymax);
        }
        *reinterpret_cast<float4v *>(boxes + (size_t)p * 4) = out;
    }
}

}  // namespace wssdl

using namespace wssdl;

extern "C" int wssdl_decode_detections(const float *rois, const float *deltas, int R, int num_classes,
                                       const float *im_info, int info_stride, int n_images, const float *bounds,
                                       float *boxes, wssdl_stream_t stream) {
    if (R < 0 || num_classes < 2 || num_classes > 65 || n_images < 1 || info_stride < 3) return WSSDL_ERR_INVALID_ARGUMENT;
    if (R == 0) return WSSDL_OK;
    if (!rois || !deltas || !im_info || !boxes) return WSSDL_ERR_INVALID_ARGUMENT;
    // the pairs move as 16-byte vectors
    if ((reinterpret_cast<uintptr_t>(deltas) | reinterpret_cast<uintptr_t>(boxes)) & 15) return WSSDL_ERR_INVALID_ARGUMENT;
    const long long pairs = (long long)R * num_classes;
    const long long blocks = (pairs + DECODE_BLOCK - 1) / DECODE_BLOCK;
    const int grid = (int)(blocks < DECODE_MAX_BLOCKS ? blocks : DECODE_MAX_BLOCKS);
    hipLaunchKernelGGL(decode_detections_kernel, dim3(grid), dim3(DECODE_BLOCK), 0, as_stream(stream), rois, deltas, pairs,
                       num_classes, im_info, info_stride, n_images, bounds, boxes);
    return check_launch();
}
