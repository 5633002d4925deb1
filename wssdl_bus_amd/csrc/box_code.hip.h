// The box coding statements of the reference, one definition each: decode + clip (proposal.hip,
// decode_detect.hip) and the target encode (anchor_target.hip, roi_targets.hip).
//
// Reference: code/lib/fast_rcnn/bbox_transform.py:10-28 (bbox_transform), :30-61 (bbox_transform_inv),
// :63-77 (clip_boxes).  NumPy's operation order with every operation rounded on its own (-ffp-contract=off):
// separate multiply and add, IEEE division, exp and log evaluated in f64 and rounded once.  One definition: every
// kernel that decodes or encodes a box includes this file (tests/decode_reference.py and
// tests/boxcode_reference.py state the same lines in NumPy).
#pragma once

#include "common.hip.h"

namespace wssdl {

typedef float float4v __attribute__((ext_vector_type(4)));

// size = x2 - x1 + 1.0 and centre = x1 + 0.5 * size of one axis (:11-19, :36-39), each statement rounded in T
template <typename T>
__device__ __forceinline__ void box_centre_size(T x1, T x2, T &size, T &centre) {
    T s = x2 - x1;
    s = s + (T)1.0;
    const T half = (T)0.5 * s;
    size = s;
    centre = x1 + half;
}

// bbox_transform_inv of one f32 box and its four deltas (:36-59): the corners, not yet clipped
__device__ __forceinline__ float4v decode_box_f32(float x1, float y1, float x2, float y2, float4v d) {
    float w, h, cx, cy;
    box_centre_size(x1, x2, w, cx);
    box_centre_size(y1, y2, h, cy);
    float pcx = d.x * w;  pcx = pcx + cx;
    float pcy = d.y * h;  pcy = pcy + cy;
    const float pw = (float)exp((double)d.z) * w;
    const float ph = (float)exp((double)d.w) * h;
    const float hpw = 0.5f * pw, hph = 0.5f * ph;
    float4v o;
    o.x = pcx - hpw;  o.y = pcy - hph;  o.z = pcx + hpw;  o.w = pcy + hph;
    return o;
}

// clip_boxes (:63-77): max(min(v, im - 1), 0) with xmax = im_w - 1, ymax = im_h - 1
__device__ __forceinline__ float4v clip_box_f32(float4v b, float xmax, float ymax) {
    b.x = fmaxf(fminf(b.x, xmax), 0.0f);
    b.y = fmaxf(fminf(b.y, ymax), 0.0f);
    b.z = fmaxf(fminf(b.z, xmax), 0.0f);
    b.w = fmaxf(fminf(b.w, ymax), 0.0f);
    return b;
}

// bbox_transform of one example box against one f32 gt box (:10-28), rounded to f32 once per target.  The gt side
// stays f32 until it meets the example side (:16-19).  E = float: f32 operands on both sides
// (proposal_target_layer_tf_bus.py:220); E = double: f64 anchors, every mixed operation in f64
// (anchor_target_layer_tf_bus.py:652).  The two precisions differ in the reference and stay apart here.
template <typename E>
__device__ __forceinline__ float4v encode_box(E ex1, E ey1, E ex2, E ey2, float gx1, float gy1, float gx2, float gy2) {
    E ew, eh, ecx, ecy;
    box_centre_size(ex1, ex2, ew, ecx);
    box_centre_size(ey1, ey2, eh, ecy);
    float gw, gh, gcx, gcy;
    box_centre_size(gx1, gx2, gw, gcx);
    box_centre_size(gy1, gy2, gh, gcy);
    float4v t;
    t.x = (float)(((E)gcx - ecx) / ew);
    t.y = (float)(((E)gcy - ecy) / eh);
    t.z = (float)log((double)((E)gw / ew));
    t.w = (float)log((double)((E)gh / eh));
    return t;
}

}  // namespace wssdl
