// The f64 pair arithmetic of every kernel that needs a box overlap (bbox_overlaps.hip, proposal_recall.hip,
// anchor_target.hip, roi_targets.hip).
//
// Reference: code/lib/utils/bbox.pyx:15-55, code/lib/utils/bbox_ui.pyx:12-47.  All-double arithmetic in the
// reference's operation order; with -ffp-contract=off and IEEE division the results are bit-identical to the
// Cython kernels.  One definition: every kernel that needs an overlap includes this file.  (The NMS rule of
// nms.hip.h and the evaluation overlap of eval_detect.hip are other statements: cpu_nms's and voc_eval's.)
#pragma once

#include "common.hip.h"

namespace wssdl {

// (x2 - x1 + 1) * (y2 - y1 + 1), bbox.pyx:34-37, :49-52, bbox_ui.pyx:30-33
__device__ __forceinline__ double box_area_f64(double x1, double y1, double x2, double y2) {
    return (x2 - x1 + 1) * (y2 - y1 + 1);
}

__device__ __forceinline__ double iou_pair(double bx1, double by1, double bx2, double by2,
                                           double qx1, double qy1, double qx2, double qy2,
                                           double qarea) {
    double iw = fmin(bx2, qx2) - fmax(bx1, qx1) + 1;
    if (iw > 0) {
        double ih = fmin(by2, qy2) - fmax(by1, qy1) + 1;
        if (ih > 0) {
            double ua = box_area_f64(bx1, by1, bx2, by2) + qarea - iw * ih;
            return iw * ih / ua;
        }
    }
    return 0.0;
}

__device__ __forceinline__ double ui_pair(double bx1, double by1, double bx2, double by2,
                                          double barea, double qx1, double qy1, double qx2,
                                          double qy2) {
    double iw = fmin(bx2, qx2) - fmax(bx1, qx1) + 1;
    if (iw > 0) {
        double ih = fmin(by2, qy2) - fmax(by1, qy1) + 1;
        if (ih > 0) return iw * ih / barea;
    }
    return 0.0;
}

}  // namespace wssdl
