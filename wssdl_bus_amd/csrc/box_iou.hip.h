// The f64 pair arithmetic of the box-overlap kernels (bbox_overlaps.hip, proposal_recall.hip).
//
// Reference: code/lib/utils/bbox.pyx:15-55, code/lib/utils/bbox_ui.pyx:12-47.  All-double arithmetic in the
// reference's operation order; with -ffp-contract=off and IEEE division the results are bit-identical to the
// Cython kernels.  One definition: every kernel that needs an overlap includes this file.
#pragma once

#include "common.hip.h"

namespace wssdl {

__device__ __forceinline__ double iou_pair(double bx1, double by1, double bx2, double by2,
                                           double qx1, double qy1, double qx2, double qy2,
                                           double qarea) {
    double iw = fmin(bx2, qx2) - fmax(bx1, qx1) + 1;
    if (iw > 0) {
        double ih = fmin(by2, qy2) - fmax(by1, qy1) + 1;
        if (ih > 0) {
            double ua = (bx2 - bx1 + 1) * (by2 - by1 + 1) + qarea - iw * ih;
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
