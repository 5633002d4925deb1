/*
 * wssdl_bus_hip.h -- C ABI of libwssdl_bus_hip.so, the MI355X (gfx950) implementation
 * of the wssdl_bus Faster-R-CNN detection hot path.
 *
 * Every entry point replaces one native/NumPy routine of the reference
 * (paths relative to code/lib of syshin1014/wssdl_bus, cited per function) and is
 * what the reference-side FFI for that routine would bind (INTEGRATION.md shows
 * the ctypes / tf.load_op_library-side stubs).
 *
 * Conventions
 *   - plain C: pointers and sizes only; no torch / HIP types in signatures.
 *     `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - all data pointers are DEVICE pointers unless the name ends in `_host`.
 *   - outputs and workspaces are caller-allocated (the PyTorch caching allocator
 *     in the shipped host layer); `*_workspace_bytes` functions size them.
 *   - nothing here allocates, frees, copies to host or synchronises: every call
 *     only enqueues kernels on `stream`, so calls are hipGraph-capturable.
 *   - return value: 0 = WSSDL_OK, otherwise a wssdl_status code; never exit(),
 *     never prints (the reference's CUDA launcher prints and exit(-1)s on a
 *     launch error, roi_pooling_op_gpu.cu.cc:102-107 -- deliberately not kept).
 *   - layouts are the reference's: feature maps NHWC f32, rois [R,5] f32
 *     (batch_idx,x1,y1,x2,y2), gt_boxes [N,MAX_GT,5] f32 (x1,y1,x2,y2,cls).
 */
#ifndef WSSDL_BUS_HIP_H
#define WSSDL_BUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *wssdl_stream_t;

#if defined(__GNUC__)
#define WSSDL_API __attribute__((visibility("default")))
#else
#define WSSDL_API
#endif

enum wssdl_status {
    WSSDL_OK = 0,
    WSSDL_ERR_INVALID_ARGUMENT = 1,   /* bad shape / null pointer / unsupported size */
    WSSDL_ERR_WORKSPACE = 2,          /* workspace too small */
    WSSDL_ERR_LAUNCH = 3              /* hipGetLastError() != hipSuccess after a launch */
};

/* bin-boundary rounding of RoI pooling */
enum wssdl_roi_rounding {
    WSSDL_ROI_ROUND_CUDA = 0,  /* floor(ph*bin), ceil((ph+1)*bin): roi_pooling_op_gpu.cu.cc:51-58 (canonical) */
    WSSDL_ROI_ROUND_CPU = 1    /* (int)(ph*bin), (int)((ph+1)*bin): roi_pooling_op.cc:167-170 */
};

/* wssdl_roi_pool_forward's N when the caller does not know the batch size (the reference's ROIPoolForwardLaucher,
 * roi_pooling_op_gpu.h:17-21): no range check of rois[:, 0] above zero.  N == 0 with RoIs to pool is an error. */
#define WSSDL_ROI_BATCH_UNKNOWN (-1)

/* dataset switch of the anchor-target layer, anchor_target_layer_tf_bus.py:120-199 */
enum wssdl_dataset {
    WSSDL_DATASET_SNUBH = 0,     /* gt holds positive boxes first, then background boxes */
    WSSDL_DATASET_SNUBH_FG = 1,  /* same layout, background boxes ignored */
    WSSDL_DATASET_FG_ONLY = 2    /* e.g. 'UDIAT': every gt box is a positive */
};

#define WSSDL_MAX_ANCHORS 32     /* base anchors per cell (reference uses 9 or 12) */
/* roi_counts[i] / num_keep of an image whose NMS sweep gave up waiting for the mask blocks of the fused
 * launch (50 ms without progress, tuning key "nms_wait_us": the GPU is held by another process or kernel).  The image's rows are
 * incomplete; every consumer must treat a negative count as an error, never as "no proposals". */
#define WSSDL_NMS_TIMED_OUT (-1)
#define WSSDL_MAX_GT 64          /* gt boxes per image (reference: MAX_GT_PER_IMAGE = 20) */

/* library / build identification: returns a static string */
WSSDL_API const char *wssdl_version(void);
/* name of the last HIP error seen by this library on the calling thread ("" if none) */
WSSDL_API const char *wssdl_last_error(void);
/* Tuning knobs.  The library never reads the environment: a knob is an int the caller sets (process
 * wide, read at call time).  Keys: "roi_bwd_plan" (plan id of the list-driven RoI-pool backward, -1 =
 * by launch size), "roi_fwd_variant",
 * "roi_bwdc_variant", "roi_bwd_cg" (shapes of the compact forward / the fallback backwards, 0 =
 * automatic), "nms_one_pass" (1: the proposal layer skips the probe pass), "nms_fused" (0: mask and sweep of a one-pass
 * NMS as two launches instead of the fused one), "topk_sort" (order of the proposal candidates: 1 sorted runs +
 * cross ranks, the default; 0 the select + sample sort), "nms_wait_us" (how long a sweep of the fused launch waits for
 * the mask blocks before it reports WSSDL_NMS_TIMED_OUT; default 50000), "roi_fwd_blocks" / "roi_fwd_blocks_sort" /
 * "roi_fwd_blocks_parts" (block-table forward, see there), "roi_fwd_one_bin" (forward launches of fewer than 32768 bin rows x
 * 256-channel slices: waves per bin row, 7 = one wave per bin, the default; 0 = the sliced kernel).  Results do not depend on
 * any of them.  One more key is a fault injector for tests, not a knob: "nms_fused_fault" (> 0: the fused
 * NMS launch withholds image 0's progress counts and that image's sweep gives up after this many microseconds,
 * reporting WSSDL_NMS_TIMED_OUT).  Unknown key -> WSSDL_ERR_INVALID_ARGUMENT. */
WSSDL_API int wssdl_set_tuning(const char *key, int value);
WSSDL_API int wssdl_get_tuning(const char *key, int *value_host);

/* ------------------------------------------------------------------ a1, a2 ---
 * generate_anchors: rpn_msr/generate_anchors.py:37-97.  Host-side (9 boxes);
 * writes n_ratios*n_scales rows of 4 doubles to anchors_host, ratio-major.
 * Returns the number of anchors, or a negative wssdl_status. */
WSSDL_API int wssdl_generate_anchors_host(int base_size, const double *ratios_host, int n_ratios,
                                const double *scales_host, int n_scales, double *anchors_host);

/* shifted anchor grid: anchor_target_layer_tf_bus.py:59-73 == proposal_layer_tf_bus.py:55-71.
 * out [H*W*A, 4] f64, row (h*W+w)*A+a = base[a] + stride*(w,h,w,h). */
WSSDL_API int wssdl_shifted_anchors(const double *base_anchors_host, int A, int H, int W, int feat_stride,
                          double *out, wssdl_stream_t stream);

/* ------------------------------------------------------------------ a3, a4 ---
 * bbox_overlaps: utils/bbox.pyx:15-55.  boxes [N, box_stride>=4] f64, query
 * [K, query_stride>=4] f64 (only columns 0..3 are read), out [N,K] f64.  Bit-exact. */
WSSDL_API int wssdl_bbox_overlaps(const double *boxes, int64_t N, int box_stride, const double *query,
                        int64_t K, int query_stride, double *out, wssdl_stream_t stream);
/* bbox_overlaps_ui: utils/bbox_ui.pyx:12-47 (intersection / area of boxes[n]). */
WSSDL_API int wssdl_bbox_overlaps_ui(const double *boxes, int64_t N, int box_stride, const double *query,
                           int64_t K, int query_stride, double *out, wssdl_stream_t stream);

/* ---------------------------------------------------------------------- a8 ---
 * nms: fast_rcnn/nms_wrapper.py:13-21 -> nms/cpu_nms.pyx:17-68.
 * dets [n,5] f32 (x1,y1,x2,y2,score), any order (sorted internally by score
 * descending; equal scores: higher input index first).  f32 box arithmetic,
 * suppression when (double)iou >= thresh -- the vendored build's rule.
 * keep [max_keep] i32 receives kept indices into dets in score order (the
 * reference's caller truncates keep[:post_nms_topN]; pass max_keep = n for
 * all); *num_keep (device i32) receives the count written.  n == 0 -> count 0. */
WSSDL_API size_t wssdl_nms_workspace_bytes(int n);
WSSDL_API int wssdl_nms(const float *dets, int n, double thresh, int max_keep, int32_t *keep,
              int32_t *num_keep, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
/* The test path's NMS is a second file with the same rule: utils/nms.pyx:17-68 `nms` (imported as
 * utils.cython_nms at fast_rcnn/test_bus.py:10, called at :293,366,375) == wssdl_nms.
 * nms_new: utils/nms.pyx:70-123 (imported at test_bus.py:10, never called by the reference): box j is also
 * suppressed when it lies almost inside the kept box i or the other way round,
 *   ovr >= thresh  or  (double)(inter / area_i) > 0.95  or  (double)(inter / area_j) > 0.95
 * (:118-121; ovr1 / ovr2 are untyped there, i.e. the f32 quotients widened to Python floats).
 * Same arguments, workspace and outputs as wssdl_nms. */
WSSDL_API int wssdl_nms_new(const float *dets, int n, double thresh, int max_keep, int32_t *keep,
              int32_t *num_keep, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);

/* ------------------------------------------------------------ a6, a7, a8, a9 ---
 * proposal_layer: rpn_msr/proposal_layer_tf_bus.py:19-148 for all N images in
 * one call.  rpn_cls_prob [N,H,W,2A] f32 (fg prob = channels A..2A-1),
 * rpn_bbox_pred [N,H,W,4A] f32, im_info [N,im_info_stride] f32 (h,w,scale,...).
 * Decode (bbox_transform_inv, f32) -> clip -> min-size filter -> sort by score
 * -> top pre_nms_topN -> NMS -> top post_nms_topN.
 * Outputs: rois_padded [N, post_nms_topN, 5] f32 (batch_idx,x1,y1,x2,y2; rows
 * beyond the image's count are zero), roi_counts [N] i32.  Optional (may be
 * NULL) debug outputs used by the parity tests: decoded [N,H*W*A,4] f32 (after
 * clip), sorted_index [N, pre_nms_topN] i32 (anchor index of each pre-NMS
 * candidate in score order, -1 padded), sorted_count [N] i32. */
WSSDL_API size_t wssdl_proposal_workspace_bytes(int N, int H, int W, int A, int pre_nms_topN);
WSSDL_API int wssdl_proposal_layer(const float *rpn_cls_prob, const float *rpn_bbox_pred,
                         const float *im_info, int im_info_stride, int N, int H, int W,
                         const double *base_anchors_host, int A, int feat_stride,
                         int pre_nms_topN, int post_nms_topN, double nms_thresh, float min_size,
                         float *rois_padded, int32_t *roi_counts,
                         float *decoded, int32_t *sorted_index, int32_t *sorted_count,
                         void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
/* f2: the same layer fed with the raw RPN class scores rpn_cls_score [N,H,W,2A] (logits):
 * the reshape -> softmax -> reshape chain in front of the layer (networks/network.py:283-291,
 * 398-404, Resnet_train_bus.py:76-81) is fused into the decode kernel: the fg probability of
 * anchor a is softmax(score[a], score[A+a])[1]. */
WSSDL_API int wssdl_proposal_layer_from_logits(const float *rpn_cls_score, const float *rpn_bbox_pred,
                         const float *im_info, int im_info_stride, int N, int H, int W,
                         const double *base_anchors_host, int A, int feat_stride,
                         int pre_nms_topN, int post_nms_topN, double nms_thresh, float min_size,
                         float *rois_padded, int32_t *roi_counts,
                         float *decoded, int32_t *sorted_index, int32_t *sorted_count,
                         void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
/* gathers the per-image lists into the reference's contiguous blob [sum counts, 5]
 * (proposal_layer_tf_bus.py:144-146).  total_host must equal sum(roi_counts). */
WSSDL_API int wssdl_proposal_compact(const float *rois_padded, const int32_t *roi_counts, int N,
                           int post_nms_topN, float *rois_out, int total_host,
                           wssdl_stream_t stream);

/* ---------------------------------------------------------------------- a5 ---
 * anchor-target layer, rpn_msr/anchor_target_layer_tf_bus.py:19-303 / :328-628,
 * split at the two random sub-samplings (:202-217) so that the host layer can
 * either draw them from numpy's legacy RandomState (bit-identical to the
 * reference) or let the device do it.
 *
 * Stage 1  wssdl_anchor_labels: for each of the first n_images images: inside
 *   filter (:100-105), f64 IoU vs positive gt / intersection ratio vs background
 *   gt, labels before sub-sampling (:115-199).
 *   labels_pre [n_images, H*W*A] i8 in anchor order (h,w,a): -1/0/1 (outside = -1)
 *   argmax_gt  [n_images, H*W*A] i32: row of gt_boxes the targets regress to (-1 outside)
 *   counts     [n_images, 4] i32: (#inside, #fg, #bg, 0)
 * Stage 2a wssdl_anchor_subsample_device: random sub-sampling on the device
 *   (counter-based hash of (seed, image, anchor); same distribution as
 *   npr.choice(replace=False), not the same stream).  In place on labels_pre.  Given stage 1's
 *   counts the fg and the bg draw of an image run side by side (the bg quota only needs #fg).
 * Stage 2b (reference RNG) happens on the host: see
 *   wssdl_bus_amd/rpn_msr/anchor_target_layer_tf_bus.py.
 * Stage 3  wssdl_anchor_targets: final labels -> the four output blobs
 *   (:219-299): rpn_labels [n_out,1,A*H,W] f32, bbox_targets / inside / outside
 *   weights [n_out,4A,H,W] f32.  Images n_images..n_out-1 are the all-ignore
 *   weak images of the joint layer (:613-626) / anchor_target_layer_ws (:306-325). */
WSSDL_API size_t wssdl_anchor_workspace_bytes(int n_images);
WSSDL_API int wssdl_anchor_labels(const float *gt_boxes, int max_gt, const int32_t *num_gt_boxes,
                        const float *im_info, int im_info_stride, int n_images, int H, int W,
                        const double *base_anchors_host, int A, int feat_stride, int dataset,
                        double positive_overlap, double negative_overlap, int clobber_positives,
                        int8_t *labels_pre, int32_t *argmax_gt, int32_t *counts,
                        void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API int wssdl_anchor_subsample_device(int8_t *labels, int n_images, int total_anchors,
                                  int rpn_batchsize, double fg_fraction, uint64_t seed,
                                  const int32_t *counts /* of stage 1, or NULL: fg then bg in sequence */,
                                  wssdl_stream_t stream);
WSSDL_API int wssdl_anchor_targets(const int8_t *labels, const int32_t *argmax_gt, const float *gt_boxes,
                         int max_gt, int n_images, int n_out, int H, int W,
                         const double *base_anchors_host, int A, int feat_stride,
                         const float *inside_weights_host /* [4] */, double positive_weight,
                         float *rpn_labels, float *bbox_targets, float *inside_w, float *outside_w,
                         wssdl_stream_t stream);

/* --------------------------------------------------------------------- a10 ---
 * proposal-target layer, rpn_msr/proposal_target_layer_tf_bus.py:15-295.
 * Stage 1  wssdl_roi_gt_assign: rois [R,5] f32 x positive gt of each roi's image:
 *   f64 IoU (utils/bbox.pyx), max_overlap [R] f64, assignment [R] i32 (row of
 *   gt_boxes of that image; first maximum, numpy argmax).  (:233-238)
 * Stage 2  sampling (:241-262): on the host with the reference's numpy stream, or
 *   wssdl_roi_sample_device: per image images[s] draw min(fg_rois_per_image, #fg)
 *   rows with max_overlap >= fg_thresh and min(rois_per_image - n_fg, #bg) rows with
 *   bg_thresh_lo <= max_overlap < bg_thresh_hi, uniformly without replacement
 *   (counter-based hash of (seed, image, row); same distribution as npr.choice,
 *   not the same stream).  The two pools are independent: when fg_thresh < bg_thresh_hi
 *   a row can be drawn once as fg and once as bg, as in the reference.  keep / is_fg [n_sample_images, rois_per_image]: rows of
 *   cand in candidate order, fg first, padded with -1; counts [n_sample_images, 2]
 *   = (n_fg, n_bg).  Rows of other images (batch index != images[s]) are ignored.
 * Stage 3  wssdl_roi_targets: for the kept rows: labels (bg clamped to 0, :265),
 *   bbox_transform in f32 (:220), expansion to 4*num_classes with inside/outside
 *   weights (:187-210, :89).  keep [n_keep] i32 indexes rois; is_fg [n_keep] u8.  A negative keep
 *   entry is a padding slot of a fixed-shape list (wssdl_roi_sample_device pads with -1 when an
 *   image runs short of candidates): its output row is (-1,0,0,0,0), label -1, zero targets and
 *   weights, so that consumers can run on the full shape without reading the counts back.
 *   normalize_host != NULL = cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED (:221-224): 8 host doubles, BBOX_NORMALIZE_MEANS
 *   then BBOX_NORMALIZE_STDS; targets = (f32 target - mean) / std evaluated in f64 and rounded to f32 once, as NumPy does
 *   when the f32 targets meet np.array(MEANS) / np.array(STDS). */
WSSDL_API int wssdl_roi_gt_assign(const float *rois, int R, const float *gt_boxes, int max_gt,
                        const int32_t *num_pos_boxes, int n_images, double *max_overlap,
                        int32_t *assignment, wssdl_stream_t stream);
/* Stage 0 (device path): candidate rows = rois [R,5] followed, when append_gt, by the max_gt gt
 *   slots of each image images[s] (:44-50); a slot's batch index is the image for its positive
 *   boxes (the first num_pos rows) and -1 otherwise.  cand [R + n_sample_images*max_gt, 5];
 *   num_pos_boxes [n_images] = boxes with class != 0 among the num_gt_boxes valid rows (:40-42). */
WSSDL_API int wssdl_roi_candidates(const float *rois, int R, const float *gt_boxes, int max_gt,
                         const int32_t *num_gt_boxes, int n_images, const int32_t *images,
                         int n_sample_images, int append_gt, float *cand, int32_t *num_pos_boxes,
                         wssdl_stream_t stream);
/* The device-sampled layer as one call: stages 0-3 (candidates, assignment, fg / bg draw, rows +
 *   targets) launched back to back, the intermediates carved from `workspace`
 *   (wssdl_proposal_target_device_workspace_bytes).  Outputs have the fixed shape
 *   n_sample_images * rois_per_image rows (rois_out [.,5], labels [.] f32, the three [., 4*num_classes]);
 *   an image that runs short of candidates leaves padding rows as described above. */
WSSDL_API size_t wssdl_proposal_target_device_workspace_bytes(int R, int n_images, int max_gt,
                                                    int n_sample_images, int rois_per_image, int append_gt);
WSSDL_API int wssdl_proposal_target_device(
    const float *rois, int R, const float *gt_boxes, int max_gt, const int32_t *num_gt_boxes, int n_images,
    const int32_t *images, int n_sample_images, int append_gt, int rois_per_image, int fg_rois_per_image,
    double fg_thresh, double bg_thresh_hi, double bg_thresh_lo, uint64_t seed, int num_classes,
    const float *inside_weights_host, const double *normalize_host, float *rois_out, float *labels, float *bbox_targets,
    float *inside_w, float *outside_w, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API int wssdl_roi_sample_device(const float *cand, const double *max_overlap, int Rc,
                            const int32_t *images, int n_sample_images, int rois_per_image,
                            int fg_rois_per_image, double fg_thresh, double bg_thresh_hi,
                            double bg_thresh_lo, uint64_t seed, int32_t *keep, uint8_t *is_fg,
                            int32_t *counts, wssdl_stream_t stream);
WSSDL_API int wssdl_roi_targets(const float *rois, const int32_t *keep, const uint8_t *is_fg, int n_keep,
                      const int32_t *assignment, const float *gt_boxes, int max_gt, int num_classes,
                      const float *inside_weights_host /* [4] */,
                      const double *normalize_host /* NULL, or means[4] then stds[4] */, float *rois_out,
                      float *labels, float *bbox_targets, float *inside_w, float *outside_w,
                      wssdl_stream_t stream);

/* ---------------------------------------------------------------- a11, a12 ---
 * RoiPool forward: roi_pooling_op.cc:31-52 (op), kernels roi_pooling_op_gpu.cu.cc:20-85
 * (rounding CUDA) / roi_pooling_op.cc:137-196 (rounding CPU).  N = WSSDL_ROI_BATCH_UNKNOWN (-1) = "batch size unknown": the
 * reference's ROIPoolForwardLaucher is not told it (roi_pooling_op_gpu.h:17-21) and never range-checks
 * rois[:, 0]; then only a negative batch index makes a RoI empty and the caller vouches for the rest (with N > 0 an
 * index >= N makes an empty RoI too; N == 0 with R > 0 returns WSSDL_ERR_INVALID_ARGUMENT).
 * bottom [N,H,W,C] f32, rois [R,5] f32, top [R,PH,PW,C] f32, argmax [R,PH,PW,C] i32
 * (flat NHWC index within the roi's image, -1 for an empty bin). */
WSSDL_API int wssdl_roi_pool_forward(const float *bottom, int N, int H, int W, int C, const float *rois,
                           int R, int pooled_h, int pooled_w, float spatial_scale, int rounding,
                           float *top, int32_t *argmax, wssdl_stream_t stream);
/* RoiPoolGrad: roi_pooling_op.cc:54-63 (op), roi_pooling_op_gpu.cu.cc:114-190 ==
 * roi_pooling_op.cc:383-458.  bottom_diff [N,H,W,C] f32 is fully written (no
 * pre-zeroing needed).  Deterministic: per element the f32 sum runs in the
 * reference's order roi^, ph^, pw^, so results are bit-identical to it. */
WSSDL_API int wssdl_roi_pool_backward(const float *top_diff, const int32_t *argmax, const float *rois,
                            int R, int N, int H, int W, int C, int pooled_h, int pooled_w,
                            float spatial_scale, float *bottom_diff, wssdl_stream_t stream);
/* The same op with a caller-owned workspace (wssdl_roi_pool_backward_workspace_bytes(R, N, H, W, pooled_h,
 * pooled_w); a TF launcher takes it from OpKernelContext::allocate_temp): the list-driven kernels of the training
 * path -- per (image, tile) the candidate bins in the reference's order, one wave per (image, tile, 128 channels)
 * -- reading the i32 arg-max.  Same bits as wssdl_roi_pool_backward; 1.4x faster on a train-sized RoI list (1.15 -> 0.80 ms).
 * Shapes the lists do not cover (C not a power of two, pooled size > 8, workspace NULL or short) run the kernel
 * of wssdl_roi_pool_backward. */
WSSDL_API int wssdl_roi_pool_backward_ws(const float *top_diff, const int32_t *argmax, const float *rois,
                            int R, int N, int H, int W, int C, int pooled_h, int pooled_w,
                            float spatial_scale, float *bottom_diff, void *workspace, size_t workspace_bytes,
                            wssdl_stream_t stream);

/* ------------------------------------------------- a11, a12: training path ---
 * The same pair with a ONE-BYTE arg-max.  In the reference the arg-max tensor never leaves the
 * op pair: networks/network.py:206-210 keeps only top_data and the registered gradient
 * (roi_pooling_op_grad.py:24-44) hands argmax straight to RoiPoolGrad, so its encoding is an
 * internal contract.  Both kernels are HBM-bound on top + argmax, and 4 + 1 bytes per element
 * instead of 4 + 4 is a 37 % cut of that traffic (re-reads of the backward included).
 *   code = (h - hstart) << 4 | (w - wstart)   within the bin's clipped window
 *          (roi_pooling_op_gpu.cu.cc:51-64 / roi_pooling_op.cc:167-176); 0xff = empty bin (-1).
 * Supported (wssdl_roi_pool_compact_supported == 1) when C % 32 == 0 and every window of a RoI
 * inside the map fits 15 x 16 cells: ceil((H+1)/pooled_h)+1 <= 15, ceil((W+1)/pooled_w)+1 <= 16
 * (7x7 bins: maps up to 97 x 104 cells).  A RoI reaching far outside the map can exceed that:
 * the forward then sets *overflow (optional device int32, OR-ed, never cleared) and that RoI's
 * codes are invalid -- callers feeding unclipped RoIs use the i32 pair above.
 * top / bottom_diff are bit-identical to the i32 pair; wssdl_roi_argmax_expand rebuilds the
 * reference's i32 argmax from the codes. */
WSSDL_API int wssdl_roi_pool_compact_supported(int H, int W, int C, int pooled_h, int pooled_w);
WSSDL_API int wssdl_roi_pool_forward_compact(const float *bottom, int N, int H, int W, int C,
                           const float *rois, int R, int pooled_h, int pooled_w, float spatial_scale,
                           int rounding, float *top, uint8_t *argmax8, int32_t *overflow,
                           wssdl_stream_t stream);
/* The same forward with the RoI geometry taken from a table: wssdl_roi_pool_forward_windows writes one
 * 32-byte entry per (roi, bin row) -- batch index, the clipped window rows, the window columns of the 7
 * bins (roi_pooling_op_gpu.cu.cc:36-64) -- and raises *overflow like the forward would;
 * wssdl_roi_pool_forward_compact_windows reads it with scalar loads instead of recomputing it in every
 * wave (~1/5 of the kernel's vector instructions).  7 x 7 bins, C % 256 == 0;
 * wssdl_roi_pool_forward_windows_bytes returns 0 for shapes it does not take (use the call above). */
WSSDL_API size_t wssdl_roi_pool_forward_windows_bytes(int R, int H, int W, int C, int pooled_h, int pooled_w);
WSSDL_API int wssdl_roi_pool_forward_windows(const float *rois, int R, int N, int H, int W, int C, int pooled_h,
                                   int pooled_w, float spatial_scale, int rounding, void *table,
                                   size_t table_bytes, int32_t *overflow, wssdl_stream_t stream);
WSSDL_API int wssdl_roi_pool_forward_compact_windows(const float *bottom, int N, int H, int W, int C,
                                           const float *rois, int R, int pooled_h, int pooled_w,
                                           float spatial_scale, int rounding, const void *table,
                                           float *top, uint8_t *argmax8, wssdl_stream_t stream);
/* The same forward for MANY proposals per image (large, heavily overlapping bin windows: the weak images' 2000
 * proposals each), where scanning every cell of every window (sum of window areas x C) is the cost.  Per call the
 * feature map is reduced once to block-maximum tables -- the first maximum, by the reference's own scan
 * (roi_pooling_op_gpu.cu.cc:66-79: (h, w) order, strict >), of the k x k block at every cell, k = 2, 3, 4 -- and a
 * bin whose window is covered by the four k x k blocks at its corners reads four table entries instead of its
 * cells; "maximum value, then smallest (h, w)" is associative and idempotent, so top and arg-max are the same bits.
 * Other bins (and every bin when the map holds a -0.0, which equals +0.0 in the reference's compare) are scanned
 * cell by cell.  Order of calls, same stream: wssdl_roi_pool_forward_windows_blocks (the window table -- it also
 * carries the block choice per bin and the sort key of the bin row -- and the counters of `blocks` cleared),
 * wssdl_roi_pool_forward_blocks_prepare (tables + the bin rows sorted by (image, first window row) so that an XCD's
 * L2 holds the band of the tables its waves read), wssdl_roi_pool_forward_compact_blocks.
 * `blocks` = wssdl_roi_pool_forward_blocks_bytes() bytes, 256-byte aligned (0: shape not supported -- 7 x 7 bins,
 * C % 256 == 0, H, W in 4..255).  wssdl_roi_pool_forward_blocks_auto = 1 where the library suggests this form for
 * the launch shape ("roi_fwd_blocks": -1 that rule, 0 never, 1 wherever supported; "roi_fwd_blocks_sort" = 0 keeps
 * the bin rows in RoI order; "roi_fwd_blocks_parts" = 1, 2 (default), 4 or 7 waves per bin row).  The order array is
 * only as good as the call sequence: built on counters that wssdl_roi_pool_forward_windows_blocks did not clear it is
 * not a permutation, and rows of `top` stay unwritten (its entries are clamped, so nothing is read out of range). */
WSSDL_API size_t wssdl_roi_pool_forward_blocks_bytes(int R, int N, int H, int W, int C, int pooled_h, int pooled_w);
WSSDL_API int wssdl_roi_pool_forward_blocks_auto(int R, int N, int H, int W, int C, int pooled_h, int pooled_w);
WSSDL_API int wssdl_roi_pool_forward_windows_blocks(const float *rois, int R, int N, int H, int W, int C, int pooled_h,
                                          int pooled_w, float spatial_scale, int rounding, void *table,
                                          size_t table_bytes, int32_t *overflow, void *blocks, size_t blocks_bytes,
                                          wssdl_stream_t stream);
WSSDL_API int wssdl_roi_pool_forward_blocks_prepare(const float *bottom, int N, int H, int W, int C, int R,
                                          int pooled_h, int pooled_w, const void *table, void *blocks,
                                          size_t blocks_bytes, wssdl_stream_t stream);
WSSDL_API int wssdl_roi_pool_forward_compact_blocks(const float *bottom, int N, int H, int W, int C, int R,
                                          int pooled_h, int pooled_w, const void *table, const void *blocks,
                                          size_t blocks_bytes, float *top, uint8_t *argmax8,
                                          wssdl_stream_t stream);
/* Backward in two calls.  The lists that drive it depend on the RoIs and the shapes only, so
 * wssdl_roi_pool_backward_prepare can run as soon as the RoIs exist (e.g. right behind the
 * forward): per (image, tile) it builds the stream of candidate bins in the reference's
 * summation order (roi, ph, pw) with the reference's in_roi / candidate-bin tests
 * (roi_pooling_op_gpu.cu.cc:141-151,169-177) evaluated once, and sorts the tiles by work.
 * It writes the plan it chose to *plan_host (a HOST int; -1 = not supported or no workspace:
 * the backward then runs a kernel that filters the RoIs itself).  wssdl_roi_pool_backward_compact
 * with that plan and the same workspace is then ONE kernel: one wave per (image, tile, 128
 * channels), heaviest tiles first.  workspace_bytes = 0 when the pooled size is not supported.
 * bottom_diff is bit-identical on every path. */
WSSDL_API size_t wssdl_roi_pool_backward_workspace_bytes(int R, int N, int H, int W, int pooled_h,
                            int pooled_w);
/* number of plans wssdl_roi_pool_backward_prepare can choose from ("roi_bwd_plan" = 0 .. count-1) */
WSSDL_API int wssdl_roi_pool_backward_plan_count(void);
/* byte offset, inside the workspace, of the int32[4] status block the prepare step fills:
 * [0] = 64-byte records in use, [1] = error flags (non-zero: the lists do not fit the workspace and
 * bottom_diff would be short -- cannot happen with wssdl_roi_pool_backward_workspace_bytes; the host
 * layer checks it with its other deferred flags). */
WSSDL_API size_t wssdl_roi_pool_backward_status_offset(int R, int N, int H, int W, int pooled_h, int pooled_w);
WSSDL_API int wssdl_roi_pool_backward_prepare(const float *rois, int R, int N, int H, int W, int C,
                            int pooled_h, int pooled_w, float spatial_scale, int rounding,
                            void *workspace, size_t workspace_bytes, int32_t *plan_host,
                            wssdl_stream_t stream);
WSSDL_API int wssdl_roi_pool_backward_compact(const float *top_diff, const uint8_t *argmax8,
                            const float *rois, int R, int N, int H, int W, int C, int pooled_h,
                            int pooled_w, float spatial_scale, int rounding, float *bottom_diff,
                            void *workspace, size_t workspace_bytes, int plan, wssdl_stream_t stream);
/* Split form of the list-driven backward: DETERMINISTIC BUT NOT BIT-ORDERED.  A launch with few images is bound
 * by the longest slot chain one wave walks alone (every RoI of a 2000-RoI weak image reaches the tiles at the
 * image's centre), not by bandwidth: each tile's stream is cut into `segments` pieces walked by separate waves
 * (segment 0 into bottom_diff, the others into scratch) and the pieces are added in segment order.  The f32 sum
 * per element is then associated differently from roi_pooling_op_gpu.cu.cc:132-186 (roi^, ph^, pw^): the same
 * result on every run, every element within 1e-6 of ..._backward_compact relative to its own sum of |terms|
 * (measured ~2e-8) and the tensor within 1e-5 of its scale (north_star's tolerance for RoI pooling), not
 * bit-identical to it.  segments = 1 is the exact walk.
 * wssdl_roi_pool_backward_split_segments suggests a count by launch shape (8; 4 for two images with 2048 and for
 * three images with up to 3072 (image, channel) pairs, where the gain is the larger tiles' fewer re-read bytes; or
 * 1 = keep the exact walk: more than 4 images, fewer than 1000 RoIs per image, or more (image, channel) pairs than
 * that -- enough waves that the chains no longer bind); wssdl_roi_pool_backward_split_plan = the plan to prepare the lists with for the split form
 * (set "roi_bwd_plan" to it around ..._backward_prepare: large tiles, since the chains no longer matter); same
 * workspace as ..._backward_compact. */
WSSDL_API int wssdl_roi_pool_backward_split_segments(int R, int N, int H, int W, int C);
WSSDL_API int wssdl_roi_pool_backward_split_plan(void);
WSSDL_API size_t wssdl_roi_pool_backward_split_scratch_bytes(int N, int H, int W, int C, int segments);
WSSDL_API int wssdl_roi_pool_backward_compact_split(const float *top_diff, const uint8_t *argmax8,
                            const float *rois, int R, int N, int H, int W, int C, int pooled_h,
                            int pooled_w, float spatial_scale, int rounding, float *bottom_diff,
                            void *workspace, size_t workspace_bytes, int plan, int segments,
                            void *scratch, size_t scratch_bytes, wssdl_stream_t stream);
/* Bin-owner form of the list-driven backward (round 5): DETERMINISTIC BUT NOT BIT-ORDERED, like the split form.
 * The exact walk lists a bin in every tile its window touches, so the launch reads top_diff / the codes ~1.5 x.  Here a
 * wave accumulates into a region that reaches past its tile (a halo of 1-3 cells) and a bin is listed once, by the tile
 * of its window's first cell (windows larger than the region continue in the next tile); the halos go to `scratch` and a
 * second kernel adds them to their owners in a fixed order (own, left, upper, upper-left).  Same result on every run;
 * the f32 sum per element is associated differently from roi_pooling_op_gpu.cu.cc:132-186, within the split form's
 * bounds.  Call ..._owner_prepare (instead of ..._backward_prepare; same workspace size) with the owner plan, then
 * ..._compact_owner with the same plan.  ..._owner_plan suggests a plan by launch shape, -1 = keep the exact walk. */
WSSDL_API int wssdl_roi_pool_backward_owner_plan_count(void);
WSSDL_API int wssdl_roi_pool_backward_owner_plan(int R, int N, int H, int W, int C);
/* the same rule for a given pooled size: -1 as well when the owner form does not take the launch (pooled_h or
 * pooled_w > 8, R * pooled_h * pooled_w * C >= 2^30 elements, N * H * W * C >= 2^31) -- what a caller that pools
 * other sizes than 7 x 7 must ask (wssdl_roi_pool_backward_owner_plan assumes 7 x 7) */
WSSDL_API int wssdl_roi_pool_backward_owner_plan_for(int R, int N, int H, int W, int C, int pooled_h, int pooled_w);
WSSDL_API size_t wssdl_roi_pool_backward_owner_scratch_bytes(int N, int H, int W, int C, int owner_plan);
WSSDL_API int wssdl_roi_pool_backward_owner_prepare(const float *rois, int R, int N, int H, int W, int C,
                            int pooled_h, int pooled_w, float spatial_scale, int rounding,
                            void *workspace, size_t workspace_bytes, int owner_plan, wssdl_stream_t stream);
WSSDL_API int wssdl_roi_pool_backward_compact_owner(const float *top_diff, const uint8_t *argmax8,
                            const float *rois, int R, int N, int H, int W, int C, int pooled_h,
                            int pooled_w, float spatial_scale, int rounding, float *bottom_diff,
                            void *workspace, size_t workspace_bytes, int owner_plan,
                            void *scratch, size_t scratch_bytes, wssdl_stream_t stream);
/* The owner form with SEGMENTS (round 6), for launches with few (image, channel) pairs -- the alternating weak step's two
 * images, the reference's default 1 + 2 batch -- where one wave per (image, tile, 128 channels) leaves most of the chip
 * waiting for the longest streams: a tile's stream is cut into `segments` pieces walked by a wave each, every piece into
 * a region buffer of its own ([segments][N * tiles][region cells][C] f32 = ..._owner_split_scratch_bytes), and a merge
 * pass writes bottom_diff = the sum over segments of own cells + neighbours' halos, in a fixed order.  Same lists
 * (wssdl_roi_pool_backward_owner_prepare), deterministic, the owner form's tolerance (every (bin, cell) pair applied
 * exactly once).  wssdl_roi_pool_backward_owner_segments suggests the count by launch shape (1 = the plain owner form);
 * "roi_bwd_owner_segments" overrides it. */
WSSDL_API int wssdl_roi_pool_backward_owner_segments(int R, int N, int H, int W, int C);
WSSDL_API size_t wssdl_roi_pool_backward_owner_split_scratch_bytes(int N, int H, int W, int C, int owner_plan, int segments);
WSSDL_API int wssdl_roi_pool_backward_compact_owner_split(const float *top_diff, const uint8_t *argmax8,
                            const float *rois, int R, int N, int H, int W, int C, int pooled_h,
                            int pooled_w, float spatial_scale, int rounding, float *bottom_diff,
                            void *workspace, size_t workspace_bytes, int owner_plan, int segments,
                            void *scratch, size_t scratch_bytes, wssdl_stream_t stream);
/* The bin-owner form reading the reference op's OWN arg-max layout (i32 flat index, roi_pooling_op_gpu.cu.cc:71-79): list
 * building + walk + halo merge in one call, owner plans 0 and 1.  Opt-in: RoiPoolGrad's declared contract
 * (wssdl_roi_pool_backward / _ws) stays the exact walk, bit for bit; this one is deterministic within the owner form's
 * bounds.  workspace = wssdl_roi_pool_backward_workspace_bytes, scratch = ..._owner_scratch_bytes. */
WSSDL_API int wssdl_roi_pool_backward_owner_i32(const float *top_diff, const int32_t *argmax, const float *rois, int R, int N,
                            int H, int W, int C, int pooled_h, int pooled_w, float spatial_scale, float *bottom_diff,
                            void *workspace, size_t workspace_bytes, int owner_plan, void *scratch, size_t scratch_bytes,
                            wssdl_stream_t stream);
WSSDL_API int wssdl_roi_argmax_expand(const uint8_t *argmax8, const float *rois, int R, int H, int W,
                            int C, int pooled_h, int pooled_w, float spatial_scale, int rounding,
                            int32_t *argmax, wssdl_stream_t stream);

/* ---------------------------------------------------------------- RoIAlign ---
 * Not in the reference: bilinear sampling of the RoI bins, no rounding of the RoI or of the bin edges
 * (cfg.ROI_POOL_MODE = 'align'; DESIGN.md "RoIAlign").  Layouts are the RoI-pool op's: bottom [N,H,W,C] f32, rois [R,5]
 * f32 (batch index, x1, y1, x2, y2), top [R,pooled_h,pooled_w,C] f32.  sampling (S) in 1..4 samples per bin and axis,
 * aligned in {0, 1} (the half-pixel offset), pooled_h / pooled_w in 1..16.
 *
 * All of a RoI's geometry lives in per-axis tables that wssdl_roi_align_tables writes and the other calls read.  One
 * buffer of wssdl_roi_align_tables_bytes, nine arrays back to back, no padding, 4-byte elements:
 *     ylo, yhi  i32 [R,pooled_h,S]     the two cells a sample reads along y
 *     yh,  yl   f32 [R,pooled_h,S]     their weights (yh for ylo, yl for yhi)
 *     xlo, xhi  i32 [R,pooled_w,S]     xh, xl  f32 [R,pooled_w,S]      the same along x
 *     win       i32 [R,5]              (image, first row, last row, first column, last column) of the cells the RoI
 *                                      reads; image = -1 for a dead row, first > last when every sample is void
 * Per axis, with RoI coordinates a1, a2, map length L and P bins, in f32 and exactly this order:
 *     off = aligned ? 0.5f : 0.0f;  s = a1*scale - off;  e = a2*scale - off;  len = e - s;
 *     if (!aligned) len = max(len, 1.0f);  bin = len / (float)P;
 *     y = (s + (float)p*bin) + (((float)i + 0.5f)*bin) / (float)S          for bin p, sample i
 *     y < -1 or y > L: void (indices 0, weights 0).  Else y = max(y, 0); lo = (int)y; lo >= L-1: lo = hi = L-1,
 *     y = (float)lo; else hi = lo+1.  l = y - (float)lo, h = 1.0f - l; the entry is (lo, hi, h, l).
 * A row is dead -- all void, a zero top row, no gradient -- when its batch index is < 0 (the padded blob's rows) or
 * >= N, or when any of its five numbers is not finite.  No kernel reads outside the map for any input.
 *
 * forward : top = sum over the S x S samples and their four cells of wy * wx * v, divided by S*S.
 * backward: bottom_diff, written in full.  wssdl_roi_align_backward_prepare builds, per (image, 4 x 4 tile of cells), the
 *           list of the RoIs whose window touches the tile, ascending; the backward is a gather: one wave owns a row of
 *           four cells and a slice of channels, walks its tile's list and stores each cell once, summed over RoI, bin row,
 *           bin column, all ascending.  No atomics: the same bits on every run.
 * R = 0 is valid: nothing is launched by the forward, the backward fills bottom_diff with zeros.  Every call below
 * clears the thread's last error on entry; an invalid argument sets it and returns WSSDL_ERR_INVALID_ARGUMENT, a buffer
 * that is too small WSSDL_ERR_INVALID_ARGUMENT as well, before anything is launched. */
WSSDL_API size_t wssdl_roi_align_tables_bytes(int R, int pooled_h, int pooled_w, int sampling);
WSSDL_API int wssdl_roi_align_tables(const float *rois, int R, int N, int H, int W, int pooled_h, int pooled_w,
                            float spatial_scale, int sampling, int aligned, void *tables, size_t tables_bytes,
                            wssdl_stream_t stream);
WSSDL_API int wssdl_roi_align_forward(const float *bottom, int N, int H, int W, int C, int R, int pooled_h, int pooled_w,
                            int sampling, const void *tables, size_t tables_bytes, float *top, wssdl_stream_t stream);
WSSDL_API size_t wssdl_roi_align_backward_workspace_bytes(int R, int N, int H, int W);
WSSDL_API int wssdl_roi_align_backward_prepare(int R, int N, int H, int W, int pooled_h, int pooled_w, int sampling,
                            const void *tables, size_t tables_bytes, void *workspace, size_t workspace_bytes,
                            wssdl_stream_t stream);
WSSDL_API int wssdl_roi_align_backward(const float *top_diff, int R, int N, int H, int W, int C, int pooled_h, int pooled_w,
                            int sampling, const void *tables, size_t tables_bytes, const void *workspace,
                            size_t workspace_bytes, float *bottom_diff, wssdl_stream_t stream);

/* --------------------------------------------------------------------- a13 ---
 * Multi-task loss of the supervised images and its gradients: fast_rcnn/train_bus.py:186-192 /
 * :605-610 (rpn_cross_entropy), :203-210 / :613-620 (rpn_loss_box, threshold |d| < 1 with the
 * sigma = 3 pieces as written), :218 / :623-630 (cross_entropy), :231-235 / :641-647 (loss_box).
 * Layouts are the layers' own (network.py:196-291): rpn_cls_score [n_images,H,W,2A] raw scores
 * (channel c*A + a: the reshape to [n, A*H, W, 2] is an index map), rpn_labels [n_images,1,A*H,W] i32
 * in {-1,0,1}, rpn_bbox_pred [n_images,H,W,4A], rpn targets / weights [n_images,4A,H,W]; the box term
 * covers the first n_box_images images (combined mode: IMS_PER_BATCH; the others get zero gradient).
 * cls_score [>= n_rows, num_classes], labels [n_rows] i32 (-1 = padding row: not counted),
 * bbox_pred [>= n_rows, 4*num_classes], bbox targets / weights [n_rows, 4*num_classes].
 * forward : losses[4] = rpn_cross_entropy, rpn_loss_box, cross_entropy, loss_box (f32; sums in f64,
 *           combined in a fixed order); the workspace keeps the two counts for the backward.
 * backward: grad_losses [4] f32 (device) = upstream gradient of each term; writes the gradients of
 *           the four prediction tensors in full (rows_total >= n_rows rows of the two head outputs:
 *           rows past n_rows and padding rows get zeros). */
WSSDL_API size_t wssdl_multi_task_loss_workspace_bytes(int n_images, int H, int W, int A);
WSSDL_API int wssdl_multi_task_loss_forward(
    const float *rpn_cls_score, const int32_t *rpn_labels, const float *rpn_bbox_pred,
    const float *rpn_bbox_targets, const float *rpn_inside_w, const float *rpn_outside_w, int n_images,
    int n_box_images, int H, int W, int A, const float *cls_score, const int32_t *labels,
    const float *bbox_pred, const float *bbox_targets, const float *bbox_inside_w,
    const float *bbox_outside_w, int n_rows, int num_classes, float *losses, void *workspace,
    size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API int wssdl_multi_task_loss_backward(
    const float *rpn_cls_score, const int32_t *rpn_labels, const float *rpn_bbox_pred,
    const float *rpn_bbox_targets, const float *rpn_inside_w, const float *rpn_outside_w, int n_images,
    int n_box_images, int H, int W, int A, const float *cls_score, const int32_t *labels,
    const float *bbox_pred, const float *bbox_targets, const float *bbox_inside_w,
    const float *bbox_outside_w, int n_rows, int rows_total, int num_classes, const float *grad_losses,
    const void *workspace, float *grad_rpn_cls_score, float *grad_rpn_bbox_pred, float *grad_cls_score,
    float *grad_bbox_pred, wssdl_stream_t stream);
/* The same four terms PER IMAGE, forward only: what a validation pass averages (fast_rcnn/train_bus.py:427-534 /
 * :792-899 evaluate the training losses on one validation image per step).  Inputs and layouts as
 * wssdl_multi_task_loss_forward; every image is a batch of its own, so there is no n_box_images.  The image of row r
 * of the RoI list is roi_image[r * roi_image_stride] (f32; column 0 of the rois blob [n_rows,5]: stride 5); rows need
 * not be grouped or ordered by image, and a row whose index is outside [0, n_images) or whose label is outside
 * [0, num_classes) contributes to nothing.
 *   losses [n_images,4]  row i = rpn_cross_entropy, rpn_loss_box, cross_entropy, loss_box of image i, each as the
 *                        forward above defines it for a batch holding that image alone (no labelled anchor / no
 *                        labelled row: NaN for the two cross-entropies) -- except that loss_box sums the labelled
 *                        rows only (the forward above adds the box sum of every row, padding rows included, which
 *                        carry zero weights there), divided by max(labelled rows, 1)
 *   counts [n_images,2]  labelled anchors (label != -1) and labelled rows of image i
 * One launch and one finish launch for all images, f64 sums combined in a fixed order (bit-identical from run to run),
 * no atomics, nothing read back.  A workspace smaller than the query's answer is WSSDL_ERR_INVALID_ARGUMENT. */
WSSDL_API size_t wssdl_multi_task_loss_per_image_workspace_bytes(int n_images, int H, int W, int A);
WSSDL_API int wssdl_multi_task_loss_per_image(
    const float *rpn_cls_score, const int32_t *rpn_labels, const float *rpn_bbox_pred,
    const float *rpn_bbox_targets, const float *rpn_inside_w, const float *rpn_outside_w, int n_images,
    int H, int W, int A, const float *cls_score, const int32_t *labels, const float *bbox_pred,
    const float *bbox_targets, const float *bbox_inside_w, const float *bbox_outside_w, int n_rows,
    int num_classes, const float *roi_image, int roi_image_stride, float *losses, float *counts,
    void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
/* y[i] = expf(x[i]) (which = 0) or log1pf(x[i]) (which = 1) for n f32 values on the device, computed by the
 * library functions exactly as the loss kernels get them (same translation unit, same compiler flags): what the
 * tests measure against f64 to fix the allowance of their error bounds. */
WSSDL_API int wssdl_loss_libm_probe(const float *x, int64_t n, int which, float *y, wssdl_stream_t stream);

/* ---------------------------------------------------------------------- f1 ---
 * MIL bag functions: mil/core.py:11-46 (get_bag_logit) with its five bag functions.  Four SELECT one row of the bag:
 * get_mal_max_logit :60-69 (largest class-2 logit), get_ben_max_logit :49-57 (largest class-1 logit),
 * get_mass_max_logit :88-96 (smallest class-0 logit), get_disc_max_logit :77-85 (largest logit over the classes
 * 1..num_classes-1).  Scanning keeps a row only on a strict improvement, and among equal keys the lowest row index
 * wins (tf.arg_max / tf.arg_min: first extremum).  get_mean_ben_logit :71-74 POOLS: the bag's logit row is
 * [0, m, 0, ...] (every class but 1 is 0, for num_classes > 3 too), m = mean of the bag's class-1 logits -- summed in
 * f64 (per-thread partials, then a fixed tree: the same bits on every run), divided by the count in f64, rounded to
 * f32 once.
 * instance_logits [R,num_classes] f32; the bag of row r is (int)(bag_of_row[r*bag_stride] -
 * bag_offset) (e.g. the batch-index column of the rois blob minus IMS_PER_BATCH,
 * fast_rcnn/train_bus.py:653); bag_labels [n_bags] i32.  Bags labelled 1 use selector_label1,
 * the others selector_other (train_bus.py:241,655).  row_out [n_bags] i32 receives the row to
 * gather (first extremum; the bag's first row for a mean-ben bag; -1 for an empty bag, whatever the selector, so
 * "row >= 0" means "not empty"), count_out (optional) the instances per bag. */
enum wssdl_mil_selector { WSSDL_MIL_MAL_MAX = 0, WSSDL_MIL_BEN_MAX = 1, WSSDL_MIL_MASS_MAX = 2,
                          WSSDL_MIL_DISC_MAX = 3, WSSDL_MIL_MEAN_BEN = 4 };
WSSDL_API int wssdl_mil_select(const float *instance_logits, int R, int num_classes,
                     const float *bag_of_row, int bag_stride, float bag_offset,
                     const int32_t *bag_labels, int n_bags, int selector_label1,
                     int selector_other, int32_t *row_out, int32_t *count_out,
                     wssdl_stream_t stream);

/* The MIL term as one op: selection as above, then fast_rcnn/train_bus.py:246-260 / :657-671 --
 * softmax CE of the bag's logit row against the bag label, weighted by class_weights_host[label]
 * ([0, WS_MAL_PCT, 1 - WS_MAL_PCT], :252,:664; host array [num_classes], 3 <= num_classes <= 8) and by `scale`
 * (1 - 0.99 * 0.9^floor(step/2000) or the constant, :248,:659), mean over the n_bags bags.  An empty
 * bag contributes 0, gets no gradient and still counts in the mean, whatever its selector.  loss [1] f32; row_out
 * [n_bags] i32 and bag_loss [n_bags] f32 are outputs the backward (row_out) and the caller may read.  The backward
 * writes the gradient of the whole [R,num_classes] logits block; grad_loss [1] f32 on the device.  With c =
 * grad_loss * scale * class_weights[label] / n_bags:
 *   a selecting bag   its selected row gets c * (softmax - onehot(label)), the label's component formed as minus the
 *                     sum of the others; every other row of the bag zeros;
 *   a mean-ben bag    every row r of the bag gets g[r,1] = c * d / count and zeros in the other columns, d the class-1
 *                     component of (softmax - onehot(label)) of the pooled row: p_1 when label != 1, minus the sum of
 *                     the other probabilities when label == 1;
 *   rows of no bag    zeros.
 * Forward: three launches (select, bag term, finish), backward: one, whatever the selector pair.
 *
 * wssdl_mil_loss_forward / _backward carry no per-bag count and no pooled row: they take the selecting functions
 * only, selectors 0..3 (WSSDL_MIL_DISC_MAX included), with the results they always had for 0..2, and return
 * WSSDL_ERR_INVALID_ARGUMENT for WSSDL_MIL_MEAN_BEN.  wssdl_mil_loss_backward takes no selectors: it puts the
 * gradient on the rows named by `rows`, whichever selecting pair found them.
 * wssdl_mil_pool_forward / _backward take all of 0..4 through the same kernels (for 0..2 bit for bit the results of
 * the pair above) and add bag_count [n_bags] i32 (instances per bag) and bag_logits [n_bags,num_classes] f32 (the
 * logit row each bag's term is taken of: the selected row's, [0, m, 0, ...] for a mean-ben bag, zeros for an empty
 * bag), which the backward reads. */
WSSDL_API int wssdl_mil_loss_forward(const float *instance_logits, int R, int num_classes,
                           const float *bag_of_row, int bag_stride, float bag_offset,
                           const int32_t *bag_labels, int n_bags, int selector_label1,
                           int selector_other, const float *class_weights_host, float scale,
                           float *loss, int32_t *row_out, float *bag_loss, wssdl_stream_t stream);
WSSDL_API int wssdl_mil_loss_backward(const float *instance_logits, int R, int num_classes,
                            const float *bag_of_row, int bag_stride, float bag_offset,
                            const int32_t *bag_labels, int n_bags, const int32_t *rows,
                            const float *class_weights_host, float scale, const float *grad_loss,
                            float *grad_logits, wssdl_stream_t stream);
WSSDL_API int wssdl_mil_pool_forward(const float *instance_logits, int R, int num_classes,
                           const float *bag_of_row, int bag_stride, float bag_offset,
                           const int32_t *bag_labels, int n_bags, int selector_label1,
                           int selector_other, const float *class_weights_host, float scale,
                           float *loss, int32_t *row_out, int32_t *bag_count, float *bag_logits,
                           float *bag_loss, wssdl_stream_t stream);
WSSDL_API int wssdl_mil_pool_backward(const float *instance_logits, int R, int num_classes,
                            const float *bag_of_row, int bag_stride, float bag_offset,
                            const int32_t *bag_labels, int n_bags, int selector_label1,
                            int selector_other, const int32_t *rows, const int32_t *bag_count,
                            const float *bag_logits, const float *class_weights_host, float scale,
                            const float *grad_loss, float *grad_logits, wssdl_stream_t stream);

/* ---------------------------------------------------------------------- f4 ---
 * The pinnable half of the host image path, on the device.  utils/blob.py:34-79
 * (prep_im_for_blob), :19-32 (im_list_to_blob), roi_data_layer/minibatch_bus.py:269-272 (grey plane
 * stacked three times, horizontal flip), datasets/imdb.py:106-121 (boxes of flipped images).
 * skimage.transform.resize (blob.py:74-77) sits in the middle: the steps around it are pinned by
 * fixtures from the reference's own blob.py, the resize follows the published algorithm of the
 * release the reference's README pins (scikit-image 0.14.2; the library is absent: parity unpinned):
 *   wssdl_image_prep     gray [h, row_stride] u8 -> out [h,w,3] f32 = what the reference hands to
 *                        the resize: flip, /255, optional brightness (+delta, clip to [0,1]),
 *                        optional contrast ((x - mean(x)) * factor + mean(x), clip), - pixel_mean/255.
 *                        delta / factor are the values the caller drew (the reference:
 *                        np.random.uniform, blob.py:50,55).  workspace: wssdl_image_prep_workspace_bytes.
 *   wssdl_image_to_blob  im [h,w,3] f64 (im_is_f64) or f32 = the resize's output -> blob
 *                        [n_images,Hmax,Wmax,3] f32, image `index`: x / scale (divide != 0: ResNet,
 *                        scale = pixel_std/255) or x * scale (VGG: 255), zero outside [h,w].
 *   wssdl_flip_boxes     in place on boxes [n, stride >= 4] f32: x1' = width - x2 - 1, x2' = width - x1 - 1.
 *   wssdl_image_resize   skimage.transform.resize(im, [rows, cols]) as blob.py:74-77 / fast_rcnn/test_bus.py:54-56 call
 *                        it (0.14 defaults: order 1, mode 'constant', cval 0, clip, no anti-aliasing):
 *                        im [h,w,channels] f32 or f64 (im_is_f64) -> out [rows,cols,channels] f64.
 *                        out(row, col) interpolates the input bilinearly at
 *                        (h/rows * (row + 0.5) - 0.5, w/cols * (col + 0.5) - 0.5); samples outside the
 *                        image read 0; the result is clipped to the input's [min, max].
 *   wssdl_image_warp     the general form = skimage.transform.warp(im, matrix, output_shape=(rows, cols),
 *                        order=1, mode, cval, clip): `matrix` = 9 doubles in HOST memory, row-major 3x3
 *                        inverse map (output (col,row,1) -> input (col,row,w)); serves rotate()
 *                        (blob.py:39-41) and a caller that brings skimage's own estimated matrix.
 *                        workspace: wssdl_image_warp_workspace_bytes (only read when clip != 0).
 *   wssdl_image_adjust_f64  blob.py:49-60 on the float64 image rotate() returns (weak images with
 *                        cfg.TRAIN.USE_ROTATION, :39-41): im = strided view [h,w,channels] f64 (row_stride in
 *                        elements; the crop :43-47 is a slice), the same brightness / contrast / mean steps as
 *                        wssdl_image_prep in f64 -> out [h,w,channels] f64 contiguous (the resize's input).
 *                        workspace: wssdl_image_prep_workspace_bytes. */
#define WSSDL_WARP_CONSTANT 0    /* mode='constant': cval outside the image */
#define WSSDL_WARP_EDGE 1        /* mode='edge': nearest edge pixel */
WSSDL_API size_t wssdl_image_warp_workspace_bytes(void);
WSSDL_API int wssdl_image_warp(const void *im, int im_is_f64, int h, int w, int channels, const double *matrix,
                     int rows, int cols, int mode, double cval, int clip, double *out, void *workspace,
                     size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API int wssdl_image_resize(const void *im, int im_is_f64, int h, int w, int channels, int rows, int cols,
                     double *out, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API int wssdl_image_adjust_f64(const double *im, int h, int w, int channels, int64_t row_stride,
                     int use_brightness, double brightness_delta, int use_contrast, double contrast_factor,
                     double pixel_mean, double *out, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API size_t wssdl_image_prep_workspace_bytes(void);
WSSDL_API int wssdl_image_prep(const uint8_t *gray, int h, int w, int row_stride, int flipped,
                     int use_brightness, float brightness_delta, int use_contrast,
                     float contrast_factor, double pixel_mean, float *out, void *workspace,
                     size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API int wssdl_image_to_blob(const void *im, int im_is_f64, int h, int w, double scale, int divide,
                     float *blob, int index, int n_images, int Hmax, int Wmax, wssdl_stream_t stream);
WSSDL_API int wssdl_flip_boxes(float *boxes, int n, int stride, float width, wssdl_stream_t stream);

/* The same image path for a whole mini-batch in one op (roi_data_layer/minibatch_bus.py:259-318: every image of the
 * batch through prep_im_for_blob, then im_list_to_blob), csrc/image_batch.hip.  AT MOST 3 LAUNCHES per batch whatever
 * n_images is (2 when no item is rotated): a statistics pass over the u8 planes, a second one that rotates the weak
 * images' planes, and the pass that writes the blob.  No host synchronise, no read-back, no allocation; no 3-channel
 * intermediate (the only temporary is the rotated, cropped plane of a rotated item: ONE f64 channel in the workspace).
 *   arena       all decoded grey planes, u8, one device buffer of arena_bytes bytes
 *   items_host  the table below, n_images items, in HOST memory: validated before anything is launched
 *   items_dev   the caller's device copy of the same table (what the kernels read)
 *   blob        [n_images, Hmax, Wmax, 3] f32: every element is written, the zero padding included
 * Item i: the plane is arena[offset + y * row_stride + x], y < h, x < w.  `flipped` mirrors it (minibatch_bus.py:271).
 * use_rotation: skimage.transform.rotate of the flipped plane / 255 with inv_map (row-major 3x3 inverse map, as
 * wssdl_image_warp takes it) and cval; f64 from there on (blob.py:39-41).  use_crop: the slice [crop_u : h - crop_d,
 * crop_l : w - crop_r] of the (flipped, rotated) image (:43-47).  use_brightness / use_contrast with the caller's draws
 * (:49-58; f32 arithmetic for an unrotated item, f64 for a rotated one), - pixel_mean / 255 (:60), resize to
 * [rows, cols] (:74, wssdl_image_resize), then x / scale (divide != 0) or x * scale (:75-77).
 * rot_offset (rotated items only): where the item's rotated plane starts in the workspace, in f64 elements = the sum
 * of (h - crop_u - crop_d) * (w - crop_l - crop_r) over the rotated items before it.
 * Every image of the blob is bit for bit what wssdl_image_prep / _warp / _adjust_f64 / _resize / _to_blob give for it:
 * the same operations in the same order, the two reductions in their partial-sum order (grid of 256 x n_images blocks);
 * the resize's clip range is taken from the extremes of the plane (every step up to the resize's input is monotone).
 * Every gather is bounded: a tap outside the view reads cval.
 * WSSDL_ERR_INVALID_ARGUMENT, nothing launched: n_images < 1 or > 65535, a null pointer, h / w / rows / cols < 1,
 * row_stride < w, a view that leaves the arena, crop offsets that leave no pixel, rows > Hmax or cols > Wmax, scale == 0,
 * a non-finite inv_map / cval / delta / factor, a wrong rot_offset.  WSSDL_ERR_WORKSPACE: workspace_bytes below
 * wssdl_image_batch_workspace_bytes(n_images, rotated_pixels), rotated_pixels = the sum named above over all items. */
typedef struct wssdl_image_batch_item {
    int64_t offset;                  /* bytes into the arena */
    int64_t rot_offset;              /* f64 elements into the workspace's plane area (rotated items) */
    double inv_map[9];
    double cval;
    double brightness_delta, contrast_factor;
    double pixel_mean;               /* 0 .. 255 scale (cfg.PIXEL_MEANS) */
    double scale;
    int32_t h, w, row_stride, flipped;
    int32_t crop_u, crop_d, crop_l, crop_r;
    int32_t use_crop, use_rotation, use_brightness, use_contrast;
    int32_t rows, cols, divide, reserved;
} wssdl_image_batch_item;
WSSDL_API size_t wssdl_image_batch_workspace_bytes(int n_images, int64_t rotated_pixels);
WSSDL_API int wssdl_image_batch_blob(const uint8_t *arena, size_t arena_bytes, const wssdl_image_batch_item *items_host,
                     const wssdl_image_batch_item *items_dev, int n_images, int Hmax, int Wmax, float *blob,
                     void *workspace, size_t workspace_bytes, wssdl_stream_t stream);

/* ---------------------------------------------------------------------- f3 ---
 * The post-detection step of the test path, fast_rcnn/test_bus.py:360-401, batched over the classes:
 * for every class j = 1 .. num_classes-1 the rows with scores[r, j] > score_thresh, greedy NMS at
 * nms_thresh with the cpu_nms rule (utils/cython_nms) on (boxes[r, 4j:4j+4], scores[r, j]) in descending
 * score order, then the cap: if more than max_per_image (> 0) detections are left over all classes, only
 * those with a score >= the max_per_image-th largest stay (ties stay, like the reference's `>=`).
 *   scores [R, num_classes] f32, boxes [R, 4 * num_classes] f32 (class-wise decoded boxes);
 *   dets   [num_classes-1, R, 5] f32: row p of class j-1 = (x1, y1, x2, y2, score) of its p-th kept
 *          detection in descending score order; counts [num_classes-1] i32 = rows that survive the cap.
 *          Rows of dets at and beyond a class's count are not written: they keep what the caller's buffer held.
 * One set of launches for all classes, no host read-back.  num_classes <= 65. */
WSSDL_API size_t wssdl_post_detections_workspace_bytes(int R, int num_classes);
WSSDL_API int wssdl_post_detections(const float *scores, const float *boxes, int R, int num_classes,
                     float score_thresh, double nms_thresh, int max_per_image, float *dets,
                     int32_t *counts, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);

/* The same step for a batch of images in one set of launches, no host read-back (test_net over a batch).
 *   rois   [R, 5] f32: the blob fed to RoI pooling; only its batch column is read.  The rows of one image are
 *          contiguous and the images come in ascending order (the compact blob and the cfg.PADDED_ROIS blob of
 *          the proposal layer both are); rows with a batch index < 0 (or >= n_images) are ignored.
 *   scores [R, num_classes] f32, boxes [R, 4 * num_classes] f32: the blob's class scores and decoded boxes;
 *   dets   [n_images, num_classes-1, max_rows_per_image, 5] f32, counts [n_images, num_classes-1] i32:
 *          dets[i, j-1, :counts[i, j-1]] = image i's class-j detections, best first, after image i's own cap
 *          (the rows at and beyond the count are not written, as in the single-image op).
 * Every image's output is bit for bit that of wssdl_post_detections on its rows alone.  An image with more
 * rows than max_rows_per_image is reported as counts[i, 0] = -1 (the other counts of the image 0).
 * num_classes <= 65, n_images * (num_classes-1) * max_rows_per_image <= 2^24 and
 * n_images * (num_classes-1) <= 65535; R == 0 or n_images == 0: zero counts, nothing else launched.
 * wssdl_post_detections is the case n_images = 1, rois = NULL (rows 0 .. R-1), max_rows_per_image = R. */
WSSDL_API size_t wssdl_post_detections_batched_workspace_bytes(int n_images, int max_rows_per_image, int num_classes);
WSSDL_API int wssdl_post_detections_batched(const float *rois, const float *scores, const float *boxes, int R,
                     int n_images, int max_rows_per_image, int num_classes, float score_thresh, double nms_thresh,
                     int max_per_image, float *dets, int32_t *counts, void *workspace, size_t workspace_bytes,
                     wssdl_stream_t stream);

/* The class-agnostic variant of both (cfg.TEST.CLS_AGNOSTIC_NMS, fast_rcnn/test_bus.py:371-384): after the
 * per-class step above (score filter, NMS at nms_thresh, kept rows in descending score order) the classes' kept
 * rows are concatenated in class order j = 1 .. num_classes-1 and the same greedy NMS runs once more over that
 * union, at the same nms_thresh, visiting it in descending score order (equal scores: the later row of the
 * concatenation first, the tie-break of every ranking here).  Class j's detections are the union's survivors that
 * came from class j, still in descending score order; the cap then applies to them exactly as above.
 * Arguments, output layout (dets, counts, the -1 flag of an image with more rows than max_rows_per_image) and the
 * limits are those of the per-class pair, so whatever consumes its output (WSSDL_EVAL_BATCHED below) takes this one
 * unchanged.  One limit more: the union of one image is ONE NMS segment of
 *   U = (num_classes-1) * max_rows_per_image <= WSSDL_POST_AGNOSTIC_MAX_UNION
 * items, ranked and swept by the kernels the proposal layer runs at 12000 candidates per image; its suppression
 * matrix takes U * ceil(U / 1024) * 128 bytes per image of the workspace (18.4 MB at the limit).  Beyond the limit:
 * WSSDL_ERR_INVALID_ARGUMENT.  One set of launches for all images and classes, no host read-back.
 * Every image's output is bit for bit that of the single-image call on its rows alone.  With num_classes == 2 the
 * second pass finds nothing left to suppress, and the output is bit for bit the per-class one as long as no two kept
 * rows of an image have the same score: among equal scores the union ranks the LATER kept row first (the tie-break
 * above, applied to the concatenation as the reference's nms call sees it), which is the reverse of their per-class
 * order.
 * The single-image call is the case n_images = 1, rois = NULL, max_rows_per_image = R. */
#define WSSDL_POST_AGNOSTIC_MAX_UNION 12000
WSSDL_API size_t wssdl_post_detections_agnostic_workspace_bytes(int R, int num_classes);
WSSDL_API int wssdl_post_detections_agnostic(const float *scores, const float *boxes, int R, int num_classes,
                     float score_thresh, double nms_thresh, int max_per_image, float *dets,
                     int32_t *counts, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);
WSSDL_API size_t wssdl_post_detections_agnostic_batched_workspace_bytes(int n_images, int max_rows_per_image,
                     int num_classes);
WSSDL_API int wssdl_post_detections_agnostic_batched(const float *rois, const float *scores, const float *boxes, int R,
                     int n_images, int max_rows_per_image, int num_classes, float score_thresh, double nms_thresh,
                     int max_per_image, float *dets, int32_t *counts, void *workspace, size_t workspace_bytes,
                     wssdl_stream_t stream);

/* Test-time augmentation: the same step over the V views of every image (mirrored copies, cfg.TEST.FLIP_AUG) with
 * optional box voting (cfg.TEST.BBOX_VOTE), one set of launches, no host read-back, capturable.
 *   rois [R, 5], scores [R, num_classes], boxes [R, 4 * num_classes] f32: as in the batched op, the blob of a forward
 *          over n_images * views SOURCE images.  Source image s is view s % views of output image s / views: the views
 *          of an image are interleaved, so the rows of one output image are contiguous and the output images come in
 *          ascending order.  Rows whose batch index is outside [0, n_images * views) are dead and ignored.
 *   flip_width [n_images * views] f32 or NULL: an entry w >= 0 marks a mirrored source image of original width w; an
 *          entry < 0 (or a NULL array) a source that is not mirrored.
 * Per output image t:
 *   1. Un-mirror.  For a row of a mirrored source every class's box becomes
 *        x1' = max((w - x2) - 1, 0),   x2' = (w - x1) - 1,
 *      every operation rounded to f32 on its own (the arithmetic of wssdl_flip_boxes, then the clamp: the clip bound
 *      of the decode can exceed w - 1 by a fraction of a pixel); y is unchanged.  The inputs are not modified: the
 *      un-mirrored boxes live in the workspace.
 *   2. Candidates of class j >= 1: the rows of t with scores[r, j] > score_thresh in ascending row order, all views
 *      together.
 *   3. Greedy NMS at nms_thresh over them exactly as in the batched op (the cpu_nms rule, descending score, among equal
 *      scores the later row first); with agnostic != 0 the union pass of wssdl_post_detections_agnostic_batched follows,
 *      with its limit (num_classes-1) * max_rows_per_image <= WSSDL_POST_AGNOSTIC_MAX_UNION.
 *   4. The cap max_per_image as in the batched op.
 *   5. Voting, when vote_thresh > 0.  For each class-j detection d left by 3-4, over the class-j candidates c of step 2
 *      (pre-NMS, un-mirrored, ascending row order): c votes when its overlap with d,
 *        the f64 statement of the overlap op above -- utils/bbox.pyx, +1 pixel convention -- with c as the box and d as
 *        the query, is >= vote_thresh
 *      (d itself always votes: its overlap is exactly 1).  In f64, serially over the voters in ascending row order,
 *        sw += (double)s_c;   sx[k] += (double)s_c * (double)c[k]      (k = x1, y1, x2, y2; the product is exact)
 *      and d[k] = (float)(sx[k] / sw): one IEEE f64 division, one rounding to f32.  The score and the order of the
 *      detections are unchanged; votes never cross classes, also under agnostic.
 *   dets [n_images, num_classes-1, max_rows_per_image, 5] f32, counts [n_images, num_classes-1] i32: the batched op's
 *          layout and conventions.  Rows of dets at and beyond a class's count are not written: they keep what the caller's buffer held.
 *          An output image whose views together span more than max_rows_per_image rows (dead rows between its views
 *          included) gets counts[t, 0] = -1 and zeros in its other counts.
 * WSSDL_ERR_INVALID_ARGUMENT without a launch: views < 1 or views > 8; the batched op's limits (on n_images output
 * images); vote_thresh > 1; vote_thresh > 0 with score_thresh < 0 (the weights must be positive); a NULL rois, scores,
 * boxes, dets or workspace with R > 0.  R == 0: zero counts, nothing else launched.
 * With views == 1, no mirrored source and vote_thresh <= 0 the output is bit for bit the batched op's. */
WSSDL_API size_t wssdl_post_detections_views_workspace_bytes(int n_images, int views, int max_rows_per_image,
                     int num_classes);
WSSDL_API int wssdl_post_detections_views(const float *rois, const float *scores, const float *boxes, int R,
                     int n_images, int views, const float *flip_width, int max_rows_per_image, int num_classes,
                     float score_thresh, double nms_thresh, int agnostic, double vote_thresh, int max_per_image,
                     float *dets, int32_t *counts, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);

/* Soft-NMS at test time (Bodla et al., 2017; cfg.TEST.SOFT_NMS; not in the reference): the views op above with a score
 * decay in place of the deletion, one set of launches, no host read-back, no allocation.
 * Inputs (rois, scores, boxes, R, n_images, views, flip_width), the views layout, dead rows, the un-mirror step
 * (x1' = max((w - x2) - 1, 0), x2' = (w - x1) - 1 in f32, inputs not modified) and the output layout are exactly
 * those of wssdl_post_detections_views: dets [n_images, num_classes-1, P, 5], counts [n_images, num_classes-1],
 * P = max_rows_per_image; counts[t, 0] = -1 (zeros in t's other counts) for an image whose views span more than P rows;
 * rows of dets at and beyond a count are not written.
 * Per output image t and class j >= 1:
 *   1. Candidates: the rows of t with scores[r, j] > score_thresh and scores[r, j] > min_score, in ascending row
 *      order, all views together, with un-mirrored boxes.  Each carries its local row index (row minus the first row of
 *      t, as in the batched op), a working score s (f32) and area = (x2 - x1 + 1) * (y2 - y1 + 1), every operation
 *      rounded to f32 (the cpu_nms rule).  All candidates are live.
 *   2. While a live candidate exists:
 *      Pick    the live i with the largest s; among equal s the largest local row index (the tie-break of every
 *              ranking here; it applies to scores that become equal through decay too).
 *      Emit    (box_i, s_i) is the class's next detection; i is no longer live.
 *      Overlap for every live j, the cpu_nms overlap in f32, every operation rounded on its own, no contraction:
 *                w = max(0, min(x2_i, x2_j) - max(x1_i, x1_j) + 1), h likewise, inter = w * h,
 *                ov = inter / ((area_i + area_j) - inter).
 *      Weight  method 0 (hard):     wt = 0 if (double)ov >= nms_thresh, else 1;
 *              method 1 (linear):   wt = 1.0f - ov if (double)ov >= nms_thresh, else 1;
 *              method 2 (Gaussian): wt = (float)exp(-((double)ov * (double)ov) / sigma) -- the product is exact in f64,
 *                                   then one f64 division, one f64 exp, one rounding to f32; ov == 0 gives exactly 1
 *                                   (the exp may be skipped); nms_thresh is not read.
 *      Decay   s_j = s_j * wt in f32; if not s_j > min_score, j stops being live for good.
 *      The comparison is >=, as in the hard NMS of this library (Bodla et al. write >), so method 0 is the existing op.
 *   3. Emitted scores never increase (every pick is the maximum of what is left, and decay only lowers), so a class's
 *      detections are in descending score order and the cap keeps a prefix.
 *   4. The cap max_per_image applies exactly as in the batched op, over the emitted (decayed) scores; ties stay.
 * No class-agnostic pass and no voting in this op.
 * WSSDL_POST_SOFT_MAX_ROWS: a segment's candidates live in the LDS of the one workgroup that runs its pick loop, at
 * 24 bytes each (box 16, working score 4, area 4).  gfx950 gives a workgroup 160 KiB = 163840 bytes:
 * 163840 / 24 = 6826 rows; 4096 rows take 98304 bytes (96 KiB) and leave room for the kernel's static part.
 * WSSDL_ERR_INVALID_ARGUMENT without a launch: views outside 1..8; method outside 0..2; sigma <= 0 or non-finite under
 * method 2; nms_thresh outside (0, 1] under methods 0 and 1; min_score outside [FLT_MIN, 1) -- with a floor at or above
 * FLT_MIN a product that underflows is dropped whether or not the hardware flushes it, so the denormal mode cannot
 * change a bit --; score_thresh < 0; num_classes outside 2..65; max_rows_per_image > WSSDL_POST_SOFT_MAX_ROWS (the
 * workspace query returns 0 there); the batched op's grid limits; a NULL rois, scores, boxes, dets or workspace with
 * R > 0.  R == 0 or n_images == 0: zero counts, nothing else launched.
 * With method 0 the output is bit for bit that of wssdl_post_detections_views with agnostic = 0, vote_thresh = 0 on
 * the same arguments, for candidates above min_score (pass min_score <= score_thresh). */
#define WSSDL_POST_SOFT_MAX_ROWS 4096
WSSDL_API size_t wssdl_post_detections_soft_workspace_bytes(int n_images, int views, int max_rows_per_image,
                     int num_classes);
WSSDL_API int wssdl_post_detections_soft(const float *rois, const float *scores, const float *boxes, int R,
                     int n_images, int views, const float *flip_width, int max_rows_per_image, int num_classes,
                     float score_thresh, int method, double nms_thresh, double sigma, float min_score,
                     int max_per_image, float *dets, int32_t *counts, void *workspace, size_t workspace_bytes,
                     wssdl_stream_t stream);

/* Decode and clip of the head's class-wise boxes: the step between a forward's layers and the post-detection ops
 * above, as the reference's validation loop does it on the sampled RoIs (fast_rcnn/train_bus.py:456-457 / :821-822:
 * boxes = rois[:, 1:5] / scale; clip_boxes(bbox_transform_inv(boxes, bbox_pred), im.shape)), for all images of a batch
 * in ONE launch.
 *   rois   [R, 5] f32 (batch index, x1, y1, x2, y2) in the scaled image's pixels; deltas [R, 4 * num_classes] f32;
 *   im_info [n_images, info_stride >= 3] f32 rows (h, w, scale, ...);
 *   bounds [n_images, 2] f32 (xmax, ymax) per image, or NULL;
 *   boxes  [R, 4 * num_classes] f32, the layout the post-detection ops read.  Class 0's four columns are written like
 *          the others, as the reference does.
 * Per (row r, class k), in this order, every operation rounded to f32 on its own (no contraction):
 *   1. i = (int)rois[r, 0].  A row whose index is outside [0, n_images) (NaN included) is a dead row: its
 *      4 * num_classes outputs are zeros and nothing else is read for it, so the blob is fully initialised.
 *   2. s = im_info[i, 2]; b = rois[r, 1..4] / s by IEEE f32 division (not a multiplication by a reciprocal).
 *   3. bbox_transform_inv (fast_rcnn/bbox_transform.py:30-61) with d = deltas[r, 4k .. 4k+3]:
 *        w = (b.x2 - b.x1) + 1;  cx = b.x1 + 0.5f * w;  pcx = d.x * w, then pcx + cx;
 *        pw = (float)exp((double)d.z) * w;  x1 = pcx - 0.5f * pw;  x2 = pcx + 0.5f * pw;  the same for y with d.y, d.w.
 *   4. clip_boxes (:63-77): max(min(v, xmax), 0) on x1 and x2, with ymax on y1 and y2, where
 *        (xmax, ymax) = bounds[i] when bounds is given (the reference clips to the original image: (W - 1, H - 1)),
 *        else xmax = (float)((double)w_i / (double)s - 1.0), ymax likewise from h_i, (h_i, w_i) = im_info[i, 0..1]
 *        (the rule of the batched test-time path).
 * No workspace, no allocation, no read-back: capturable like the other entry points.  R == 0 returns WSSDL_OK and
 * launches nothing.  WSSDL_ERR_INVALID_ARGUMENT, without a launch: R < 0, num_classes < 2 or > 65, n_images < 1,
 * info_stride < 3, and with R > 0 a NULL rois, deltas, im_info or boxes, or deltas / boxes not 16-byte aligned (a pair's
 * four values move as one vector).  Behaviour on non-finite coordinates, deltas and scales is unspecified. */
WSSDL_API int wssdl_decode_detections(const float *rois, const float *deltas, int R, int num_classes,
                     const float *im_info, int info_stride, int n_images, const float *bounds, float *boxes,
                     wssdl_stream_t stream);

/* ---------------------------------------------------------------- evaluation ---
 * Detection evaluation, datasets/voc_eval_bus.py + the 44 calls of datasets/bus.py:_do_python_eval in one pass:
 * for every class j = 1 .. n_classes-1 the PASCAL VOC precision / recall curve and AP (11-point and area), and for
 * every one of T score thresholds the CorLoc count nok and the FROC count num_all_fps.  One overlap pass (f64, the
 * operation order of voc_eval_bus.py:221-236, first maximum like np.argmax), one sort, one first-hit-per-box pass
 * and one prefix sum.  No allocation, no read-back, no host synchronisation: capturable like the other entry points.
 *
 * flags
 *   WSSDL_EVAL_QUANTISE  evaluate what the reference wrote to its result file (bus.py:257-261): the score as
 *          '{:.3f}' -- conf = rint(double(s) * 1000.0) / 1000.0 -- and every coordinate as '{:.1f}' of the f32 value
 *          x + 1 -- rint(double(x +f32 1.0f) * 10.0) / 10.0; both reproduce the parsed doubles exactly (the products
 *          are exact in f64, rint rounds half to even like the correctly rounded formatting, the division is the
 *          decimal parse).  The ground truth then holds the annotation's 1-based pixel values as they stand.
 *          Without the flag the f32 values are used as they are, no + 1 on either side.
 *   WSSDL_EVAL_BATCHED   the detections are the (dets, counts) pair wssdl_post_detections_batched wrote:
 *          dets [N, n_classes-1, P, 5] f32, counts [N, n_classes-1] i32 (a count < 0 reads as 0); batch image i is
 *          image first_image + i.  Input index of a slot = ((i * (n_classes-1) + j-1) * P + p); D is ignored and the
 *          outputs sized by D below are sized by N * (n_classes-1) * P.
 *          Without the flag: det_boxes [D,4] f32, det_scores [D] f32, det_image [D] i32, det_class [D] i32 in
 *          1 .. n_classes-1.  A detection whose image is outside 0 .. n_images-1 or whose class is outside
 *          1 .. n_classes-1 is ignored.  The pointers of the layout that is not used may be NULL.
 * Ground truth: gt_boxes [G,4] f64, gt_class [G] i32, gt_difficult [G] u8, gt_image_offsets [n_images+1] i32 (the
 * boxes of image i are rows gt_image_offsets[i] .. gt_image_offsets[i+1]-1).
 *
 * Order: per class, descending confidence; detections of equal confidence keep their INPUT order (image index,
 * then rank within the image) -- the stable sort of the result file's lines.  The reference's
 * np.argsort(-confidence) is an unstable introsort: its order among equal scores, and every curve value that depends
 * on it, is an accident of NumPy; with pairwise distinct (quantised) scores the two agree bit for bit.
 *
 * Outputs (device):
 *   order [D] i32          input indices, class 1's detections first (best first), then class 2's, ...; -1 past the end
 *   class_offsets [n_classes] i32   class j's segment of order / tp / fp / rec / prec is [class_offsets[j-1], class_offsets[j])
 *   tp, fp [D] i32         cumulative counts along the class's segment (integer-exact)
 *   rec, prec [D] f64      tp / double(npos), tp / max(tp + fp, DBL_EPSILON)
 *   ap07, ap_area [n_classes-1] f64   voc_ap with use_07_metric True (bit-equal: p / 11. accumulated in the
 *                          reference's order by one thread) and False; -1 for a class without detections (the
 *                          reference's sentinel for an empty result file; its tp / fp / nok / num_all_fps are 0)
 *   npos, ni [n_classes-1] i32   non-difficult boxes of the class; images with a box of the class (0 is reported as
 *                          0: the caller decides what CorLoc means then, the reference divides by zero)
 *   nok, num_all_fps [n_classes-1, T] i32   for thresholds [T] f64 (device), `conf >= t`
 *   arr_ok [n_classes-1, n_images] u8, num_fp_per_img [n_classes-1, n_images] i32   at thresholds[base_threshold]
 * D == 0 and G == 0 are valid.  WSSDL_ERR_INVALID_ARGUMENT: negative sizes, T < 1, n_classes < 2 or > 65, more than
 * 2^24 detections (slots), base_threshold outside 0 .. T-1, a missing pointer, a workspace smaller than
 * wssdl_eval_detections_workspace_bytes(D or N * (n_classes-1) * P, G, n_images, n_classes) (pure host; 0 for
 * sizes the op rejects). */
#define WSSDL_EVAL_QUANTISE 1
#define WSSDL_EVAL_BATCHED 2
WSSDL_API size_t wssdl_eval_detections_workspace_bytes(int64_t D, int G, int n_images, int n_classes);
WSSDL_API int wssdl_eval_detections(int flags, const float *det_boxes, const float *det_scores, const int32_t *det_image,
                     const int32_t *det_class, int D, const float *dets, const int32_t *counts, int N, int P,
                     int first_image, const double *gt_boxes, const int32_t *gt_class, const uint8_t *gt_difficult,
                     const int32_t *gt_image_offsets, int G, int n_images, int n_classes, double ovthresh,
                     const double *thresholds, int T, int base_threshold, int32_t *order, int32_t *class_offsets,
                     int32_t *tp, int32_t *fp, double *rec, double *prec, double *ap07, double *ap_area, int32_t *npos,
                     int32_t *ni, int32_t *nok, int32_t *num_all_fps, uint8_t *arr_ok, int32_t *num_fp_per_img,
                     void *workspace, size_t workspace_bytes, wssdl_stream_t stream);

/* ------------------------------------------------------------ proposal recall ---
 * RPN proposal recall, datasets/imdb.py:125-213 (evaluate_recall) for every (area range a, limit l) cell of the
 * recall table in one call: the f64 IoU matrix of every image is computed once (the operation order of
 * utils/bbox.pyx, bit-identical), the cells mask its columns (area) and cut its rows (limit) and run the reference's
 * greedy matching on it.  No allocation, no read-back, no host synchronisation.
 *
 * Candidate boxes, exactly one of
 *   boxes_f32   padded f32: the first coordinate of row 0 of image 0; row p of image i starts at
 *               boxes_f32 + (i * P + p) * row_stride and holds x1, y1, x2, y2 (for the proposal layer's
 *               rois [N, P, 5]: rois + 1, row_stride 5).  With scale [N] f32 (may be NULL) every coordinate is
 *               divided by scale[i] in f32 (IEEE, round to nearest) and then widened to f64: im_proposals' boxes.
 *   boxes_f64   padded f64 [N, P, row_stride >= 4], used as they are (the reference's boxes.astype(np.float)).
 * counts [N] i32: image i has rows 0 .. counts[i]-1 (read as clamped to 0 .. P).
 * Ground truth, already filtered to gt_classes > 0 and max gt_overlaps == 1: gt_boxes [Gtot, 4] f64, gt_areas [Gtot]
 * f64 (the roidb's seg_areas), gt_image_offsets [N + 1] i32 in HOST memory (validated before anything is launched,
 * then copied to the workspace on the stream: keep it valid until the stream has passed the call); image i owns rows
 * gt_image_offsets[i] .. gt_image_offsets[i+1]-1, at most WSSDL_RECALL_MAX_GT of them.
 * area_ranges [A, 2] f64, limits [L] i32 (<= 0: no limit, otherwise the first `limit` boxes), thresholds [T] f64:
 * device memory.
 *
 * Per cell and image: the valid gts are those with lo <= area <= hi; num_pos counts them over ALL images (the
 * reference adds before its `continue`); an image with no boxes contributes nothing else.  Otherwise G_valid rounds:
 * column maximum per unused gt over the unused boxes (lowest box index among equal maxima, argmax(axis=0)), the gt
 * with the largest column maximum (lowest gt index among equal maxima), one record, gt and box marked used.  An
 * overlap of 0 is a legal match and takes the first unused box.  When the boxes run out before the gts (the
 * reference's assert(gt_ovr >= 0) fires) the remaining rounds record the lowest unused gt with box -1 and overlap -1
 * and add 1 to the cell's flag word; nothing is read or written out of range.
 *
 * Outputs (device; hits, num_pos and flags are zeroed by the call):
 *   hits [A, L, T] i32       records with overlap >= thresholds[t]
 *   num_pos [A, L] i32
 *   flags [A, L] i32         rounds that found no box, 0 for a clean cell
 *   match_gt, match_box [A, L, Gtot] i32, match_ov [A, L, Gtot] f64 (each may be NULL): image i's records of cell
 *          (a, l) in ROUND order from slot gt_image_offsets[i] on: the gt's index within the image's rows, the box's
 *          row, the overlap; the slots of the image that the rounds do not fill hold -1, -1, -1.0.
 * N == 0, P == 0 and Gtot == 0 are valid.  WSSDL_ERR_INVALID_ARGUMENT: negative sizes, P > WSSDL_RECALL_MAX_BOXES,
 * A, L or T < 1, row_stride < 4, both or neither box form, a scale without boxes_f32, gt_image_offsets that do not
 * start at 0, decrease, give an image more than WSSDL_RECALL_MAX_GT rows or do not end at Gtot, a missing pointer,
 * a workspace smaller than wssdl_proposal_recall_workspace_bytes(N, P, Gtot) (pure host; 0 for sizes the op
 * rejects).  Behaviour on non-finite coordinates is unspecified. */
#define WSSDL_RECALL_MAX_GT 1024
#define WSSDL_RECALL_MAX_BOXES 65536
WSSDL_API size_t wssdl_proposal_recall_workspace_bytes(int N, int P, int Gtot);
WSSDL_API int wssdl_proposal_recall(const float *boxes_f32, const float *scale, const double *boxes_f64, int row_stride,
                     const int32_t *counts, int N, int P, const double *gt_boxes, const double *gt_areas,
                     const int32_t *gt_image_offsets_host, int Gtot, const double *area_ranges, int A,
                     const int32_t *limits, int L, const double *thresholds, int T, int32_t *hits, int32_t *num_pos,
                     int32_t *flags, int32_t *match_gt, int32_t *match_box, double *match_ov, void *workspace,
                     size_t workspace_bytes, wssdl_stream_t stream);

/* ---------------------------------------------------------------------- f7 ---
 * Qualitative results: the ground truth and the detections of all N images of a pass drawn over their grey planes in
 * one op (what fast_rcnn/test_bus.py:337-390 and fast_rcnn/train_bus.py:824-870 do per image with matplotlib),
 * csrc/draw_detect.hip.  TWO LAUNCHES whatever N is (one builds the per-image item records, one paints); no
 * read-back, no allocation on the device, capturable.  The semantics are this project's own and exact; matplotlib's
 * anti-aliased rendering is NOT reproduced and parity with its pictures is unpinned.
 *
 * Inputs (device memory unless said otherwise)
 *   arena        all grey planes, u8, one buffer of arena_bytes bytes
 *   items_host   N items of the table below in HOST memory (validated before anything is launched); items_dev: the
 *                caller's device copy of it.  Plane i is arena[offset + y * row_stride + x], y < h, x < w; its picture
 *                is the tight [h, w, 3] u8 array at out[out_offset ...].
 *   gt_boxes [G, 4] f32 in the plane's pixels, gt_classes [G] i32, gt_image_offsets [N + 1] i32 (a host copy that is
 *                validated and a device copy that the kernels read): image i owns rows offsets[i] .. offsets[i+1]-1,
 *                at most WSSDL_DRAW_MAX_GT of them.  A row whose class is outside 0 .. K-1 is not drawn.
 *   dets [N, K-1, P, 5] f32 (x1, y1, x2, y2, score), counts [N, K-1] i32, as the batched post-detection op or a
 *                DetectionAccumulator leave them.  Rows at and beyond counts are never read.
 *   colours [K, 3] u8 (r, g, b) per class; glyphs [n_glyphs, 7] u8: 5x7 bitmaps, one byte per row from the top, bit 4
 *                the left column, in this fixed order: index 0 space, 1 '.', 2 '-', 3 '_', 4..13 '0'..'9', further
 *                ones (14..39 'a'..'z') as the caller likes; labels [K, WSSDL_DRAW_LABEL_LEN] u8 glyph indices per
 *                class, terminated by 255 (an index >= n_glyphs paints nothing).
 *   style        HOST pointer, read during the call.  line_width odd 1..15 (default 3), dash_on 1..255 (11), dash_off
 *                0..255 (5), glyph_scale 1..4 (2), tag_pad 0..15 (3), tag_dy 0..64 (4), max_draw 0..192 (10),
 *                vis_thresh not NaN (0.5).
 * Output: out, u8, out_bytes bytes.  Bytes outside every image are not written.
 *
 * Per image, in this painting order (later items go over earlier ones):
 *   1. every pixel starts as (g, g, g);
 *   2. the image's ground-truth boxes in table order: a solid outline in the class colour, no tag;
 *   3. detections class by class j = 1 .. K-1 and within a class by row: rows p = 0 .. min(max_draw, counts[i, j-1],
 *      P) - 1 are candidates; a row is drawn only if its score > vis_thresh (f32 compare, strict, false for NaN);
 *      counts[i, 0] == -1 (the batched op's overflow flag) draws no detection of image i.  A drawn row gets a dashed
 *      outline in the class colour, then its tag, then its text.
 * Outline: corners X1 = rint(x1) and so on (round half to even of the f32).  A box with a non-finite coordinate or one
 * of |v| >= 2^24, or with X2 < X1 or Y2 < Y1, is skipped.  With hw = (line_width - 1) / 2 pixel (x, y) is on the outline
 * when X1-hw <= x <= X2+hw and Y1-hw <= y <= Y2+hw and not (X1+hw < x < X2-hw and Y1+hw < y < Y2-hw).  Dashed: a
 * pixel of a horizontal band (|y-Y1| <= hw or |y-Y2| <= hw; the corners count as horizontal) is on when
 * (x - (X1-hw)) mod (dash_on + dash_off) < dash_on, every other outline pixel when (y - (Y1-hw)) mod (dash_on +
 * dash_off) < dash_on.  An on pixel becomes the class colour; pixels outside the image are dropped.
 * Text: the class label, a space, the score as d.ddd ('{:s} {:.3f}').  The decimals come from the f32's bits: with
 * score = m * 2^-s (m the 24-bit significand, or the subnormal one) n = round-half-even(m * 1000 / 2^s) in 64-bit
 * integers, n = 0 once s > 40, and the text is n / 1000 '.' n % 1000 (three digits).  Outside [0, 1] the text is
 * unspecified (one leading digit, sign dropped); no access leaves its arrays.
 * A glyph cell is 5x7 bits times glyph_scale, the advance 6 * glyph_scale: Wt = n_chars * 6 * glyph_scale -
 * glyph_scale, Ht = 7 * glyph_scale.  The tag is [X1, X1 + Wt + 2*tag_pad) x [Y1 + tag_dy, Y1 + tag_dy + Ht +
 * 2*tag_pad): every pixel of it inside the image becomes (o + colour + 1) >> 1 per channel, then every set glyph bit
 * inside the image (255, 255, 255); the text's origin is the tag's top-left plus tag_pad.
 *
 * WSSDL_ERR_INVALID_ARGUMENT, nothing launched: N < 1 or > 65535, K < 2 or > 65, G or P < 0, n_glyphs <
 * WSSDL_DRAW_MIN_GLYPHS or > 254, a null pointer where data is needed, h / w < 1, row_stride < w, a plane or an output
 * image that leaves its arena, output images that overlap, more than WSSDL_DRAW_MAX_GT boxes in one image, (K-1) *
 * max_draw > WSSDL_DRAW_MAX_DETS, a style value outside its range, gt_image_offsets (host) that are not non-decreasing
 * from 0 to G.  WSSDL_ERR_WORKSPACE: a workspace below the workspace query's size for N (pure host; 0 for an N the
 * op rejects). */
#define WSSDL_DRAW_MAX_GT 64
#define WSSDL_DRAW_MAX_DETS 192
#define WSSDL_DRAW_LABEL_LEN 24
#define WSSDL_DRAW_MIN_GLYPHS 14
typedef struct wssdl_draw_item {
    int64_t offset;                  /* bytes into the arena */
    int64_t out_offset;              /* bytes into out */
    int32_t h, w, row_stride, reserved;
} wssdl_draw_item;
typedef struct wssdl_draw_style {
    int32_t line_width, dash_on, dash_off, glyph_scale, tag_pad, tag_dy, max_draw;
    float vis_thresh;
} wssdl_draw_style;
WSSDL_API size_t wssdl_draw_workspace_bytes(int N);
WSSDL_API int wssdl_draw_detections(const uint8_t *arena, size_t arena_bytes, const wssdl_draw_item *items_host,
                     const wssdl_draw_item *items_dev, int N, const float *gt_boxes, const int32_t *gt_classes,
                     const int32_t *gt_image_offsets_host, const int32_t *gt_image_offsets_dev, int G,
                     const float *dets, const int32_t *counts, int K, int P, const uint8_t *colours,
                     const uint8_t *glyphs, int n_glyphs, const uint8_t *labels, const wssdl_draw_style *style,
                     uint8_t *out, size_t out_bytes, void *workspace, size_t workspace_bytes, wssdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WSSDL_BUS_HIP_H */
