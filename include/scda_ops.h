/*
 * scda_ops.h -- C ABI of libscda_ops.so, the MI355X (gfx950) implementation of
 * the SCDA Faster-R-CNN hot path.
 *
 * This is the drop-in boundary: every entry point replaces one function that
 * the reference exported through torch.utils.ffi (cffi) or Cython; the
 * reference declaration it replaces is cited as  <file>:<line>  relative to the
 * reference tree.  INTEGRATION.md shows the ctypes stub that binds each one.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer
 *     (hipMalloc'd / torch CUDA tensor .data_ptr()) unless the name ends in _host
 *   - the caller owns and allocates every output and workspace buffer
 *     (reference convention: Python allocates keep/num_out/output/argmax/...,
 *     extensions/_roi_pooling/functions/roi_pool.py:19-22)
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *     all work is enqueued asynchronously on it, nothing synchronises
 *   - return value: 0 = ok, <0 = error (SCDA_E*), never exit(): the reference's
 *     "1 = ok / 0 = bad shape / exit(-1) on launch failure"
 *     (roi_pooling_cuda.c:20-23, roi_pooling_kernel.cu:117-122) becomes a status
 *   - all tensors are contiguous, row-major, fp32 unless stated
 */
#ifndef SCDA_OPS_H
#define SCDA_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCDA_OK 0
#define SCDA_EINVAL (-1)  /* bad shape / null pointer / unsupported size */
#define SCDA_ELAUNCH (-2) /* hipGetLastError() != hipSuccess after a launch */
#define SCDA_ENODEV (-3)  /* no HIP device */

/* library / device probes (no compute) */
int scda_version(void);
int scda_device_count(void);
const char *scda_last_error(void);

/* launch profiler for the GEMM-class kernels: for every kernel class k whose bit is set in kernel_mask a hipEvent
 * pair is recorded on the launch stream around each launch of that kernel; after a device synchronisation
 * scda_prof_collect() fills, per class k in [0, scda_prof_num_kernels()), the number of launches, their summed
 * duration (ms), algorithmic FLOPs and (bytes may be NULL) algorithmic HBM bytes = operands read once + result written
 * once.  (Event records are queue markers: keep the mask narrow inside timed regions.) */
void scda_prof_enable(unsigned kernel_mask);
int scda_prof_num_kernels(void);
const char *scda_prof_kernel_name(int k);
int scda_prof_collect(long long *launches, double *ms, double *flops, double *bytes);
/* test aid: {tile rows, tile cols, split-K count, 1 = direct-to-LDS kernel family} of the calling thread's most recent conv /
 * GEMM launch (the planner's choice, or the SCDA_PLAN_FORCE="bm,bn,splits" override when that is legal for the shape) */
void scda_debug_last_plan(int *out4);
/* test aid, no GPU needed: the complete launch decision (csrc/launch_plan.h LaunchDecision, its 16 ints in declaration order:
 * family 0 register-staged / 1 direct-to-LDS / 2 bf16 x 9 / 3 small-Cin direct forward, x9 stream-K, bm, bn, splits, k_per_split, nx,
 * ny, grid, swz, parity, nc, ncp, weight-gradient slab depth, reduce / fix-up launch follows, stream-K units per workgroup) the
 * library takes for a convolution (dir 0 forward, 1 data gradient, 2 weight gradient, 3 weight + fused bias gradient) or a dense
 * GEMM.  aligned: every pointer 16-byte aligned and a workspace present.  Nothing is launched or allocated; a 256-CU device is
 * assumed, so the answer does not depend on the machine.  SCDA_PLAN_FORCE and the other plan variables act as in a real launch. */
void scda_debug_plan_conv(int dir, int batch, int Cin, int IH, int IW, int Cout, int KH, int KW, int S, int P, int row_period,
                          int aligned, size_t ws_bytes, int *out16);
void scda_debug_plan_gemm(int M, int N, int K, int lda, int ldb, int ldc, int trans_a, int trans_b, int aligned, size_t ws_bytes,
                          int *out16);
/* which kernels a convolution takes (csrc/launch_plan.h route_conv; no GPU needed): dir 0 forward, 1 data gradient, 2 weight gradient,
 * the shape as the forward convolution has it -> 0 implicit GEMM, 1 Winograd, 2 Winograd on stacked 7 x 7 maps.  *pool (may be NULL):
 * the forward may run conv + activation + 2x2 max-pool as one launch (scda_conv2d_wino_pool_hip); *maps (may be NULL): the image is a
 * stack of that many 7 x 7 maps (row_period 7, IW 7, batch 1), else 0.  SCDA_WINOGRAD=0, SCDA_WINO_STACKED=0 and
 * SCDA_CONV_POOL_FUSE=0 keep the respective path out (the tests' reference paths); scda_conv2d_wino_enabled: SCDA_WINOGRAD is not 0. */
int scda_conv2d_route(int dir, int batch, int Cin, int IH, int IW, int Cout, int KH, int KW, int S, int P, int row_period, int *pool,
                      int *maps);
int scda_conv2d_wino_enabled(void);
/* test aid, no GPU needed: both Winograd launch decisions (csrc/launch_plan.h WinoDecision: tile rows / 32, pixel-block-major XCD order,
 * gm, splits, slabs per split, items per XCD, workgroup slots, persistent form, epilogue 0 plain / 1 mask / 2 pool / 3 split-K slab;
 * WinoWgradDecision: K-slabs, splits, slabs per split, splits per XCD, order as scda_debug_wino_last_order, grid) for
 * y [batch, M, H, W] from x [batch, C, H, W] (stack > 0: that many 7 x 7 maps) and for the weight gradient of the layer with
 * (Cin, Cout) = (C, M), on a 256-CU device.  The SCDA_WINO_* variables act as in a real launch. */
void scda_debug_plan_wino(int batch, int C, int H, int W, int M, int stack, int pool, int masked, int with_db, size_t ws_bytes, int *fwd9,
                          int *wgrad6);
/* test aid: launch order of the calling thread's most recent Winograd launches -- forward / data gradient {tile rows / 32,
 * 1 = contiguous pixel-block runs per XCD, gm (XCDs split gm x 8/gm over m-tile groups x runs; 1 = none), split-K count}, weight
 * gradient {K-splits, 0 = dealt as they come / 1 = whole splits per XCD / 2 = one split + one m-tile group per XCD} */
void scda_debug_wino_last_order(int *out6);
/* ... and whether the calling thread's most recent forward / data-gradient launch was the PERSISTENT form (one workgroup per CU walking
 * the tiles: launches of more 64-row tiles than CUs; SCDA_WINO_PERSIST=0 turns it off): 1 / 0 */
int scda_debug_wino_last_persistent(void);

/* ---------------------------------------------------------------- NMS ---- */
/* replaces  int gpu_nms(THLongTensor* keep, THLongTensor* num_out, THCudaTensor* boxes, float thresh)
 *           extensions/_nms/src/nms_cuda.h:1, nms_cuda.c:17-67, cuda/nms_kernel.cu:26-83
 * boxes   [n,5] (x1,y1,x2,y2,score) sorted by score descending
 * mask_ws  workspace, scda_nms_workspace_bytes(n) bytes
 * keep    int64 [n]   indices of kept boxes, ascending            (device)
 * num_out int64 [1]   number of valid entries in keep             (device)
 * max_keep  <=0: full sweep (reference semantics); >0: stop after max_keep
 *           kept boxes (identical to truncating the full result, which is what
 *           both call sites do: functions/rpn_proposal.py:65-66)
 * Unlike the reference nothing is copied to the host: the greedy sweep
 * (nms_cuda.c:47-58) also runs on the device.                                */
size_t scda_nms_workspace_bytes(int n);
int scda_nms_hip(const float *boxes, int n, float thresh, void *mask_ws, int64_t *keep, int64_t *num_out,
                 int max_keep, void *stream);
/* the same with per-box validity flags (uint8 [n], may be NULL): boxes flagged 0 are treated as absent -- never kept, never
 * suppressing -- and `keep` indexes the ORIGINAL list: the min-size filter of functions/rpn_proposal.py:57-59 without compaction */
int scda_nms_valid_hip(const float *boxes, const unsigned char *valid, int n, float thresh, void *mask_ws, int64_t *keep,
                       int64_t *num_out, int max_keep, void *stream);
/* the pairwise suppression bit-mask alone (upper triangle of col-blocks only):
 * mask uint64 [n, ceil(n/64)]                                                */
int scda_nms_mask_hip(const float *boxes, int n, float thresh, uint64_t *mask, void *stream);
/* S independent score-sorted lists in one mask launch + one sweep launch (one workgroup per list) -- the per-(class, image) calls of
 * functions/predict_bbox.py:29-55 batched.  seg: DEVICE int64 [S][3] = {first row of the list in boxes / keep, its length n, first
 * word of its mask in mask_ws (a list owns n * ceil(n / 64) words)}; max_n = the longest list.  keep [all rows]: each list's kept
 * indices, LOCAL to the list, from its first row on; num_out [S]: the counts. */
int scda_nms_segments_hip(const float *boxes, const long long *seg, int S, int max_n, float thresh, void *mask_ws, int64_t *keep,
                          int64_t *num_out, void *stream);

/* ------------------------------------------------------------ RoIPool ---- */
/* replaces  int roi_pooling_forward_cuda(int ph,int pw,float scale, THCudaTensor* features,
 *               THCudaTensor* rois, THCudaTensor* output, THCudaIntTensor* argmax)
 *           extensions/_roi_pooling/src/roi_pooling_cuda.h:1-2, roi_pooling_kernel.cu:24-125
 * features [B,C,H,W], rois [R,5] (batch,x1,y1,x2,y2), out [R,C,PH,PW],
 * argmax int32 [R,C,PH,PW] (flat index into features, -1 = empty bin; may be NULL) */
int scda_roi_pool_fwd_hip(const float *features, const float *rois, int R, int B, int C, int H, int W, int PH, int PW,
                          float spatial_scale, float *out, int32_t *argmax, void *stream);
/* replaces  int roi_pooling_backward_cuda(..., top_grad, rois, bottom_grad, argmax)
 *           roi_pooling_cuda.h:4-5, roi_pooling_kernel.cu:128-234
 * bottom_grad [B,C,H,W] is fully overwritten (need not be zeroed).
 * Summation order per input element: roi ascending, ph ascending, pw ascending
 * -- the reference's order, so the result is bit-identical.                    */
int scda_roi_pool_bwd_hip(const float *top_grad, const int32_t *argmax, const float *rois, int R, int B, int C, int H,
                          int W, int PH, int PW, float spatial_scale, float *bottom_grad, void *stream);

/* ----------------------------------------------------------- RoIAlign ---- */
/* replaces  roi_align_forward_cuda / roi_align_backward_cuda
 *           extensions/_roi_align/src/roi_align_cuda.h:1-5, roi_align_kernel.cu:15-162
 * out [R,C,AH,AW]; bottom_grad [B,C,H,W] must be zeroed by the caller
 * (reference convention, functions/roi_align.py:40-41; the kernel accumulates) */
int scda_roi_align_fwd_hip(const float *features, const float *rois, int R, int B, int C, int H, int W, int AH, int AW,
                           float spatial_scale, float *out, void *stream);
int scda_roi_align_bwd_hip(const float *top_grad, const float *rois, int R, int B, int C, int H, int W, int AH,
                           int AW, float spatial_scale, float *bottom_grad, void *stream);
/* the same operator with the pooled maps stored CHANNEL-MAJOR: out / top_grad are [C,R,AH,AW].  No reference counterpart: it is
 * the layout the ResNet-C4 RoI head (models/mask_rcnn/resnet.py:140-146, layer4 on R x 7 x 7 maps) runs in here -- viewed as
 * [1, C, R*AH', AW'] every 1x1 convolution and every batch-norm of the head sees one long contiguous row per channel instead of
 * R pieces of 49 floats (see the row_period argument of the conv entry points for the 3x3 convolutions). */
int scda_roi_align_cmajor_fwd_hip(const float *features, const float *rois, int R, int B, int C, int H, int W, int AH, int AW,
                                  float spatial_scale, float *out, void *stream);
int scda_roi_align_cmajor_bwd_hip(const float *top_grad, const float *rois, int R, int B, int C, int H, int W, int AH,
                                  int AW, float spatial_scale, float *bottom_grad, void *stream);

/* --------------------------------------------------------- focal loss ---- */
/* replaces the four functions of extensions/_focal_loss/src/focal_loss_cuda.h:2-43
 * N = rows*num_classes; logits [rows,num_classes]; targets int32 [rows]
 * (-1 ignore, 0 background, 1..C foreground)                                  */
int scda_focal_sigmoid_fwd_hip(int N, const float *logits, const int32_t *targets, float weight_pos, float gamma,
                               float alpha, int num_classes, float *losses /*[N]*/, void *stream);
int scda_focal_sigmoid_bwd_hip(int N, const float *logits, const int32_t *targets, float *dX /*[N]*/,
                               float weight_pos, float gamma, float alpha, int num_classes, void *stream);
int scda_focal_softmax_fwd_hip(int N, const float *logits, const int32_t *targets, float weight_pos, float gamma,
                               float alpha, int num_classes, float *losses /*[rows]*/, float *priors /*[N]*/,
                               void *stream);
int scda_focal_softmax_bwd_hip(int N, const float *logits, const int32_t *targets, float *dX /*[N]*/,
                               float weight_pos, float gamma, float alpha, int num_classes,
                               const float *priors /*[N]*/, float *buff /*[rows]*/, void *stream);

/* -------------------------------------------------------- box overlaps ---- */
/* replaces  int gpu_iou_overlaps(THCudaTensor* b1, THCudaTensor* b2, THCudaTensor* out)
 *           extensions/_bbox_helper/src/bbox_helper_cuda.h:1, cuda/iou_overlap_kernel.cu:33-100
 * (no +1, union clamped to >= 1)                                              */
int scda_iou_overlaps_hip(const float *b1, const float *b2, int size_bbox, int n1, int n2, float *out, void *stream);
/* replaces  cython_bbox.bbox_overlaps(boxes f32[N,4], query f32[K,4]) -> f32[N,K]
 *           extensions/_cython_bbox/cython_bbox.pyx:32-73   (no +1, 0 unless iw>0 and ih>0) */
int scda_bbox_overlaps_hip(const float *boxes, int N, const float *query, int K, float *out, void *stream);

/* ------------------------------------------ box logic on the device ---- */
/* What the reference computes in numpy on the host between the RPN and the RCNN head.  The host keeps
 * the two jobs whose results are observable behaviour of the reference: drawing from numpy's global RNG (it gets two counts
 * back) and ranking scores with numpy's argpartition / argsort.
 *
 * functions/anchor_target.py:38-64 -- labels of one image before sub-sampling (-1 ignore, 0 bg, 1 fg), ascending index lists
 * of the positives / negatives, counts = {#pos, #neg}.  anchors [KA,4] fp32, gts [G,gt_stride>=4] fp32; all buffers are the
 * caller's (best_iou f32 [KA], best_gt i32 [KA], gt_best u32 [G], labels i8 [KA], pos_list / neg_list i32 [KA], counts i32 [2]) */
int scda_anchor_label_hip(const float *anchors, int KA, const float *gts, int G, int gt_stride, float neg_thresh, float pos_thresh,
                          float min_gt_best, float *best_iou, int *best_gt, unsigned *gt_best, signed char *labels, int *pos_list,
                          int *neg_list, int *counts, void *stream);
/* scda_anchor_label_hip with ignore regions (:71-76): ign [I, ign_stride >= 4] fp32 rows (x1, y1, x2, y2, ...), padded zero rows
 * included (the reference filters none here; their IoF is 0).  Per anchor the max over the rows of the IoF of
 * utils/bbox_helper.py:29-45 -- intersection over the ANCHOR's area, no +1, numerator max(xmax - xmin, 0) * max(ymax - ymin, 0),
 * divisor max(area, 1) -- in float64 on anchors64 (the float64 grid [KA,4]; the rows are promoted, as numpy promotes them); where it
 * is > ign_thresh (strict, double) the label becomes -1, after the background assignment and before the two foreground
 * assignments: a foreground anchor inside an ignore region stays foreground.  I has no cap.  I = 0 (ign, anchors64 may be null):
 * the same launches and results as scda_anchor_label_hip, which forwards here. */
int scda_anchor_label_ign_hip(const float *anchors, int KA, const float *gts, int G, int gt_stride, float neg_thresh, float pos_thresh,
                              float min_gt_best, const double *anchors64, const float *ign, int I, int ign_stride, double ign_thresh,
                              float *best_iou, int *best_gt, unsigned *gt_best, signed char *labels, int *pos_list, int *neg_list,
                              int *counts, void *stream);
/* :66-107 -- drop the surplus the host drew (drop_* index INTO pos_list / neg_list, as np.random.choice returns them) and emit
 * cls_targets int64 [A,fh,fw], loc_targets / loc_masks fp32 [4A,fh,fw]; anchors64 = the float64 anchor grid [KA,4] */
int scda_anchor_finalize_hip(signed char *labels, const int *best_gt, const int *pos_list, const int *drop_pos, int n_drop_pos,
                             const int *neg_list, const int *drop_neg, int n_drop_neg, const double *anchors64, const float *gts,
                             int gt_stride, int A, int fh, int fw, long long *cls_targets, float *loc_targets, float *loc_masks,
                             void *stream);
/* functions/rpn_proposal.py:36-60 for the n candidates the host ranked (order i32 [n], anchor indices): decode + clip in float64,
 * props5 fp32 [n,5] = (x1,y1,x2,y2,score), ok u8 [n] = the roi_min_size test.  loc [4A,fh,fw] / prob [2A,fh,fw] are the RPN's
 * NCHW outputs of that image; exp_wh f32 [n,2] = np.exp of the candidates' (dw, dh) evaluated by numpy on the host (numpy's
 * float32 exp is not correctly rounded: only numpy reproduces it).  Then scda_nms_valid_hip(props5, ok, ...) and
 * scda_proposal_gather_hip. */
int scda_proposal_decode_hip(const int *order, const float *exp_wh, int n, const double *anchors64, const float *loc, const float *prob, int A, int fh,
                             int fw, double img_h, double img_w, double min_size, float *props5, unsigned char *ok, void *stream);
/* out6 [max_rows,6] rows i < min(max_rows, *num_keep) = (image_index, props5[keep[i]]) */
int scda_proposal_gather_hip(const float *props5, const long long *keep, const long long *num_keep, float image_index, int max_rows,
                             float *out6, void *stream);
/* RoI sampling for the RCNN head with the candidates resident on the device (functions/proposal_target.py:38-62, one image).
 * Step 1: candidates = the n_prop proposals (rows (b, x1, y1, x2, y2, ...), stride prop_stride) followed by the G ground-truth
 * boxes (rows (x1, y1, x2, y2, class), stride gt_stride), clipped to the image (utils/bbox_helper.py:105-110) -> rois [n_prop+G,4];
 * per candidate the first best gt and its IoU (cython_bbox.pyx:32-73 arithmetic); labels 1 (IoU > pos_thresh) / 0 (neg_lo <= IoU <
 * neg_hi, not foreground) / -1; pos_list / neg_list = the ascending index lists np.where returns, counts [2] their lengths.  The
 * host then orders the negatives as the reference's Python-set arithmetic does, draws np.random.choice, and evaluates the <= 128
 * foreground rows' regression targets with numpy (its float32 log is numpy's own routine). */
int scda_proposal_match_hip(const float *props, int n_prop, int prop_stride, const float *gts, int G, int gt_stride, float img_h,
                            float img_w, float pos_thresh, float neg_hi, float neg_lo, float *rois, float *best_iou, int *best_gt,
                            signed char *labels, int *pos_list, int *neg_list, int *counts, void *stream);
/* scda_proposal_match_hip with ignore regions (:79-86): ign [I, ign_stride >= 4] fp32 rows, already filtered by the host (:82, x2 -
 * x1 > 1).  Per CLIPPED candidate the max IoF over the rows (the rule above, float32 throughout); ign_flags i8 [n_prop+G] = 1 where
 * it is > ign_thresh (strict; the float32 the threshold rounds to, as numpy compares a float32 array), else -1; ign_list i32
 * [n_prop+G] = the ascending indices of the flagged candidates -- np.where(max_iof > t)[0], over foreground, background and
 * neither --, ign_count i32 [2] = {its length, 0}.  labels, pos_list, neg_list and counts are scda_proposal_match_hip's: the host
 * takes the ignored candidates out of the negatives with the reference's own set arithmetic (:87), whose order depends on both
 * sets' sizes.  I has no cap.  I = 0 (ign, ign_flags, ign_list, ign_count may be null and are not touched): the same launches and
 * results as scda_proposal_match_hip, which forwards here. */
int scda_proposal_match_ign_hip(const float *props, int n_prop, int prop_stride, const float *gts, int G, int gt_stride, float img_h,
                                float img_w, float pos_thresh, float neg_hi, float neg_lo, const float *ign, int I, int ign_stride,
                                float ign_thresh, float *rois, float *best_iou, int *best_gt, signed char *labels, int *pos_list,
                                int *neg_list, int *counts, signed char *ign_flags, int *ign_list, int *ign_count, void *stream);
/* Step 2 (:64-136): sel i32 [R] = sampled candidate indices, gt_of i32 [R] = matched gt (-1: background), enc f32 [R,4] = the
 * foreground rows' normalised targets -> rois5 [R,5] = (image_index, box), labels int64 [R], loc_targets / loc_weights [R, 4*C]. */
int scda_proposal_finalize_hip(const float *cand_rois, const int *sel, const int *gt_of, const float *enc, const float *gts,
                               int gt_stride, int R, int num_classes, float image_index, float *rois5, long long *labels,
                               float *loc_targets, float *loc_weights, void *stream);

/* ------------------------------------------- cluster-region generator (cluster_ops.hip) ---- */
/* functions/mask.py:183-237 with the k-means on the device.  The rule restated is scikit-learn 1.7.2's
 * KMeans(n_clusters=k, random_state=0).fit with its defaults (init 'k-means++', n_init 'auto' = 1 run, max_iter 300, tol 1e-4,
 * Lloyd); the device path does not depend on the scikit-learn the process would import.
 *   1. points     X[i] = ((x2 + x1) / 2, (y2 + y1) / 2) in float32 from the RoI rows (b, x1, y1, x2, y2, ...), stride roi_stride
 *   2. tolerance  tol_abs = 1e-4 * mean(var(X, axis=0))
 *   3. centring   mean = X.mean(axis=0) (rounded to float32); all work is on Xc = X - mean (a float32 subtraction);
 *                 centres out = float32(centre) + mean, a float32 addition
 *   4. seeding    (_kmeans_plusplus) every draw comes from ONE np.random.RandomState(0) that KMeans re-creates per fit, so the draws
 *                 are constants of (N, k): first_index = searchsorted(cdf, random_sample(), side='right') with cdf the normalised
 *                 float64 cumsum of p = 1/N, then t = trials = 2 + int(ln k) uniforms per further centre: uniforms_host [k-1][t]
 *                 (a HOST array, passed on as kernel arguments).  closest = squared distance to the nearest chosen seed, pot = sum
 *                 of closest; the t candidates of a round are searchsorted(cumsum(closest), u * pot) (side 'left'), clipped to N - 1,
 *                 the cumsum sequential and float64 (stable_cumsum); the candidate whose min(closest, distance to it) sums to the
 *                 lowest potential wins, the first one on a tie
 *   5. Lloyd      label = the first minimum of the squared distance to each centre; each centre becomes the mean of its members;
 *                 after that: labels equal to the iteration before's -> stop (strict convergence: the means just computed are
 *                 returned, no further E-step); else sum_c |shift_c|^2 <= tol_abs -> stop and run one E-step against the final
 *                 centres; else stop after 300 iterations (and run that E-step).  n_iter counts iterations as sklearn's n_iter_
 *   6. a cluster that goes empty during Lloyd is NOT relocated as sklearn does: status bit 0 is raised and the caller takes the
 *      host path for that call (also when a cluster is empty after the final E-step, where the reference raises)
 *   7. members    row c of members [k,N] = the indices of cluster c ascending, then -1; counts [k] their numbers.  The caller
 *                 takes the first `threshold` of a row, or draws np.random.choice(count, threshold, replace=True) from numpy's
 *                 GLOBAL generator on the host (the reference's observable behaviour) and passes the picks to the gather.
 * Arithmetic: float64 on the float32 centred points, direct squared distances dx * dx + dy * dy, one IEEE operation per operator.
 * Every sum has a fixed order (lane l of one wave adds elements l, l + 64, ... in turn, then an xor butterfly over 32, 16, ... 1),
 * no floating-point atomics: two runs are bit-identical.  ONE launch of ONE workgroup; nothing is allocated, the host is not
 * waited for.  Capacity: N <= scda_kmeans_capacity() (1024) points, k <= 8, k <= N.
 * Outputs (the caller's): centres f32 [k,2], labels i32 [N], counts i32 [k], members i32 [k,N], seed_index i32 [k], n_iter i32 [1],
 * status i32 [1]: 0 ok; bit 0 = a cluster went empty; bit 1 = bad arguments or over capacity (only status and n_iter = 0 are
 * written); bit 2 = a mean or the tolerance of steps 2-3 is not finite, which is the case exactly when a float32 point is NaN or
 * infinite: sklearn refuses such input with a ValueError, so the run ends before the seeding (counts = 0 for all k, n_iter = 0 and
 * status are written, the other outputs keep what they held) and the caller takes the host path, which raises.  Any non-zero
 * status sends the call to the host path.  Bit 0 has two cases, told apart by n_iter: a cluster went empty DURING Lloyd -> the run ends there, only counts = 0
 * (all k), n_iter = 0 and status are written and the other outputs keep what they held; a cluster is empty only AFTER the final
 * E-step -> every output is written and valid (labels, the real counts with a 0 among them, members, seed_index, centres,
 * n_iter >= 1), the flag says that the reference would raise on the empty cluster. */
int scda_kmeans_capacity(void);
int scda_kmeans_hip(const float *rois, int roi_stride, int N, int k, int first_index, const double *uniforms_host, int trials,
                    float *centres, int *labels, int *counts, int *members, int *seed_index, int *n_iter, int *status, void *stream);
/* out [k, threshold, F] (contiguous): out[c, j, :] = feats[row(c, j), :] (feats [N,F] f32, row stride feat_stride elements) with
 * row(c, j) = members[c][j] where counts[c] >= threshold, else members[c][picks[c][j]] (picks i32 [k, threshold], may be NULL when no
 * cluster is short); bit-equal to the index_select it replaces.  A row without a valid source (an empty cluster, a pick outside
 * [0, counts[c])) is filled with zeros.  16-byte accesses when F, feat_stride and both addresses allow it. */
int scda_cluster_gather_hip(const float *feats, long long feat_stride, int N, int F, const int *members, const int *counts,
                            const int *picks_or_null, int k, int threshold, float *out, void *stream);

/* ------------------------------------------- batched inference (infer_ops.hip) ---- */
/* The test-time half of the detector's box logic (functions/rpn_proposal.py with the test config, functions/predict_bbox.py:13-66)
 * for B images at once, with nothing copied to the host and nothing allocated: a fixed-shape batch can be captured into one graph.
 * Tie rules (numpy's orders wherever numpy defines one; every key carries its tie-break, so each result is unique):
 *   RPN top-k        score descending, equal scores by ASCENDING anchor index       (np.argsort(-s, kind='stable')[:n])
 *   per-class sort   score descending, equal scores by DESCENDING row index          (a stable ascending argsort, reversed)
 *   per-image top_n  score descending, equal scores by DESCENDING position in the class-major list of kept rows (the same rule)
 * exp of the RPN's float32 size deltas is the correctly rounded float32 exp here; numpy's float32 exp is its own SIMD routine, a few
 * ulp apart at most, so RPN proposal coordinates may differ from the reference's in their last bits (nothing else does).
 *
 * scda_rpn_topk_hip: prob [B, 2A, fh, fw] soft-maxed objectness (fg score of anchor k = (h * fw + w) * A + a in channel 2a + 1)
 *   -> order i32 [B, n], n = top_n, or KA = A * fh * fw when top_n <= 0 or top_n >= KA (a full sort).  One workgroup per image:
 *   radix select of the n-th key, compaction, a sort in LDS (n <= 6144) or in ws (scda_rpn_topk_workspace_bytes, 0 when n fits). */
size_t scda_rpn_topk_workspace_bytes(int B, int KA, int top_n);
int scda_rpn_topk_hip(const float *prob, int B, int A, int fh, int fw, int top_n, int *order, void *ws, void *stream);
/* scda_proposal_decode_hip over B images with exp evaluated on the device: order i32 [B, n] (anchor indices), loc [B, 4A, fh, fw],
 * prob [B, 2A, fh, fw], image_info [B, info_stride >= 2] (h, w, ...) -> props5 [B, n, 5], ok u8 [B, n] (the roi_min_size test) */
int scda_rpn_decode_batched_hip(const int *order, int n, const double *anchors64, const float *loc, const float *prob, int B, int A,
                                int fh, int fw, const float *image_info, int info_stride, double min_size, float *props5,
                                unsigned char *ok, void *stream);
/* all of functions/rpn_proposal.py:36-66 for B images: top-k, decode + clip + size test, NMS at nms_thresh stopping after
 * post_nms_top_n (P) kept boxes (one scda_nms_valid_hip per image), gather.  Fixed capacity: rois5 [B * P, 5] = (b, x1, y1, x2, y2),
 * props6 [B * P, 6] = (b, x1, y1, x2, y2, score); rows i < counts[b] (i32 [B]) of image b are its proposals in NMS order, the others
 * the degenerate RoI (b, 0, 0, 0, 0) with score 0.  ws: scda_rpn_proposals_workspace_bytes(...) bytes. */
size_t scda_rpn_proposals_workspace_bytes(int B, int A, int fh, int fw, int top_n);
int scda_rpn_proposals_hip(const float *prob, const float *loc, const double *anchors64, int B, int A, int fh, int fw,
                           const float *image_info, int info_stride, int pre_nms_top_n, double min_size, float nms_thresh,
                           int post_nms_top_n, void *ws, float *rois5, float *props6, int *counts, void *stream);
/* functions/predict_bbox.py:13-66 for B images on the fixed-capacity RoIs above: rois [B * P, 5], roi_counts i32 [B] (rows beyond
 * are ignored), prob [B * P, C] soft-maxed, loc [B * P, 4C]; stds_host / means_host: 4 doubles each, HOST memory (the de-normalisation
 * of bbox_normalize_stats_precomputed).  Per (image, class 1..C-1): decode in float64 (float32 deltas * float64 stds + means), clip,
 * drop scores <= score_thresh when score_thresh > 0, sort; NMS at nms_thresh (scda_nms_segments_hip on a device segment table); per
 * image the top_n (> 0) best kept rows -> det [B, top_n, 7] = (b, x1, y1, x2, y2, score, class), det_counts i32 [B], rows beyond the
 * count zero.  ws: scda_box_predict_workspace_bytes(B, P, C) bytes. */
size_t scda_box_predict_workspace_bytes(int B, int P, int C);
int scda_box_predict_hip(const float *rois, const int *roi_counts, int B, int P, const float *prob, const float *loc, int C,
                         const float *image_info, int info_stride, const double *stds_host, const double *means_host,
                         float score_thresh, float nms_thresh, int top_n, void *ws, float *det, int *det_counts, void *stream);
/* Soft-NMS at test time (scda_amd/csrc/soft_nms.hip): extensions/_cython_bbox/cython_nms.pyx:98-203 for S independent lists in one
 * launch, one wave per list, bit for bit.  boxes / seg as scda_nms_segments_hip reads them (lists back to back, seg [S][3] = {first
 * row, length, unused here}); the lists need NOT be sorted.  method 0 hard (ov > Nt drops), 1 linear (ov > Nt: score * (1 - ov)),
 * 2 Gaussian (score * exp(-ov^2 / sigma)); a rescored row is discarded when its score falls below threshold.  keep: from a list's
 * first row on, its surviving rows as LOCAL indices in selection order (the reference's returned `inds`); num_out [S]: their
 * counts; the score column of boxes is rewritten IN PLACE with each surviving row's final score (a discarded row's score is
 * unspecified), so boxes[first + keep[j]] is the reference's j-th returned row.  No workspace.  A list of length 0 gives count 0.
 * Capacity: max_n <= scda_soft_nms_capacity() = 2048 rows per list (its working copy fills 48 KB of LDS); a larger max_n, S <= 0 or
 * a method outside 0..2 returns SCDA_EINVAL before anything is launched.  A list LONGER than max_n is cut to its first max_n rows:
 * the sweep runs on those alone, the rows beyond them are neither read nor written and never appear in keep.  Non-finite input
 * follows the reference's own comparisons.  Selection is `maxscore < boxes[pos, 4]` from maxscore = boxes[i, 4]: a NaN score at the
 * head of the live range is selected, a NaN score anywhere else is never greater (it is selected once it stands at the head), +-inf
 * order as numbers; a rescored NaN is not below the threshold, so it stays.  Overlap uses the reference's inline min / max (`a if
 * a <= b else b`, the selected row's coordinate first), so a row with a NaN coordinate is not touched by any selected row.  Every
 * index and loop bound is independent of the values: the sweep stays within bounds and terminates.  Gaussian caveat: the weight is the DEVICE's double exp rounded to float32, the
 * reference's is glibc's; the two may differ in the last place of the double, which changes the float32 weight only when the value
 * lies within about 2^-53 relative of a float32 rounding midpoint -- about one evaluation in 2^28. */
int scda_soft_nms_capacity(void);
int scda_soft_nms_segments_hip(float *boxes, const long long *seg, int S, int max_n, int method, float sigma, float Nt, float threshold,
                               int64_t *keep, int64_t *num_out, void *stream);
/* scda_box_predict_hip with that sweep in place of scda_nms_segments_hip: the same decode + sort, the soft sweep of every (image,
 * class) list, then the per-image top_n ranked by the RESCORED scores (equal scores: the later row of the class-major list of
 * selections first, as before, a class's rows now standing in selection order).  nms_thresh plays no part, Nt does.  The same ws
 * (scda_box_predict_workspace_bytes; the mask piece goes unused).  P above scda_soft_nms_capacity() or a method outside 0..2 returns
 * SCDA_EINVAL before anything is launched. */
int scda_box_predict_soft_hip(const float *rois, const int *roi_counts, int B, int P, const float *prob, const float *loc, int C,
                              const float *image_info, int info_stride, const double *stds_host, const double *means_host,
                              float score_thresh, int top_n, int method, float sigma, float Nt, float threshold, void *ws, float *det,
                              int *det_counts, void *stream);

/* ---- instance masks of the mask-branch detector (scda_amd/csrc/mask_ops.hip; opt-in: scda_amd.infer.Predictor(masks=True)) ----------
 * The detections as RoIs of the mask head: det [B, top_n, 7] + det_counts i32 [B] (scda_box_predict_hip's outputs) ->
 * rois5 [B * top_n, 5] = (b, x1, y1, x2, y2) and cls i32 [B * top_n]; rows past an image's count are (b, 0, 0, 0, 0), class -1. */
int scda_det_rois_hip(const float *detections, const int *detection_counts, int B, int top_n, float *rois5, int *cls, void *stream);
/* Each RoI's own class plane: logits [R, C, ph, pw] addressed by ELEMENT strides (the tall channel-major view of the mask head or
 * NCHW) + cls i32 [R] -> out [R, ph, pw] contiguous.  sigmoid != 0: 1 / (1 + e), e = the correctly rounded float32 exp(-x), float32
 * add and divide (the Mask R-CNN definition; parity-unpinned: the reference's use of the heat map is in its missing mask_rcnn.py).
 * Rows of class < 0 (padding) or >= C give zeros. */
int scda_mask_select_hip(const float *logits, long long stride_r, long long stride_c, long long stride_h, long long stride_w,
                         const int *cls, int R, int C, int ph, int pw, int sigmoid, float *out, void *stream);
/* functions/mask.py:21-49 (predict_masks) under Pillow >= 7, one plane of [H, W] per RoI.  rois [R, roi_stride >= 5] float32
 * (b, x1, y1, x2, y2, ...), planes [R, ph, pw] float32 (ph, pw <= 32), out: packed == 0: float32 [R, H, W]; packed != 0: uint32
 * [R, H, ceil(W / 32)], bit (c % 32) of word c / 32 = (the float form's value >= threshold) -- outside the windows that value is
 * 0.0f --, bits past W zero.  Every element of `out` is written (no clear needed).  Per RoI:
 *   x1, y1, x2, y2 = the float32 values truncated towards zero; roi_w = x2 - x1 + 1, roi_h = y2 - y1 + 1;
 *   the plane is resized to roi_h x roi_w as Pillow resizes a mode-F image with its default filter (BICUBIC, a = -0.5, support 2):
 *   a horizontal pass into a float32 intermediate [ph, roi_w], then a vertical pass; a pass whose sizes are equal is skipped.  Per
 *   output index xx of an axis n_in -> n_out: scale = n_in / n_out, fs = max(scale, 1), support = 2 fs, center = (xx + 0.5) scale,
 *   xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), n_in),
 *   w[k] = bicubic((k + xmin - center + 0.5) * (1.0 / fs)), ww = their left-to-right sum, w[k] /= ww if ww != 0; the sample is (float)
 *   of the left-to-right double sum of (double)pixel * w[k].  bicubic(x), x = |x|: ((a + 2) x - (a + 3)) x x + 1 below 1,
 *   (((x - 5) x + 8) x - 4) a below 2, else 0.  All in IEEE double, one operation per operator (no FMA contraction): Pillow's result
 *   bit for bit (tests/test_mask_infer_rules.py);
 *   the result lands at rows y1.., columns x1.. of a zero plane.
 * Where the reference would raise (the window leaves the plane) the part outside is DROPPED; roi_w <= 0 or roi_h <= 0, coordinates
 * that are not finite or beyond +-5e8, and rows with cls_or_null[r] < 0 (padding) give an empty mask. */
int scda_mask_paste_hip(const float *rois, int roi_stride, const int *cls_or_null, const float *planes, int R, int ph, int pw, int H,
                        int W, int packed, float threshold, void *out, void *stream);
/* tools/mask_rcnn_train_val.py:422-423 (write_results_to_file: the pasted float mask resized once more to the ORIGINAL image size,
 * then `> mask_thresh`) under Pillow >= 7, one plane of [Ho, Wo] per RoI (scda_amd/csrc/mask_rescale.hip; opt-in:
 * scda_amd.infer.Predictor(masks=True, original_size=(Ho, Wo))).  rois, cls_or_null, planes, ph, pw as scda_mask_paste_hip takes them;
 * image_info float32 DEVICE rows of info_stride >= 5 floats (h, w, resize_scale, origin_h, origin_w), detection r belongs to image
 * b = r / masks_per_image.  Per detection r of image b:
 *   (h, w) = image_info[b][0:2], (oh, ow) = image_info[b][3:5], truncated towards zero;
 *   P [h, w] = the float plane scda_mask_paste_hip (packed == 0) defines for the RoI, taken as the top-left h x w sub-plane of its
 *   [H, W] plane: the window is clipped to h x w, and the resize never reads a column >= w or a row >= h (Pillow clamps the taps to
 *   [0, n_in) of the h x w image, not of the padded batch plane);
 *   O [oh, ow] = P resized under the axis rule stated above for the paste: BICUBIC, a = -0.5, support = 2 max(scale, 1), weights
 *   normalised by their left-to-right double sum, each sample (float) of the left-to-right double sum of (double)pixel * w[k], the
 *   horizontal pass w -> ow into a float32 intermediate [h, ow] first, then the vertical pass h -> oh, a pass of equal sizes skipped
 *   ((oh, ow) == (h, w) gives P itself).  A down-scaled sample has up to ceil(2 n_in / n_out) * 2 + 1 taps.  One IEEE operation per
 *   operator: Pillow's result bit for bit (tests/mask_orig_np.py, tests/test_mask_orig_rules.py).
 * out: packed != 0: uint32 [R, Ho, ceil(Wo / 32)], bit (c % 32) of word c / 32 of row y = (O[y, c] > threshold) -- `>`, the reference's
 * line 423, NOT the `>=` of scda_mask_paste_hip's packed form; packed == 0: float32 [R, Ho, Wo] = O.  Bits and values outside oh x ow
 * are zero.  Every element of out, foot_rois and status is written (no clear needed; graph-capturable, no workspace, one launch).
 * Footprint: an output sample none of whose taps [xmin, xmax) lies inside the RoI's window (clipped to h x w) on either axis is exactly
 * +0.0f, its bit is (0.0f > threshold); the samples with a tap inside form one rectangle, written as foot_rois [R, 5] =
 * (b, fx1, fy1, fx2, fy2), inclusive -- (b, 0, 0, -1, -1) when it is empty -- and only there is anything computed.  foot_rois may be
 * given to scda_mask_rle_hip as its rois hint (with image_info + 3 as its sizes) when threshold >= 0.
 * Limits, reported per image in status int32 [ceil(R / masks_per_image)] (0 = fine; the masks of a flagged image are EMPTY, all words
 * zero whatever the threshold, its foot_rois empty; the other images are unaffected; nothing is read or written out of bounds):
 *   1  oh > Ho or ow > Wo (the capacity of the output planes);
 *   2  oh < 1 or ow < 1;
 *   4  h > 4 oh or w > 4 ow: a down-scale above scda_mask_rescale_max_ratio() = 4.  A workgroup owns 32 output columns and blocks of 4
 *      output rows; its LDS tiles hold the 31 * 4 + 2 * 8 + 1 = 141 columns and 3 * 4 + 2 * 8 + 1 = 29 rows of P those can reach at
 *      ratio 4, and 17 weights per sample;
 *   8  h or w outside [1, H] x [1, W], or a size that is not finite.
 * Empty masks as for scda_mask_paste_hip (cls < 0, an empty or non-finite RoI).  R <= 65535, ph, pw <= 32. */
int scda_mask_rescale_max_ratio(void);
int scda_mask_rescale_hip(const float *rois, int roi_stride, const int *cls_or_null, const float *planes, int R, int ph, int pw, int H,
                          int W, const float *image_info, int info_stride, int masks_per_image, int Ho, int Wo, int packed,
                          float threshold, void *out, float *foot_rois, int *status, void *stream);

/* ---- keypoints of the keypoint-branch detector (scda_amd/csrc/keypoint_ops.hip; opt-in: scda_amd.infer.Predictor(keypoints=True)) ----
 * R x Kp heat maps -> one (x, y, score) row per RoI and keypoint, without writing any image-sized plane.
 *
 * PROVENANCE.  The reference's own heat-map -> keypoint code is in its missing models/mask_rcnn/mask_rcnn.py, so there is no reference
 * keypoint decoder to restate: THE CHOICE OF THIS RULE IS OURS.  It is the one place where the reference takes a head's map to image
 * coordinates, functions/mask.py:21-49 (predict_masks), followed by numpy's argmax, and its parity is pinned bit for bit to exactly
 * that -- predict_masks + np.argmax (tests/golden/keypoints_ref.npz) --, not to a reference keypoint decoder.
 *
 * rois [R, roi_stride >= 5] float32 (b, x1, y1, x2, y2, ...); cls_or_null int32 [R] (< 0: a padding slot); heat float32
 * [R, Kp, ph, pw] addressed by ELEMENT strides (NCHW, or the transposed tall channel-major view of the keypoint head; all >= 0);
 * (H, W): the batch's padded shape; out float32 [R, Kp, 3], every element written.  For RoI r and keypoint k:
 *   1. x1, y1, x2, y2 = the float32 values truncated towards zero; roi_w = x2 - x1 + 1, roi_h = y2 - y1 + 1.  A coordinate that is not
 *      finite or beyond +-5e8, roi_w <= 0 or roi_h <= 0, or cls[r] < 0 gives the row (0, 0, 0).
 *   2. M [roi_h, roi_w] = heat[r, k] resized as scda_mask_paste_hip resizes a plane (Pillow >= 7, mode F, BICUBIC: a horizontal pass
 *      into float32, then a vertical pass, a pass of equal sizes skipped; the axis rule stated there, bit for bit).
 *   3. Only the window pixels with 0 <= x1 + px < W and 0 <= y1 + py < H count (as in the paste); none visible: the row (0, 0, 0).
 *   4. (py, px) = the first maximum of the visible part in row-major order -- np.argmax: a NaN is a maximum, the first NaN wins;
 *      +0.0 and -0.0 are equal.
 *   5. the row is ((float)(x1 + px), (float)(y1 + py), M[py, px]): the third value is the raw resized map value (COCO's OKS ignores a
 *      detection's third value; it is carried because write_results_to_file writes it).
 * Limits: ph, pw <= 64 (the keypoint head gives 56; anything larger returns SCDA_EINVAL, nothing is clamped), R, Kp <= 65535,
 * H * W < 2^31.  workspace: scda_keypoint_decode_workspace_bytes(R, Kp, W) bytes (one (value, position) pair per 128-column strip,
 * keypoint and RoI), fully rewritten by every call.  Two launches, no atomics (two runs give the same bytes), graph-capturable. */
size_t scda_keypoint_decode_workspace_bytes(int R, int Kp, int W);
int scda_keypoint_decode_hip(const float *rois, int roi_stride, const int *cls_or_null, const float *heat, long long stride_r,
                             long long stride_k, long long stride_h, long long stride_w, int R, int Kp, int ph, int pw, int H, int W,
                             void *workspace, float *out, void *stream);

/* ---- training the keypoint branch: the heat-map loss (scda_amd/csrc/keypoint_loss.hip; scda_amd.autograd_ops.keypoint_heatmap_loss) ----
 * PROVENANCE.  The reference's keypoint targets and loss are in its missing models/mask_rcnn/mask_rcnn.py; its driver only names the
 * contract (tools/mask_rcnn_train_val.py:309-329: 'ground_truth_keypoints' [b, max_gts, K, 3] in, a fifth loss out).  THE TARGET RULE AND
 * THE LOSS BELOW ARE OUR CHOICE, parity unpinned.
 *
 * The target rule (host code, dropin.functions.mask.compute_keypoint_targets) is the inverse of the decode above, which resizes a map to
 * a window of roi_w x roi_h pixels.  With M_w x M_h the map size, (x1, y1, x2, y2) the integer-clipped RoI, roi_w = x2 - x1 + 1,
 * roi_h = y2 - y1 + 1 and (kx, ky, v) the keypoint of the RoI's matched ground truth, in float64:
 *   the pair (RoI, keypoint) is COUNTED iff v > 0 and x1 <= kx < x2 + 1 and y1 <= ky < y2 + 1;
 *   then bx = min(floor((kx - x1) * M_w / roi_w), M_w - 1), by likewise with y, and target = by * M_w + bx;
 *   every other pair has target -1.
 *
 * The loss is the soft-max cross-entropy over the HW positions of each counted map (the Mask R-CNN keypoint loss), averaged over the
 * counted pairs:  row_loss = logsumexp(map) - map[target];  out2[0] = sum of row_loss over counted pairs / their number, out2[1] = that
 * number; with no counted pair out2 = (0, 0) and the gradient is all zeros (no division by zero, no NaN).  A target outside [0, HW) is
 * uncounted, whatever its value.
 *
 * heat float32: R x Kp planes of HW contiguous elements each, plane (r, k) at heat + r * stride_r + k * stride_k (ELEMENT strides, >= 0:
 * [R, Kp, h, w], or the transposed channel-major view of the keypoint head, taken as it is).  1 <= HW <= 4096 (the decode's 64 x 64
 * limit; anything larger returns SCDA_EINVAL and nothing is launched).  targets int32 [R * Kp].  stats float32 [R * Kp * 2]: (max,
 * log of the sum of exp(x - max)) per counted map, (0, 0) per uncounted one; row_loss float32 [R * Kp] (0 for uncounted maps); both are
 * fully written.  Forward: one workgroup per map, which reads its map once (uncounted maps are not read), then one single-workgroup
 * launch sums row_loss in a fixed order.  Backward: dheat plane (r, k) at dheat + r * dstride_r + k * dstride_k gets
 * (exp(x - max - logsum) - onehot(target)) * grad_scalar[0] / out2[1] for counted maps and exactly 0.0f for uncounted ones; every plane
 * is fully written, nothing between planes is touched.  grad_scalar: one float32 on the device.  No atomics: the same input gives the
 * same bytes on every launch; graph-capturable. */
int scda_keypoint_ce_fwd_hip(const float *heat, long long stride_r, long long stride_k, int R, int Kp, int HW, const int *targets,
                             float *stats, float *row_loss, float *out2, void *stream);
int scda_keypoint_ce_bwd_hip(const float *heat, long long stride_r, long long stride_k, int R, int Kp, int HW, const int *targets,
                             const float *stats, const float *out2, const float *grad_scalar, float *dheat, long long dstride_r,
                             long long dstride_k, void *stream);

/* ---- COCO run-length results from packed masks (scda_amd/csrc/mask_rle.hip; opt-in: scda_amd.infer.Predictor(masks=True, rle=True)) ----
 * The per-mask primitives of the reference's datasets/pycocotools/common/maskApi.c on scda_mask_paste_hip's packed planes, bit for bit
 * (integers below 2^32 and one IEEE double division; no atomics: two runs give the same bytes).  tests/mask_rle_np.py restates the
 * rules in numpy; tests/golden/mask_rle_ref.npz holds what the reference's C gives.
 *
 * scda_mask_rle_hip: bits uint32 [R, H, Wd] (bit c % 32 of word c / 32 of row y = pixel (y, c)).  The image of mask r is the top-left
 * h_r x w_r sub-plane, 1 <= h_r <= H, 1 <= w_r <= 32 Wd; bits outside it do not count.  (h_r, w_r) = image_info[r / masks_per_image]
 * [0:2] (float32 DEVICE rows of info_stride floats, truncated and clamped to that range), or (h_all, w_all) for every mask when
 * image_info is NULL.  rois_or_null [R, roi_stride >= 5] = the rows given to scda_mask_paste_hip, a HINT: a pasted mask is zero outside
 * the columns of its truncated window, so only those are read.  That holds for planes pasted with threshold > 0 only (at threshold
 * <= 0 the outside is set); for such planes the result is the same with and without the hint.  Outputs per mask r:
 *   n_runs int32 [R]             the TRUE number of runs, also when it exceeds cap_runs -- n_runs[r] > cap_runs is the overflow flag;
 *   counts uint32 [R, cap_runs]  rleEncode (maskApi.c:32-42): pixels in column-major order (index = x * h_r + y); the first run counts
 *                                zeros and may be 0, runs alternate; an empty mask is the single run h_r * w_r;
 *   chars uint8 [R, cap_bytes], n_bytes int32 [R]   rleToString (maskApi.c:203-215) of those counts, no terminator: for run i,
 *                                x = counts[i] - (i > 2 ? counts[i - 2] : 0) as a signed value; repeat c = x & 0x1f, x >>= 5 (arithmetic),
 *                                more = (c & 0x10) ? x != -1 : x != 0, if (more) c |= 0x20, emit c + 48, while more;
 *   area uint32 [R]              rleArea: the sum of the odd runs (= the set pixels of the sub-plane);
 *   bbox uint32 [R, 4]           (x, y, w, h) as rleToBbox (maskApi.c:133-146) computes it FROM THE RUN END POINTS: over every run of
 *                                ones, x and y of its first and of its last pixel enter the min / max, nothing in between.  A run that
 *                                wraps from the bottom of one column into the top of the next therefore contributes only its end points'
 *                                rows: the 10 x 6 mask with [5:, 1] and [:4, 2] set gives (1, 3, 2, 3), not rows 0..9.  This is what
 *                                this pycocotools version computes and what rleIou's box gate sees; it is reproduced on purpose, a
 *                                "tight" box is not what the reference returns.  The columns (x, w) are exact.  Empty mask: 0, 0, 0, 0.
 * counts [r, i >= n_runs[r]] and chars [r, i >= n_bytes[r]] are not written and hold nothing.  On overflow n_bytes[r] = 0 and counts /
 * chars of that mask hold nothing a caller may use; n_runs, area and bbox are exact all the same; the other masks are unaffected.
 * A count difference takes at most scda_mask_rle_max_chars(h, w) = ceil((bitlength(h * w) + 1) / 5) characters (a signed value of
 * bitlength + 1 bits, 5 bits per character; 5 for every plane below 2^24 pixels); cap_bytes >= cap_runs *
 * scda_mask_rle_max_chars(H, 32 Wd) is required, so the string of a mask that fits cap_runs always fits cap_bytes.
 * ws: scda_mask_rle_workspace_bytes(R, H, Wd, cap_runs) bytes, 16-byte aligned.  R, H <= 65535, H * 32 Wd < 2^31.  Four launches, no
 * host wait, no allocation: graph-capturable. */
int scda_mask_rle_max_chars(int h, int w);
size_t scda_mask_rle_workspace_bytes(int R, int H, int Wd, int cap_runs);
int scda_mask_rle_hip(const uint32_t *bits, int R, int H, int Wd, const float *image_info, int info_stride, int masks_per_image,
                      int h_all, int w_all, const float *rois_or_null, int roi_stride, int cap_runs, int cap_bytes, void *ws,
                      int *n_runs, uint32_t *counts, int *n_bytes, unsigned char *chars, uint32_t *area, uint32_t *bbox, void *stream);
/* rleIou (maskApi.c:77-96) of packed masks: dt_bits [M, H, Wd], gt_bits [N, H, Wd], one image size (h, w) for all, iscrowd uint8 [N]
 * (device) or NULL -> iou float64 [N, M] in the reference's layout o[g * M + d] and inter uint32 [N, M], the raw |dt & gt| inside the
 * h x w sub-plane.  i = |dt & gt|; u = iscrowd[g] ? area(dt) : area(dt) + area(gt) - i; o = (double) i / (double) u; o = 0 when i == 0,
 * AND o = 0 wherever the reference's box gate gives 0: bbIou (maskApi.c:110-121) of the two rleToBbox boxes above -- end-point rows
 * included -- has w <= 0 or h <= 0.  (The wrapped mask above as dt and gt = [7:9, 1] give 0.0 although 2 pixels intersect; inter
 * still says 2.)  ws: scda_mask_iou_workspace_bytes(M, N, H, Wd) bytes, 16-byte aligned. */
size_t scda_mask_iou_workspace_bytes(int M, int N, int H, int Wd);
int scda_mask_iou_hip(const uint32_t *dt_bits, int M, const uint32_t *gt_bits, int N, int H, int Wd, int h, int w,
                      const unsigned char *iscrowd_or_null, void *ws, double *iou, uint32_t *inter, void *stream);

/* ---- COCO ground-truth masks from annotations (scda_amd/csrc/mask_poly.hip; opt-in: scda_amd.coco_gt.GroundTruth) --------------------
 * COCO.annToMask of the reference's datasets/pycocotools/coco.py:411-439 -- rleFrPoly (maskApi.c:161-201), rleMerge with intersect = 0
 * (:49-70), frUncompressedRLE and rleDecode (:43-47) -- from vertices / run counts to scda_mask_paste_hip's packed planes, bit for bit
 * (integers plus single IEEE double operations, no FMA contraction).  The only atomics are integer XORs and adds: two runs give the same
 * bytes.  tests/mask_poly_np.py restates the rule in numpy; tests/golden/mask_poly_ref.npz holds what the reference's C gives.
 *
 * Inputs, all DEVICE memory: polygon p has the vertices xy[poly_first[p] .. poly_first[p + 1]) (float64 (x, y) pairs, V in all) and
 * belongs to output plane poly_plane[p]; RLE q has the counts rle_counts[rle_first[q] .. rle_first[q + 1]) (uint32, C in all; a
 * compressed string is decoded on the host first: rleFrString, maskApi.c:217-230) and belongs to plane rle_plane[q].  poly_first,
 * rle_first, poly_plane and rle_plane are non-decreasing.  sizes int32 [N, 2] = (h, w) of the image inside plane n, 1 <= h <= H,
 * 1 <= w <= 32 Wd.  The rule, for one polygon of k vertices in an h x w image:
 *   1. x[j] = (int)(5 * xy[2j] + .5), y[j] likewise (a double multiply, a double add, truncation towards zero); x[k] = x[0], y[k] = y[0].
 *   2. Edge j runs from (x[j], y[j]) to (x[j+1], y[j+1]) and has n_j = max(|dx|, |dy|) + 1 points d = 0 .. n_j - 1 (dx = |xe - xs|,
 *      dy = |ye - ys|): flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye) swaps the ends, t = flip ? n_j - 1 - d : d; if dx >= dy:
 *      s = (double)(ye - ys) / dx, u = t + xs, v = (int)(ys + s * t + .5); else s = (double)(xe - xs) / dy, v = t + ys,
 *      u = (int)(xs + s * t + .5).  The last point of an edge is NOT always the next vertex ((int)(negative + .5) truncates towards 0).
 *   3. dx == dy == 0: the one point is u = xs, v = INT_MIN (s = 0.0 / 0 is NaN and (int)NaN is INT_MIN on the reference's x86-64
 *      build).  A duplicated vertex therefore changes the reference's mask, and it changes this one in the same way.
 *   4. Every point q but the very first has the predecessor p in the concatenated sequence of all edges (point d - 1 of its edge, or
 *      the last point of the edge before).  u_q == u_p gives nothing.  Otherwise xd = (double)(u_q < u_p ? u_q : u_q - 1),
 *      xd = (xd + .5) / 5 - .5; dropped if floor(xd) != xd, xd < 0 or xd > w - 1; yd = (double)min(v_q, v_p), yd = (yd + .5) / 5 - .5,
 *      clamped to [0, h], yd = ceil(yd); the point TOGGLES position (int)xd * h + (int)yd of the column-major pixel sequence
 *      (index = x * h + y).
 *   5. Pixel i, 0 <= i < h * w, is the parity of the number of toggles at positions <= i -- over the LINEAR sequence, not per column:
 *      yd == h toggles the top of the next column, a toggle at h * w does nothing.  (The reference's sort, difference and zero-run
 *      merge, :192-199, amount to this.)
 * An RLE is the same fill with toggles at the running sums of its counts; the pixels behind the last run stay 0 (rleDecode into a
 * zeroed image).  A plane is the union (OR) of the fills of its polygons and RLEs; a plane that nothing maps to is empty.
 * Outputs: bits uint32 [N, H, Wd], bit c % 32 of word c / 32 of row y = pixel (y, c) -- EVERY word is written, bits outside the h x w
 * sub-plane are zero --, and area_or_null uint32 [N] = the set pixels (rleArea).
 * Limits, checked here: N, H <= 65535, H * 32 Wd < 2^31; status < 0 and nothing launched otherwise.  The limits on the DATA -- sizes
 * in range, coordinates finite with |coordinate| <= 65535, the counts of an RLE summing to at most h * w (the reference writes past its
 * buffer there) -- are checked on the host by scda_amd.coco_gt.flatten_annotations, which raises ValueError; the kernels skip a shape or
 * edge that violates them (its plane is then unspecified), so that nothing is read or written out of bounds.
 * ws: scda_mask_frpoly_workspace_bytes(P, Q, H, Wd) bytes (one column-major toggle plane per polygon and RLE), 16-byte aligned.  Two
 * clears and four launches ordered by the kernel boundary alone, no host wait, no allocation: graph-capturable. */
size_t scda_mask_frpoly_workspace_bytes(int P, int Q, int H, int Wd);
int scda_mask_frpoly_hip(const double *xy, int V, const int *poly_first, const int *poly_plane, int P, const uint32_t *rle_counts, int C,
                         const int *rle_first, const int *rle_plane, int Q, const int *sizes, int N, int H, int Wd, void *ws,
                         uint32_t *bits, uint32_t *area_or_null, void *stream);

/* ---- COCO AP on the device (scda_amd/csrc/coco_eval.hip; opt-in: scda_amd.coco_eval.CocoEvaluator) ---------------------------------
 * The detection evaluator of the reference's datasets/pycocotools/cocoeval.py (COCOeval.evaluate / accumulate / summarize, iouType
 * 'bbox' and 'segm', useCats = 1) and bbIou of datasets/pycocotools/common/maskApi.c, bit for bit: integer work plus single IEEE double
 * operations in the reference's order.  The only atomics are integer adds; two runs give the same bytes.  tests/coco_eval_np.py restates
 * the rules in numpy; tests/golden/coco_eval_ref.npz holds what the reference's own code gives.  Thresholds, area ranges and maxDets
 * are DEVICE arrays filled by the host (np.linspace values as Params.setDetParams computes them); the limits are T <= 16 thresholds,
 * A <= 8 area ranges, M <= 4 maxDets, R <= 128 recall thresholds, K <= 255 categories (indices 1..K), D, G <= 1024 detection slots /
 * ground truths per image.  Keypoints (OKS) and useCats = 0 (proposal AR) are stated behind the detection rules below.  Not covered:
 * the keypoint head, useCats = 0 for keypoints, the JSON round trip, annotation loading (annToMask: see above).  No call waits for
 * the host or allocates.
 *
 * scda_coco_det_rows_hip: detections [B, top_n, 7] = (b, x1, y1, x2, y2, score, class) + detection_counts i32 [B] (scda_box_predict_hip's
 *   outputs) -> dt_xywh f64 [B, top_n, 4] = ((double) x1, (double) y1, (double) x2 - (double) x1, (double) y2 - (double) y1), dt_area f64
 *   = w * h, or (double) mask_area_or_null[slot] (uint32 [B, top_n], scda_mask_rle_hip's area) for 'segm'; score f32; cat i32 = the class
 *   when the slot is below its image's count and 1 <= class <= K, else 0 (the slot takes no part).
 * scda_coco_box_iou_hip: bbIou (maskApi.c:110-121) for B images: dt f64 [B, D, 4] and gt f64 [B, G, 4] xywh, iscrowd u8 [B, G], counts
 *   i32 [B] read on the device -> iou f64 [B, G * D], o[g * D + d] per image (D = the slot capacity: the layout scda_mask_iou_hip
 *   writes for M = D detections), written for d < dt_counts[b], g < gt_counts[b].  Per pair, all in double, in this order:
 *   w = fmin(d.x + d.w, g.x + g.w) - fmax(d.x, g.x), h likewise; o = 0 when w <= 0 or h <= 0; i = w * h;
 *   u = iscrowd[g] ? d.w * d.h : d.w * d.h + g.w * g.h - i; o = i / u.
 * scda_coco_match_hip: evaluateImg (cocoeval.py:236-314) for B images in one launch, one workgroup per (image, category k = 1..K), one
 *   lane per (area range a, threshold t).  iou as above (either source).  Per (image, category) with at least one detection or GT:
 *   seen[k - 1] = 1;
 *   detections: the slots of cat == k in descending score order, ties in slot order (the stable mergesort on -score); rank = the
 *     position in that order, written for every such slot; only rank < max_det (= maxDets[-1]) take part;
 *   GTs (rows < gt_counts[b] with gt_cat == k): _ignore = iscrowd || area < aRng[a][0] || area > aRng[a][1] -- both bounds inclusive, an
 *     area equal to a bound is inside --; visited non-ignored first, otherwise in row order (the stable argsort of _ignore);
 *     npig[k - 1, a] += the number of non-ignored ones (integer atomic add);
 *   per (a, t), detections in rank order: iou = min(t, 1 - 1e-10), m = none; for each GT in that order: skip it when it is matched
 *     already and is no crowd; STOP when m is a non-ignored GT and this one is ignored; skip it when ious < iou; else iou = ious, m = it
 *     (so an IoU equal to the threshold matches, and of two GTs with equal IoU the later one wins).  m found: the detection is matched,
 *     its ignore flag is m's _ignore, m is marked matched.  Not found: it is ignored when its area < aRng[a][0] or > aRng[a][1].
 *   Outputs per slot (the rows of its image): rank i32 [B, D]; bits u32 [B, D, A] = matched (bit t) | ignored (bit 16 + t), zero for
 *   rank >= max_det; with dbg_match_or_null i32 [B, D, A, T]: the matched GT's row in its image or -1, written for the slots of cat > 0.
 *   The (image, category)'s IoU block is staged in LDS when it has at most 2048 entries and read from memory otherwise.
 *   npig i32 [K, A] and seen i32 [K] ACCUMULATE over calls: zero them before the first image.
 * scda_coco_accumulate_hip: accumulate (cocoeval.py:316-419) over the rows of n_images images (image_ids i32 [n_images], distinct; cat,
 *   rank, score [n_images, D], bits [n_images, D, A] as written above, in ANY image order).  The reference's concatenation and stable
 *   mergesort on -score is the total order (category, score descending, image id ascending, rank ascending); it is produced by a stable
 *   LSD radix sort, 8 bits per pass: the images by id (4 passes), then the rows in (image, slot) order by score (4 passes) and category
 *   (1 pass) -- within an (image, category) equal scores are in slot order, which is their rank order.  The maxDets subsets are the
 *   rows of rank < maxDets[m] of that one order.  Per (k, a, m, t) over the category's rows: tp = matched && !ignored, fp = !matched &&
 *   !ignored as inclusive integer scans converted to double; rc = tp / npig; pr = tp / (fp + tp + 2.220446049250313e-16); pr replaced
 *   by its right-to-left running maximum; per recall threshold the first index with rc >= thr (searchsorted left) gives precision
 *   [t, r, k, a, m] = pr there and scores [...] = the score there, 0 for every threshold no index satisfies; recall [t, k, a, m] =
 *   rc[last], 0 without detections.  Entries are -1 where seen[k] == 0 or npig[k, a] == 0.  precision / scores f64 [T, R, K, A, M],
 *   recall f64 [T, K, A, M].  ws: scda_coco_accumulate_workspace_bytes(n_images, D, K, A) bytes, 16-byte aligned.
 * scda_coco_summarize_hip: _summarizeDets.  spec i32 [n_stats, 4] (device) = (ap, t, a, m): the mean over the entries > -1 of
 *   precision[t, :, :, a, m] (ap != 0) or recall[t, :, a, m]; t = -1 every threshold, t = -2 none (the reference's np.where found no
 *   such threshold); -1 when no entry qualifies -> stats f64 [n_stats].  The sum is taken in a fixed order (deterministic); it differs
 *   from numpy's pairwise mean by at most 2 N 2^-53 for N averaged entries in [0, 1].  The 12 specs are the host's
 *   (scda_amd.coco_eval.stat_specs) and select maxDets as the reference does: maxDets[2] for stats 1..5 and 8..11, maxDets[0] and
 *   maxDets[1] for stats 6 and 7, and for stat 0 the entry EQUAL to 100 (_summarize's default), none -- t = -2, the stat is -1 -- when
 *   the list holds no 100.
 *
 * Keypoints (iouType 'keypoints', computeOks of cocoeval.py:193-234, Params.setKpParams, _summarizeKps): the same match, accumulate
 * and summarize kernels over an OKS block in place of the IoU block.  Kp <= 32 keypoints (only Kp = 17 with the reference's sigmas is
 * pinned to the reference), A >= 3 area ranges (all, medium, large).
 * scda_coco_kp_rows_hip: the rows of scda_coco_det_rows_hip for keypoint results.  detections [B, top_n, 7] supply score and class (the
 *   corners are not read); keypoints f32 [B, top_n, Kp, 3] = (x, y, anything), each value cast to double.  As loadRes (coco.py:350-357):
 *   x0, x1 = min, max over ALL Kp x values, visible or not, y likewise; dt_xywh = (x0, y0, x1 - x0, y1 - y0), dt_area = (x1 - x0) *
 *   (y1 - y0).  Slots at or past the image's count get zero rows and cat 0 whatever their keypoints hold.
 * scda_coco_oks_hip: computeOks for B images -> oks f64 [B, G * D], o[g * D + d] per image, the layout of scda_coco_box_iou_hip, written
 *   for d < dt_counts[b], g < gt_counts[b] (nothing else is touched).  dt_keypoints f32 [B, D, Kp, 3]; gt_keypoints f64 [B, G, Kp, 3] =
 *   (x, y, v); gt_boxes f64 [B, G, 4] xywh; gt_areas f64 [B, G]; vars f64 [Kp] = (sigmas * 2) ** 2 as numpy computes it.  Per pair, in
 *   double, each line single IEEE operations left to right, nothing contracted:
 *     k1 = the number of vg > 0;
 *     k1 > 0: dx = xd - xg, dy = yd - yg for every keypoint; else x0 = bb.x - bb.w, x1 = bb.x + bb.w * 2, y0 = bb.y - bb.h,
 *       y1 = bb.y + bb.h * 2; dx = fmax(0, x0 - xd) + fmax(0, xd - x1), dy likewise;
 *     e = (dx * dx + dy * dy) / vars / (area_gt + 2.220446049250313e-16) / 2;
 *     oks = (the sum of exp(-e) over the keypoints with vg > 0 when k1 > 0, else over all Kp, in ascending keypoint order) / (k1 > 0 ?
 *       k1 : Kp).
 *   e is the reference's bit for bit; exp is not (numpy's and the device's are each faithful to about 1 ulp, and np.sum adds in another
 *   order): at most 17 terms in [0, 1] keep the difference below 1e-14.  One thread per pair, one workgroup per (image, GT, 256
 *   detection slots); the GT's values and vars are staged in LDS once.  computeOks also cuts the detections at maxDets[-1] behind the
 *   score sort and returns [] when either side is empty: both are what scda_coco_match_hip does already (ranks >= max_det take no part;
 *   without GTs nothing matches), so every pair of the image is written here.
 *   With gt_ignore_or_null u8 [B, G] (then gt_iscrowd u8 and gt_num_keypoints i32 [B, G] are required): gt_ignore[b, g] = iscrowd ||
 *   num_keypoints == 0 for g < gt_counts[b] -- the annotation's OWN num_keypoints field (cocoeval.py:108-112), while k1 above counts
 *   v > 0; the two may disagree in a malformed file and both are kept as the reference keeps them.
 * scda_coco_match_ign_hip: scda_coco_match_hip (the same kernel) with the GT's ignore flag given apart from its iscrowd.
 *   gt_ignore_or_null u8 [B, G]: _ignore = gt_ignore || area outside the range, while "matched already and no crowd" still reads the
 *   raw iscrowd (cocoeval.py:262, 281).  A null pointer means iscrowd: the results of scda_coco_match_hip, byte for byte.
 * The ten specs of _summarizeKps go through scda_coco_summarize_hip (scda_amd.coco_eval.kps_stat_specs): AP, AP50, AP75, APm, APl, AR,
 *   AR50, AR75, ARm, ARl, area indices 0 / 1 / 2, all at the maxDets entry EQUAL to 20 -- none (t = -2, the stat is -1) when the list
 *   holds no 20.
 *
 * Category-agnostic evaluation (useCats = 0, cocoeval.py:99-101, 143, 169-171, 245-247; utils/coco_eval.py:56-58 switches it on for
 * proposals with maxDets [1, 100, 1000]): K = 1 in every result array; per image the detections are the concatenation of the
 * categories' lists in ascending category id, each in the order given, and the GTs likewise.  So score ties are broken by (category
 * ascending, given order) and the GT order -- which decides "the later GT wins at equal IoU" and the order among ignored GTs -- is
 * (category ascending, given order).
 * scda_coco_regroup_hip: that order, made physical BEHIND the IoU (computed in the given order, so 'segm' needs no plane moved) and
 *   BEFORE scda_coco_match_hip, which then runs unchanged with K = 1.  Per image one workgroup: a stable counting sort (LDS histogram,
 *   block scan) of the slots d < dt_counts[b] with 1 <= in_cat <= K and of the GT rows g < gt_counts[b] with 1 <= gt_cat <= K ->
 *   perm_dets i32 [B, D] / perm_gts i32 [B, G]: the given slot / row at each regrouped place, -1 behind the live ones.  The rows
 *   (dt_xywh, dt_area, score; out_gt_area, out_gt_iscrowd) are gathered into that order, cat / out_gt_cat = 1 for the live places and 0
 *   (zero rows) behind; out_iou[g * D + d] = in_iou[perm_gts[g] * D + perm_dets[d]] for the live places.  Inputs and outputs must be
 *   different buffers.  K <= 255, D, G <= 1024.
 * scda_coco_prop_rows_hip: the rows of scda_coco_det_rows_hip from proposals f32 [B, P, 6] = (b, x1, y1, x2, y2, score)
 *   (scda_rpn_proposals_batched_hip's) with cat = 1 below the image's count.  xyxy_as_xywh != 0 takes (x2, y2) as (w, h): the reference's
 *   'proposal' run hands [x1, y1, x2, y2] to COCO as if it were xywh (utils/coco_eval.py:33-36), a defect reproduced only on request.
 * Still not covered: the keypoint head itself, the JSON round trip, useCats = 0 for keypoints (computeOks then finds no GT). */
int scda_coco_det_rows_hip(const float *detections, const int *detection_counts, int B, int top_n, const uint32_t *mask_area_or_null,
                           int K, double *dt_xywh, double *dt_area, float *score, int *cat, void *stream);
int scda_coco_box_iou_hip(const double *dt, const int *dt_counts, const double *gt, const int *gt_counts, const unsigned char *iscrowd,
                          int B, int D, int G, double *iou, void *stream);
int scda_coco_match_hip(const double *iou, int B, int D, int G, const int *dt_counts, const int *dt_cat, const float *score,
                        const double *dt_area, const int *gt_counts, const int *gt_cat, const double *gt_area,
                        const unsigned char *gt_iscrowd, int K, const double *iou_thrs, int T, const double *area_rng, int A, int max_det,
                        int *rank, uint32_t *bits, int *npig, int *seen, int *dbg_match_or_null, void *stream);
int scda_coco_match_ign_hip(const double *iou, int B, int D, int G, const int *dt_counts, const int *dt_cat, const float *score,
                            const double *dt_area, const int *gt_counts, const int *gt_cat, const double *gt_area,
                            const unsigned char *gt_iscrowd, const unsigned char *gt_ignore_or_null, int K, const double *iou_thrs, int T,
                            const double *area_rng, int A, int max_det, int *rank, uint32_t *bits, int *npig, int *seen,
                            int *dbg_match_or_null, void *stream);
int scda_coco_kp_rows_hip(const float *detections, const int *detection_counts, int B, int top_n, const float *keypoints, int Kp, int K,
                          double *dt_xywh, double *dt_area, float *score, int *cat, void *stream);
int scda_coco_oks_hip(const float *dt_keypoints, const int *dt_counts, const double *gt_keypoints, const double *gt_boxes,
                      const double *gt_areas, const int *gt_counts, const double *vars, int Kp, const unsigned char *gt_iscrowd_or_null,
                      const int *gt_num_keypoints_or_null, int B, int D, int G, double *oks, unsigned char *gt_ignore_or_null,
                      void *stream);
int scda_coco_prop_rows_hip(const float *proposals, const int *proposal_counts, int B, int P, int xyxy_as_xywh, double *dt_xywh,
                            double *dt_area, float *score, int *cat, void *stream);
int scda_coco_regroup_hip(int B, int D, int G, int K, const int *dt_counts, const double *in_xywh, const double *in_area,
                          const float *in_score, const int *in_cat, const int *gt_counts, const int *gt_cat, const double *gt_area,
                          const unsigned char *gt_iscrowd, const double *in_iou, double *dt_xywh, double *dt_area, float *score, int *cat,
                          double *out_gt_area, unsigned char *out_gt_iscrowd, int *out_gt_cat, double *out_iou, int *perm_dets,
                          int *perm_gts, void *stream);
size_t scda_coco_accumulate_workspace_bytes(int n_images, int D, int K, int A);
int scda_coco_accumulate_hip(const int *image_ids, int n_images, int D, const int *cat, const int *rank, const float *score,
                             const uint32_t *bits, const int *npig, const int *seen, int K, int T, int A, const double *rec_thrs, int R,
                             const int *max_dets, int M, int max_det_last, void *ws, double *precision, double *recall, double *scores,
                             void *stream);
int scda_coco_summarize_hip(const double *precision, const double *recall, int T, int R, int K, int A, int M, const int *spec,
                            int n_stats, double *stats, void *stream);

/* ---- Cityscapes mAP on the device (scda_amd/csrc/map_eval.hip; opt-in: scda_amd.map_eval.MapEvaluator) -------------------------------
 * The reference's metric: the rows validate() writes (tools/faster_rcnn_train_val.py:826-858) scored by utils/cal_mAP.py (parse_res,
 * calIoU, cal_mAP), and the RPN recall of bbox_helper.compute_recall -- bit for bit: integer work plus single IEEE operations in the
 * reference's order.  The only atomics are integer adds; two runs give the same bytes.  tests/voc_map_np.py restates the rules in numpy;
 * tests/golden/voc_map_ref.npz holds what the reference's own code gives.  Limits: D, G <= 1024 detection / ground-truth slots per
 * image, 2 <= num_classes C <= 256 (classes 1..C-1), 1 <= keep_num <= D.  No call waits for the host or allocates; every capacity
 * violation is refused with SCDA_EINVAL before anything is launched.
 *
 * R1, scda_map_rows_hip (validate() :838-857, then parse_res): detections f32 [B, D, 7] = (b, x1, y1, x2, y2, score, class) and
 *   detection_counts i32 [B] (scda_box_predict_hip's outputs), image_info f32 [B, info_w] = (h, w, ...).  Per image the live rows are
 *   d < detection_counts[b].  rank = a live row's position under the stable sort by descending float32 score (equal scores: the
 *   earlier row first; padding rows keep rank = d, so rank is a permutation of 0..D-1); kept = live && rank < keep_num && 1 <= class
 *   <= C-1 (validate() never writes the other classes).  Each coordinate in float32: x -> fmin(fmax(x, 0), w - 1), y -> fmin(fmax(y,
 *   0), h - 1), then the correctly rounded quotient by image_info[b, scale_column], then truncation toward zero -> box i32 [B, D, 4]
 *   (int(float(str(np.float32))) is that truncation: the shortest repr of a float32 cannot cross an integer).  score f32 (0 for
 *   padding), cls i32 = (int) class of a live row (0 for padding).  The rows of an image in the file are class ascending, then rank
 *   ascending.  validate() orders with argsort()[::-1], whose order among EQUAL scores is numpy's, not this one.  Also resets the
 *   slots' later outputs: tp = 0, dbg_match = -1, dbg_claimed [B, G] = 0.
 * R2, scda_map_match_hip (calIoU, cal_mAP :67-114): one wave per (image, class c = 1..C-1).  gt_boxes i32 [B, G, 5] = (x1, y1, x2, y2,
 *   label), rows < gt_counts[b]; the class's ground truths are those of label == c in row (meta) order; gt_num[c] += their number
 *   (integer atomic add; ACCUMULATES over calls).  The class's kept detections are visited in rank order (= descending score, ties in
 *   row order).  Per detection, over the ground truths in order: ix1 = max(x1, gx1), iy1 = max(y1, gy1), ix2 = min(x2, gx2), iy2 =
 *   min(y2, gy2); the pair counts only if ix1 < ix2 && iy1 < iy2 (both strict); inter = (ix2-ix1+1) * (iy2-iy1+1); IoU = (double) inter
 *   / (double) (a_dt + a_gt - inter) with the +1 areas, integers in int64, one double division.  best starts at -1 and is replaced on
 *   strict > only (the first maximum wins; across lanes: the larger IoU, on equal IoU the smaller index).  tp = 1 iff best >= iou_thr
 *   and that ground truth is unclaimed, which is then claimed; otherwise the detection is a false positive, nothing is claimed, and
 *   there is no second choice.  tp i32 [B, D]; dbg_match_or_null i32 [B, D] = the claimed ground truth's row or -1;
 *   dbg_claimed_or_null i32 [B, G].
 * R4, scda_map_recall_hip (bbox_helper.compute_recall): proposals f32 [B, P, prop_w] (columns 1..4 = the box), rows <
 *   proposal_counts[b]; gts f32 [B, Gr, gt_w] (columns 0..3), rows < gt_counts[b].  Per (ground truth, proposal) the float32 IoU of
 *   scda_bbox_overlaps_hip (no +1; boxes = the ground truth, query = the proposal); a ground truth is recalled if its row maximum is
 *   > 0.5f.  counters i32 [2]: [0] += recalled, [1] += gt_counts[b] (also without proposals) -- integer atomic adds, ACCUMULATE.
 * R3, scda_map_accumulate_hip (cal_mAP :105-131) over the rows of n_images images (score, cls, rank, kept, tp [n_images, D] as written
 *   above, the images in the order they were added).  Per class the kept rows in the order of the reference's stable sort by
 *   descending score -- equal scores keep the image order, then the row order -- produced by the stable LSD radix sort of
 *   csrc/radix_sort.h over the rows in (image, rank) order: 4 passes by score, 1 by class.  tp, fp cumulative counts; rec = tp /
 *   sum_gt[c], prec = tp / (tp + fp) in double; env = the running maximum of prec from the right; ap = rec[0] * env[0] + sum_v (rec[v]
 *   - rec[v-1]) * env[v], summed left to right in double by one lane; max_recall = max(rec), NaN if any rec is NaN.  sum_gt i32 [C] on
 *   the device: the meta file's counts, or gt_num.  A class with rows and sum_gt == 0 gives NaN as IEEE 0 / 0 does; a class without
 *   rows gives ap = max_recall = 0 and rows = 0 (the reference raises ValueError there: np.max of an empty array).  ap, max_recall
 *   f64 [C], rows i32 [C]; entry 0 is 0.  ws: scda_map_accumulate_workspace_bytes(n_images, D) bytes, 16-byte aligned. */
int scda_map_rows_hip(const float *detections, const int *detection_counts, int B, int D, const float *image_info, int info_w,
                      int scale_column, int num_classes, int keep_num, int *box, float *score, int *cls, int *rank, int *kept, int *tp,
                      int *dbg_match_or_null, int G, int *dbg_claimed_or_null, void *stream);
int scda_map_match_hip(const int *box, const int *cls, const int *rank, const int *kept, int B, int D, const int *gt_boxes,
                       const int *gt_counts, int G, int num_classes, double iou_thr, int *tp, int *gt_num, int *dbg_match_or_null,
                       int *dbg_claimed_or_null, void *stream);
int scda_map_recall_hip(const float *proposals, const int *proposal_counts, int B, int P, int prop_w, const float *gts,
                        const int *gt_counts, int Gr, int gt_w, int *counters, void *stream);
size_t scda_map_accumulate_workspace_bytes(int n_images, int D);
int scda_map_accumulate_hip(int n_images, int D, const float *score, const int *cls, const int *rank, const int *kept, const int *tp,
                            const int *sum_gt, int num_classes, void *ws, double *ap, double *max_recall, int *rows, void *stream);

/* ---- Merging sharded evaluators (scda_amd/csrc/eval_merge.hip; StreamingEvaluator.absorb / merge of scda_amd/eval_base.py) -------------
 * Data-parallel validation: every rank fills an evaluator of its own over its shard; the ranks' rows are gathered as [W, cap, ...]
 * (W shards of cap image slots each) and merged into one evaluator, so that scda_map_accumulate_hip / scda_coco_accumulate_hip run
 * unchanged on the merged rows.  What the reference does there: each rank writes results.txt.rank<r>, rank 0 concatenates them with
 * `cat results.txt.rank*` (the shell's order: by the decimal rank STRING, so 0, 1, 10, 2, ... with 11 ranks) and scores the whole;
 * images a DistributedSampler repeats as padding are not removed.  Integer work only; two runs give the same bytes.  No call waits for
 * the host or allocates.  tests/sharded_map_np.py restates the rules in numpy; tests/golden/sharded_map_ref.npz holds what the
 * reference's own cal_mAP gives for the concatenated rank files.  flags i32 [4] on the device, zeroed by the caller before the first
 * merge: [0] = 1 the merged images exceeded max_images, [1] = 1 a duplicate that is not covered, [2] the number of duplicates,
 * [3] the number of merged images when the counts live on the device.
 *
 * M1, scda_eval_place_rows_hip: one row array, as 32-bit words: src [W, cap, row_words] -> dst [max_images, row_words].  order_host
 *   int [W] (host): a permutation of the shards; the merged images are, for k = 0..W-1, the images 0..counts[order[k]]-1 of shard
 *   order[k], and they are written to the slots start, start + 1, ...  Either counts_host_or_null int [W] (host) or
 *   counts_dev_or_null i32 [W] (device) is given.  Host counts: a count outside 0..cap or start + total > max_images is refused with
 *   SCDA_EINVAL before anything is launched; only the total's slots are written.  Device counts: each is clamped to 0..cap; a total
 *   beyond max_images - start sets flags[0] = 1 and the images beyond are dropped; EVERY slot start..max_images-1 is written, the
 *   ones behind the total with an empty row -- fill 0: zeros, 1: word w = w (a rank that is a permutation of the slots), 2: all bits
 *   set (the id -1) -- so that the caller can take max_images as its image count without knowing the total; flags[3] = start + total.
 * M2, scda_eval_sum_counters_hip: dst[j] += sum over the W shards of src[w, j], src i32 [W, n] (gt_num and the recall counters of
 *   scda_map_match_hip / scda_map_recall_hip, npig and seen of scda_coco_match_hip).  A duplicated image's ground truths are therefore
 *   counted once per copy.
 * M3, scda_eval_mark_duplicates_hip: image_ids i32 [n] in merged order.  A stable LSD radix sort (csrc/radix_sort.h, 4 passes) of the
 *   positions by id; a position whose predecessor in that order has the same id >= 0 is a duplicate, and first[position] = the first
 *   position of that id (the head of its run: block_scan256 with the maximum over 256 positions a round, one block); first = -1 for
 *   every other position.  Ids < 0 mean "no identity" and are never duplicates.  flags[2] = the number of duplicates (overwritten);
 *   with raise_on_duplicate != 0 any duplicate sets flags[1] = 1 (COCO: the reference would re-evaluate the image with both copies'
 *   detections, which the stored rows cannot reproduce).  ws: scda_eval_mark_duplicates_workspace_bytes(n) bytes, 16-byte aligned.
 * M4, scda_map_merge_duplicates_hip: cal_mAP with a repeated image: the later copy's rows sort behind the equal-scored rows of the
 *   first copy (the sort is stable, R3), find their best ground truth claimed already or below the threshold, and are false positives.
 *   For every image with first >= 0: tp = 0 for all its rows (kept stays); its box, score (by bits), cls, rank and kept are compared
 *   with the first copy's over all D slots, and any difference sets flags[1] = 1 -- the rule is exact only for equal copies. */
int scda_eval_place_rows_hip(const void *src, int W, int cap, int row_words, const int *order_host, const int *counts_host_or_null,
                             const int *counts_dev_or_null, int start, int max_images, int fill, void *dst, int *flags, void *stream);
int scda_eval_sum_counters_hip(const int *src, int W, int n, int *dst, void *stream);
size_t scda_eval_mark_duplicates_workspace_bytes(int n);
int scda_eval_mark_duplicates_hip(const int *image_ids, int n, void *ws, int *first, int *flags, int raise_on_duplicate, void *stream);
int scda_map_merge_duplicates_hip(const int *first, int n, int D, const int *box, const float *score, const int *cls, const int *rank,
                                  const int *kept, int *tp, int *flags, void *stream);

/* ------------------------------------------------- convolution / GEMM ---- */
/* The reference reaches these through torch.nn (cuDNN / cuBLAS): nn.Conv2d in
 * models/faster_rcnn/vgg_adver_expansion_cluster.py:101-114 (VGG body),
 * models/head.py:13-18 (RPN), models/faster_rcnn/common_net.py:59-80,251-293 (GAN blocks);
 * nn.Linear in vgg_adver_expansion_cluster.py:46-60 (FC6/FC7/heads).
 * Here they are fp32-MFMA implicit-GEMM kernels; tensors are NCHW fp32, weights
 * [Cout,Cin,KH,KW] exactly as the reference's state_dict stores them.
 * Supported (KH,KW,stride): (3,3,1) (3,3,2) (1,1,1); any padding.
 * act: 0 none, 1 ReLU, 2 LeakyReLU(slope) fused into the epilogue.
 * ws: workspace of scda_conv2d_workspace_bytes(...) bytes (split-K slabs).      */
size_t scda_conv2d_workspace_bytes(int batch, int Cin, int IH, int IW, int Cout, int KH, int KW, int S, int P);
/* GEMM-ready weight: [Cout,Cin,KH,KW] -> the A operand of the forward (for_dgrad = 0, M = Cout, reduced channels
 * C = Cin) or data-gradient (for_dgrad = 1, M = Cin, C = Cout) implicit GEMM.  The layout is private to the library:
 *   C % 16 == 0 : [K][mpad] (M contiguous, padded with zero columns to the 64/128-row tile), K ordered
 *                 channel-block major so that a 16-deep K-slab is 16 consecutive channels at one filter tap
 *   otherwise   : [M][K], K tap-major
 * `out` holds scda_conv2d_packed_elems(...) floats.  Re-pack whenever the weight changes. */
size_t scda_conv2d_packed_elems(int Cout, int Cin, int KH, int KW, int for_dgrad);
int scda_conv2d_pack_weight_hip(const float *w, float *out, int Cout, int Cin, int KH, int KW, int for_dgrad,
                                void *stream);
/* The same packing for MANY weights in one launch (all conv layers of an optimiser group, right after its Adam step), one
 * workgroup per tile, both sides coalesced through LDS: desc = n rows of 7 int64 {source offset in floats from `base`, destination
 * offset in floats from `out`, Cout, Cin, KH*KW, for_dgrad, first tile id}, destinations ascending and back to back, tile ids
 * consecutive: a row owns scda_conv2d_pack_tiles(...) of them; n_tiles = their sum.  for_dgrad 2 / 3 in a row (and in
 * scda_conv2d_packed_elems / scda_conv2d_pack_tiles): the Winograd kernel's transformed filters for the forward / the data gradient
 * (see scda_conv2d_wino_pack_hip below; scda_conv2d_packed_elems returns 0 for a weight that has no such packing: not 3x3, or the
 * reduced channel count is not a multiple of 8). */
long long scda_conv2d_pack_tiles(int Cout, int Cin, int KH, int KW, int for_dgrad);
int scda_conv2d_pack_weights_batched_hip(const float *base, float *out, const long long *desc, int n, long long n_tiles,
                                         void *stream);
/* wp = pack(w, 0) */
/* row_period (all conv entry points): 0 = plain image.  > 0: the image [batch, C, IH, IW] is a vertical STACK of independent
 * maps of `row_period` rows each (IH % row_period == 0; stride 1, 2*P == K-1) and filter taps must not reach from one map into
 * the next -- what a batch of R maps [R, C, period, IW] computes, on the channel-major layout [1, C, R*period, IW].  A call
 * that cannot honour it fails with SCDA_EINVAL. */
int scda_conv2d_fwd_hip(const float *x, const float *wp, const float *bias /*[Cout] or NULL*/, float *y, int batch,
                        int Cin, int IH, int IW, int Cout, int KH, int KW, int S, int P, int row_period, int act, float slope,
                        void *ws, size_t ws_bytes, void *stream);
/* dx [batch,Cin,IH,IW] = conv-transpose of dy [batch,Cout,OH,OW] (fully overwritten); wt = pack(w, 1) */
int scda_conv2d_dgrad_hip(const float *dy, const float *wt, float *dx, int batch, int Cin, int IH, int IW, int Cout,
                          int KH, int KW, int S, int P, int row_period, void *ws, size_t ws_bytes, void *stream);
/* ... with the gradient of the activation that PRODUCED this conv's input folded into the epilogue (replaces one elementwise
 * pass of the reference's autograd: ReLU / LeakyReLU backward of models/faster_rcnn/vgg_adver_expansion_cluster.py:108-111,
 * common_net.py:251-262): dx = dgrad(dy) * (act_src > 0 ? 1 : act_slope); act_src = the conv's input x, or NULL */
int scda_conv2d_dgrad_act_hip(const float *dy, const float *wt, float *dx, int batch, int Cin, int IH, int IW, int Cout,
                              int KH, int KW, int S, int P, int row_period, const float *act_src, float act_slope, void *ws,
                              size_t ws_bytes, void *stream);
/* the same for a conv with <= 4 input channels (image-side layers), direct form, HBM-bound on dy; w = the UNPACKED weight */
int scda_conv2d_dgrad_small_cin_hip(const float *dy, const float *w, float *dx, int batch, int Cin, int IH, int IW, int Cout,
                                    int KH, int KW, int S, int P, void *stream);
/* dw [Cout,Cin,KH,KW] (+)= sum over batch and pixels; deterministic split-K (no atomics) */
int scda_conv2d_wgrad_hip(const float *dy, const float *x, float *dw, int batch, int Cin, int IH, int IW, int Cout,
                          int KH, int KW, int S, int P, int row_period, int accumulate, void *ws, size_t ws_bytes, void *stream);
/* the same plus the bias gradient db[Cout] (+)= sum over batch and pixels of dy, fused: the row sums ride along on the
 * operand fragments of the weight-gradient GEMM and are finished by its split-K reduce (no extra launches, no second read
 * of dy).  Only when scda_conv2d_wgrad_bias_fusable(...) != 0 (OH*OW % 16 == 0, 16-byte aligned dy); otherwise call
 * scda_conv2d_wgrad_hip + scda_bias_grad_nchw_hip. */
int scda_conv2d_wgrad_bias_fusable(int batch, int Cout, int OH, int OW, const float *dy);
int scda_conv2d_wgrad_bias_hip(const float *dy, const float *x, float *dw, float *db, int batch, int Cin, int IH, int IW,
                               int Cout, int KH, int KW, int S, int P, int row_period, int accumulate, int db_accumulate, void *ws,
                               size_t ws_bytes, void *stream);

/* Winograd F(2x2, 3x3) form of the stride-1, pad-1 3x3 convolution on the fp32 MFMA (csrc/conv_wino.hip): 2.25x fewer matrix
 * operations than the implicit GEMM above, fp32 throughout (results differ from the direct form by rounding only: the transforms
 * use the exact constants 0, +-1, +-1/2).  What cuDNN picks for the same nn.Conv2d layers of the reference
 * (vgg_adver_expansion_cluster.py:101-114, head.py:13, common_net.py:59-80).
 *   scda_conv2d_wino_supported: C % 8 == 0, H and W even (8 x 32-pixel blocks, partial on the right / bottom edge), per-image
 *       tensors below 2 GB
 *   u = scda_conv2d_wino_pack_hip(w [Cout,Cin,3,3], for_dgrad): the transformed filters G g G^T in the kernel's MFMA fragment
 *       order, scda_conv2d_wino_packed_elems floats; for_dgrad = 1: the data gradient's filters (rows = Cin, rotated by 180 degrees)
 *   scda_conv2d_wino_hip: y [batch,M,H,W] = act(conv3x3(x [batch,C,H,W]) + bias), optionally * act'(mask_src) as
 *       scda_conv2d_dgrad_act_hip does; forward: (C, M) = (Cin, Cout), u = pack(w, 0); data gradient: x = dy, (C, M) = (Cout, Cin),
 *       u = pack(w, 1).  for_dgrad only labels the launch for scda_prof_*.  ws: split-K slabs (scda_conv2d_workspace_bytes). */
int scda_conv2d_wino_supported(int batch, int C, int H, int W, int M);
size_t scda_conv2d_wino_packed_elems(int Cout, int Cin, int for_dgrad);
int scda_conv2d_wino_pack_hip(const float *w, float *out, int Cout, int Cin, int for_dgrad, void *stream);
int scda_conv2d_wino_hip(const float *x, const float *u, const float *bias, float *y, int batch, int C, int H, int W, int M, int act,
                         float slope, const float *mask_src, float mask_slope, int for_dgrad, void *ws, size_t ws_bytes, void *stream);

/* conv3x3 + bias + activation + nn.MaxPool2d(2, 2) in ONE launch (a Winograd tile is a pooling window): pool_y [batch,M,H/2,W/2] and
 * pool_idx (uint8 winner 0..3, scda_maxpool2x2_fwd_hip's convention: the backward is scda_maxpool2x2_bwd[_relu]_hip as usual); the
 * full-resolution map is never written.  The pools of vgg_adver_expansion_cluster.py:101-114 behind conv1_2 / 2_2 / 3_3 / 4_3. */
/* the same on x [1, C, maps * 7, 7] read as a vertical STACK of `maps` independent 7 x 7 maps (row period 7, see scda_conv2d_fwd_hip's
 * row_period: the channel-major RoI head of models/mask_rcnn/resnet.py:131-148): four maps per pixel block, as 8 x 8 each with row /
 * column 7 discarded; y [1, M, maps * 7, 7].  Needs C % 8 == 0 and tensors below 2 GB. */
int scda_conv2d_wino_stacked_hip(const float *x, const float *u, const float *bias, float *y, int maps, int C, int M, int act, float slope,
                                 const float *mask_src, float mask_slope, int for_dgrad, void *ws, size_t ws_bytes, void *stream);
int scda_conv2d_wino_pool_hip(const float *x, const float *u, const float *bias, float *pool_y, unsigned char *pool_idx, int batch, int C,
                              int H, int W, int M, int act, float slope, void *stream);
/* ... and the weight gradient in the same (transposed) algorithm: dw [Cout,Cin,3,3] (+)= G^T [ sum over 2x2 tiles (A dy A^T) .*
 * (B^T x B) ] G, db [Cout] (+)= sum of dy (fused, may be NULL); deterministic split-K like scda_conv2d_wgrad_hip.
 * scda_conv2d_wino_wgrad_supported: >= 32 channels on both sides, H and W even (K-slabs of 2 x 16 pixels, partial at the right edge). */
int scda_conv2d_wino_wgrad_supported(int batch, int Cin, int H, int W, int Cout);
int scda_conv2d_wino_wgrad_hip(const float *dy, const float *x, float *dw, float *db, int batch, int Cin, int H, int W, int Cout,
                               int accumulate, int db_accumulate, void *ws, size_t ws_bytes, void *stream);
/* ... on dy [1, Cout, maps * 7, 7] / x [1, Cin, maps * 7, 7] read as stacks of `maps` independent 7 x 7 maps (row period 7, see
 * scda_conv2d_wino_stacked_hip): a K-slab is one tile row of a pair of maps; >= 64 channels on both sides */
int scda_conv2d_wino_wgrad_stacked_hip(const float *dy, const float *x, float *dw, float *db, int maps, int Cin, int Cout, int accumulate,
                                       int db_accumulate, void *ws, size_t ws_bytes, void *stream);

/* C[M,N] (row stride ldc) (+)= op(A) op(B) (+ bias) -> act
 * trans_a = 0: A is [M,K] row-major (lda);  1: A is stored [K,M]
 * trans_b = 0: B is [N,K] row-major (ldb);  1: B is stored [K,N]
 * nn.Linear forward  y = x W^T + b : A=x, B=W, trans_a=0, trans_b=0, bias_on_n=1        */
size_t scda_gemm_workspace_bytes(int M, int N, int K);
int scda_gemm_hip(const float *A, const float *B, float *C, int M, int N, int K, int lda, int ldb, int ldc,
                  int trans_a, int trans_b, const float *bias, int bias_on_n, int act, float slope, int accumulate,
                  void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------ layer kernels ---- */
/* HBM-bound pieces the reference reaches through torch.nn / torch.nn.functional.
 * `grad_scalar` arguments are DEVICE pointers to the upstream scalar gradient so
 * that no loss value ever has to visit the host.                                */
/* nn.MaxPool2d(2,2): vgg_adver_expansion_cluster.py:106.  idx uint8 = winner 0..3 */
int scda_maxpool2x2_fwd_hip(const float *x, float *y, uint8_t *idx, int planes, int H, int W, void *stream);
int scda_maxpool2x2_bwd_hip(const float *dy, const uint8_t *idx, float *dx, int planes, int H, int W, void *stream);
/* nn.MaxPool2d(3, stride 2, padding 1), forward (ResNet stem, models/mask_rcnn/resnet.py:120; frozen there, so no backward);
 * y [planes, (H-1)/2+1, (W-1)/2+1] */
int scda_maxpool3x3s2_fwd_hip(const float *x, float *y, int planes, int H, int W, void *stream);
/* y = relu(a + b): residual join of a ResNet block (resnet.py:104-105) */
int scda_add_relu_hip(const float *a, const float *b, float *y, long long n, void *stream);
/* max-pool backward + backward of the ReLU in front of the pool (a window's winner is > 0 iff the pooled value y_pooled is) */
int scda_maxpool2x2_bwd_relu_hip(const float *dy, const uint8_t *idx, const float *y_pooled, float *dx, int planes, int H, int W,
                                 void *stream);
/* mode: 0 ReLU, 1 LeakyReLU(slope), 2 tanh, 3 sigmoid; backward takes the forward OUTPUT y */
int scda_act_fwd_hip(const float *x, float *y, long long n, int mode, float slope, void *stream);
int scda_act_bwd_hip(const float *dy, const float *y, float *dx, long long n, int mode, float slope, void *stream);
/* y = alpha*a + beta*b (b may be NULL) */
int scda_axpby_hip(const float *a, const float *b, float *y, long long n, float alpha, float beta, void *stream);
/* nn.Dropout(p): mask[i] = keep ? 1 : 0 from a counter-based generator; y = mask ? x*scale : 0 */
int scda_dropout_mask_hip(uint8_t *mask, long long n, float p, uint64_t seed, void *stream);
int scda_dropout_apply_hip(const float *x, const uint8_t *mask, float *y, long long n, float scale, void *stream);
/* nn.Dropout with the keep decision recomputed from (seed, index) -- forward and backward, no mask tensor; relu_src (backward,
 * may be NULL): the dropout's input when it is a ReLU output, whose gradient is then applied in the same pass */
int scda_dropout_seeded_hip(const float *x, float *y, long long n, float p, uint64_t seed, float scale, const float *relu_src,
                            void *stream);
/* out1 (+)= scale * sum_c w[c] * mean_i BCE(sigmoid(x[c][i]), t[c or 0][i]): the per-cluster adversarial loss terms of
 * tools/faster_rcnn_train_val.py:584-600,675-687,723-732 in one launch (x [C,n] logits; t [t_rows,n], t_rows 1 or C; w [C] or NULL);
 * prob_out [C,n] (may be NULL) receives sigmoid(x) for the backward, which returns d out1 / d x * grad_scalar */
int scda_sigmoid_bce_rows_fwd_hip(const float *x, const float *t, int t_rows, const float *w, int C, int n, float scale,
                                  int accumulate, float *prob_out, float *out1, void *stream);
int scda_sigmoid_bce_rows_bwd_hip(const float *prob, const float *t, int t_rows, const float *w, int C, int n, float scale,
                                  const float *grad_scalar, float *dx, void *stream);
size_t scda_bias_grad_workspace_bytes(int C);
int scda_bias_grad_nchw_hip(const float *dy, float *db, int B, int C, int HW, int accumulate, float *ws, void *stream);
int scda_colsum_hip(const float *dy, float *db, int M, int N, int accumulate, void *stream);
/* F.cross_entropy(ignore_index), mean over valid rows (faster_rcnn_adver_expansion_reweight_cluster.py:49,63)
 * out2[0] = loss, out2[1] = number of valid rows; probs [R,C] is kept for the backward */
int scda_softmax_ce_fwd_hip(const float *logits, const int64_t *targets, int R, int C, int ignore_index, float *probs,
                            float *out2, void *stream);
int scda_softmax_ce_bwd_hip(const float *probs, const int64_t *targets, int R, int C, int ignore_index,
                            const float *fwd_out2, const float *grad_scalar, float *dlogits, void *stream);
int scda_row_softmax_hip(const float *x, float *y, int R, int C, void *stream);
/* top-1 accuracy in percent over rows whose target != ignore_index (...reweight_cluster.py:249-267) */
int scda_accuracy_hip(const float *logits, const int64_t *targets, int R, int C, int ignore_index, float *out1,
                      void *stream);
/* smooth_l1_loss_with_sigma(pred*mask, target, sigma) * scale  (...reweight_cluster.py:238-246; mask may be NULL) */
size_t scda_smooth_l1_workspace_bytes(void);
int scda_smooth_l1_fwd_hip(const float *pred, const float *mask, const float *target, long long n, float sigma,
                           float scale, float *partial_ws, float *out1, void *stream);
int scda_smooth_l1_bwd_hip(const float *pred, const float *mask, const float *target, long long n, float sigma,
                           float scale, const float *grad_scalar, float *dpred, void *stream);
/* nn.InstanceNorm2d(affine=False) with optional fused activation (act 0/1/2 as for conv) : common_net.py:69-72,288-290 */
int scda_instnorm_fwd_hip(const float *x, float *y, float *mean, float *rstd, int planes, int HW, float eps, int act,
                          float slope, void *stream);
int scda_instnorm_bwd_hip(const float *dy, const float *x, const float *mean, const float *rstd, float *dx, int planes,
                          int HW, int act, float slope, void *stream);
/* The tail of a residual block, x + Dropout(InstanceNorm(h)) (INSResBlock, common_net.py:59-80), as ONE launch each way: the norm of
 * `x`, nn.Dropout(p) with the keep decision of element i recomputed from (seed, i) exactly as scda_dropout_seeded_hip makes it, plus
 * `residual` -- and the matching gradient w.r.t. x (the residual's gradient is dy itself).  Bit-identical to the three launches. */
int scda_instnorm_drop_add_fwd_hip(const float *x, const float *residual, float *y, float *mean, float *rstd, int planes, int HW,
                                   float eps, float p, uint64_t seed, float scale /* 1 / (1 - p) */, void *stream);
int scda_instnorm_drop_bwd_hip(const float *dy, const float *x, const float *mean, const float *rstd, float *dx, int planes, int HW,
                               float p, uint64_t seed, float scale, void *stream);
/* ... with the seed read from DEVICE memory (one uint64): a launch recorded in a hipGraph draws fresh keep decisions on every replay */
int scda_instnorm_drop_add_fwd_dev_hip(const float *x, const float *residual, float *y, float *mean, float *rstd, int planes, int HW,
                                       float eps, float p, const uint64_t *seed_dev, float scale, void *stream);
int scda_instnorm_drop_bwd_dev_hip(const float *dy, const float *x, const float *mean, const float *rstd, float *dx, int planes, int HW,
                                   float p, const uint64_t *seed_dev, float scale, void *stream);
/* nn.BatchNorm2d, training mode, with optional fused activation : common_net.py:214-223 */
size_t scda_batchnorm_workspace_bytes(int B, int C, int HW);   /* 0: the one-workgroup-per-channel form needs none (ws may be NULL) */
int scda_batchnorm_fwd_hip(const float *x, float *y, const float *gamma, const float *beta, float *running_mean,
                           float *running_var, float *save_mean, float *save_rstd, int B, int C, int HW, float eps,
                           float momentum, int act, float slope, float *ws, void *stream);
int scda_batchnorm_bwd_hip(const float *dy, const float *x, const float *gamma, const float *beta, const float *save_mean,
                           const float *save_rstd, float *dx, float *dgamma, float *dbeta, int B, int C, int HW, int act,
                           float slope, int accumulate, float *ws, void *stream);
/* bn3 -> "out += residual" -> ReLU of a bottleneck (models/mask_rcnn/resnet.py:95-104) inside the batch norm's pass:
 * y = relu(bn_train(x) + residual), statistics and running-stat update as scda_batchnorm_fwd_hip; the backward gates dy by y > 0,
 * writes the gated gradient (what the residual branch receives) to d_residual and differentiates the batch norm on it.  Served for the
 * shapes scda_batchnorm_add_relu_ok() accepts (batch 1, HW % 4 == 0, HW <= 40960, 16-byte aligned tensors); SCDA_EINVAL otherwise. */
int scda_batchnorm_add_relu_ok(int B, int HW);
int scda_batchnorm_add_relu_fwd_hip(const float *x, const float *residual, float *y, const float *gamma, const float *beta,
                                    float *running_mean, float *running_var, float *save_mean, float *save_rstd, int B, int C,
                                    int HW, float eps, float momentum, void *stream);
int scda_batchnorm_add_relu_bwd_hip(const float *dy, const float *x, const float *y, const float *gamma, const float *beta,
                                    const float *save_mean, const float *save_rstd, float *dx_or_null, float *d_residual,
                                    float *dgamma, float *dbeta, int B, int C, int HW, int accumulate, void *stream);
/* nn.BatchNorm2d in eval mode (running statistics): out = act((x - mean) * rsqrt(var + eps) * gamma + beta); with dy given,
 * out = the gradient w.r.t. x instead (dy * act'(y) * gamma * rsqrt(var + eps); statistics and affine parameters are constants) */
int scda_batchnorm_eval_hip(const float *x, const float *dy_or_null, float *out, const float *gamma, const float *beta,
                            const float *running_mean, const float *running_var, int B, int C, int HW, float eps, int act,
                            float slope, void *stream);
/* Interpolate(scale_factor=2, 'bilinear', align_corners=True) : common_net.py:160-170 */
int scda_upsample2x_fwd_hip(const float *x, float *y, int planes, int IH, int IW, void *stream);
int scda_upsample2x_bwd_hip(const float *dy, float *dx, int planes, int IH, int IW, void *stream);
/* Instance norm (+ fused activation, or + the residual block's dropout-and-add tail) and the Interpolate behind it as ONE launch
 * (common_net.py:59-80 / :288-289 feeding :279-293 -- in the decoders nothing but the Interpolate reads those norms' outputs):
 * y2 [planes, 2 IH, 2 IW] = upsample2x(instance_norm...(x)), bit-identical to the two launches; mean / rstd as scda_instnorm_fwd_hip
 * (the backward is scda_upsample2x_bwd_hip followed by scda_instnorm_bwd_hip / scda_instnorm_drop_bwd_hip: it needs x, not the small
 * plane).  Planes of 4096 or 16384 elements, IW % 32 == 0, 16-byte aligned tensors (scda_instnorm_up2_supported; SCDA_EINVAL otherwise). */
int scda_instnorm_up2_supported(int IH, int IW);
int scda_instnorm_up2_fwd_hip(const float *x, float *y2, float *mean, float *rstd, int planes, int IH, int IW, float eps, int act,
                              float slope, void *stream);
int scda_instnorm_drop_add_up2_fwd_hip(const float *x, const float *residual, float *y2, float *mean, float *rstd, int planes, int IH,
                                       int IW, float eps, float p, uint64_t seed, float scale /* 1 / (1 - p) */, void *stream);
int scda_instnorm_drop_add_up2_fwd_dev_hip(const float *x, const float *residual, float *y2, float *mean, float *rstd, int planes,
                                           int IH, int IW, float eps, float p, const uint64_t *seed_dev, float scale, void *stream);
/* ... and their backward in one launch: the bilinear gather of dy2 [planes, 2 IH, 2 IW] feeds the norm's gradient in registers;
 * dresidual [planes, IH, IW] = the gathered gradient itself (the residual input's gradient of the tail form).  Bit-identical to
 * scda_upsample2x_bwd_hip followed by scda_instnorm_bwd_hip / scda_instnorm_drop_bwd_hip. */
int scda_instnorm_up2_bwd_hip(const float *dy2, const float *x, const float *mean, const float *rstd, float *dx, int planes, int IH,
                              int IW, int act, float slope, void *stream);
int scda_instnorm_drop_up2_bwd_hip(const float *dy2, const float *x, const float *mean, const float *rstd, float *dx, float *dresidual,
                                   int planes, int IH, int IW, float p, uint64_t seed, float scale, void *stream);
int scda_instnorm_drop_up2_bwd_dev_hip(const float *dy2, const float *x, const float *mean, const float *rstd, float *dx,
                                       float *dresidual, int planes, int IH, int IW, float p, const uint64_t *seed_dev, float scale,
                                       void *stream);
/* F.binary_cross_entropy(p, t), mean : tools/faster_rcnn_train_val.py:584-600,627-628,675-687,723-732 */
int scda_bce_fwd_hip(const float *p, const float *t, int n, float *out1, void *stream);
int scda_bce_bwd_hip(const float *p, const float *t, int n, const float *grad_scalar, float *dp, void *stream);
/* F.avg_pool2d(kernel_size=2, stride=1) of [planes, H+1, W+1] -> [planes, H, W] and its gradient: the pooling half of RoIAlignAvg
 * (extensions/_roi_align/modules/roi_align.py:18-30) */
int scda_avg2x2s1_fwd_hip(const float *x, float *y, int planes, int H, int W, void *stream);
int scda_avg2x2s1_bwd_hip(const float *dy, float *dx, int planes, int H, int W, void *stream);
/* nn.AvgPool2d(full extent) and torch.mean(x, 1) */
int scda_gap_fwd_hip(const float *x, float *y, int planes, int HW, void *stream);
int scda_gap_bwd_hip(const float *dy, float *dx, int planes, int HW, void *stream);
int scda_row_mean_hip(const float *x, float *y, int R, int C, void *stream);
/* torch.optim.Adam step on one flat bucket (tools/faster_rcnn_train_val.py:305-316); step counts from 1 */
int scda_adam_hip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, void *stream);
/* the same step with the cap of the (grid-stride) launch given explicitly; 0 = the library's choice (512 workgroups) */
int scda_adam_limited_hip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, int max_blocks, void *stream);

/* ---- data path: one image from 8-bit interleaved pixels to the network's input tensor ------------------------------
 * datasets/example_dataset.py:76-100,106-131 and datasets/target_dataset.py:23-71: PIL `img.resize((new_w, new_h))`, optional
 * FLIP_LEFT_RIGHT, ToTensor (/ 255) and Normalize ((x - mean) / std).  Pillow's resize is a two-pass separable convolution in
 * fixed point (22 fractional bits) with an 8-bit intermediate image; the caller builds its per-output-coordinate tables
 * (scda_amd/device_image.py: bounds = [xmin, n] pairs, kk = n weights each, `ksize` entries per coordinate) and the two launches
 * reproduce it bit for bit.  src [H, W, C] uint8 (C = 1 or 3: modes L and RGB; PIL pre-multiplies alpha modes before resizing, those are not supported), tmp >= scda_image_resize_tmp_bytes(rows, out_w, C) bytes holds the
 * horizontally resized rows [row0, row0 + rows) -- the rows the vertical tables reach --, out [C, out_h, out_w] float.
 * normalize = 0 stops after ToTensor.  All pointers are device pointers. */
size_t scda_image_resize_tmp_bytes(int rows, int out_w, int C);
int scda_image_resize_normalize_hip(const unsigned char *src, int H, int W, int C, const int *bounds_h, const int *kk_h,
                                    int ksize_h, int out_w, const int *bounds_v, const int *kk_v, int ksize_v, int out_h,
                                    int row0, int rows, unsigned char *tmp, size_t tmp_bytes, int normalize, float mean,
                                    float stdv, int flip, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SCDA_OPS_H */
