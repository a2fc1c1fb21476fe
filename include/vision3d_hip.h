/*
 * vision3d_hip.h -- C ABI of libvision3d_hip.so, the MI355X (gfx950) implementation of the
 * vision3d point-cloud hot path.
 *
 * Conventions:
 *   - plain pointers + sizes, no torch types.  Every pointer is a DEVICE pointer unless its name ends
 *     in `_host`.  The caller owns every buffer, including workspaces (query the *_workspace() size
 *     first); the library never allocates or frees across this boundary (the v3d_second_plan object
 *     below owns a private arena for its own lifetime).
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it -- no call
 *     synchronises the device, data-dependent sizes are returned through device-side counters.
 *   - return value: 0 = ok; < 0 = invalid argument (V3D_E*); > 0 = hipError_t from the runtime.
 *   - stateless and re-entrant: no global mutable state; concurrent calls on different streams are
 *     safe (reference ops are called from 6 DataLoader worker processes, train.py:18).
 *   - row-major contiguous inputs of exactly the stated dtype (reference: raw data_ptr use without
 *     .contiguous(), box_iou_rotated_cuda.cu:81-82).
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference root).
 */
#ifndef VISION3D_HIP_H
#define VISION3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V3D_OK 0
#define V3D_EINVAL (-1)     /* bad size / null pointer / unsupported shape */
#define V3D_EWORKSPACE (-2) /* workspace too small */
#define V3D_EUNSUPPORTED (-3)

typedef void* v3d_stream_t;

/* ---- version probes: vision3d/ops/csrc/vision.cpp:14-58 (get_cuda_version/get_compiler_version) */
const char* v3d_version(void);          /* "vision3d_hip x.y (gfx950)" */
int v3d_hip_runtime_version(void);      /* hipRuntimeGetVersion, replaces cuda_version.cu:6-8 */
const char* v3d_compiler_version(void); /* "clang M.m.p" */
const char* v3d_error_string(int code);

/* ---- A2: pairwise rotated BEV IoU.
 * Replaces detectron2::box_iou_rotated (ops/csrc/box_iou_rotated/box_iou_rotated.h:20-32,
 * box_iou_rotated_cuda.cu:65-121).  boxes (.,5) f32 = (xc, yc, w, h, angle_DEGREES); ious (M,N) f32.
 * Arithmetic follows the HOST branch of box_iou_rotated_utils.h (the CPU path is the parity target). */
int v3d_box_iou_rotated(const float* boxes1, int M, const float* boxes2, int N, float* ious, v3d_stream_t stream);

/* 3-D IoU of (x, y, z, w, l, h, yaw) boxes, z = centre: (M,7) x (N,7) -> (M,N).  BEV intersection area through the operator of
 * v3d_box_iou_rotated on columns (0,1,3,4,6) -- the yaw is read the way that operator reads it -- times the overlap of the z
 * extents, over the union of the volumes.  Replaces the stub vision3d/ops/iou_nms.py:12-13 (`box_iou_rotated_3d` raises
 * NotImplementedError upstream): defined by oracle/v3d_oracle.c:orc_box_iou_rotated_3d. */
int v3d_box_iou_rotated_3d(const float* boxes1, int M, const float* boxes2, int N, float* ious, v3d_stream_t stream);

/* ---- A3: greedy rotated NMS.
 * Replaces detectron2::nms_rotated (ops/csrc/nms_rotated/nms_rotated.h:22-36; CPU semantics
 * nms_rotated_cpu.cpp:7-59: suppress when IoU >= thr).  keep (N) i64 receives indices into the
 * ORIGINAL arrays in decreasing-score order (ties: lower index first); *n_keep (device i32) the count.
 * The reference's CUDA build suppresses on IoU > thr (nms_rotated_cuda.cu:62-63): pass nextafterf(thr, INFINITY) for that rule
 * (the two differ only at IoU == thr exactly; vision3d_amd.ops.nms_rotated(..., rule="cuda") does so).
 * The score sort, the IoU bitmask and the sequential reduction all run on the device. */
size_t v3d_nms_rotated_workspace(int N);
int v3d_nms_rotated(const float* boxes, const float* scores, int N, float iou_threshold, int64_t* keep,
                    int32_t* n_keep, void* workspace, size_t workspace_bytes, v3d_stream_t stream);

/* ---- Proposal stage of the BEV head, fused on the device.
 * Replaces ProposalLayer.inference after the 1x1 heads (detector/proposal.py:39-80: sigmoid, top-k per (frame, class),
 * core/box_encode.py:13-21 decode, ops/iou_nms.py:90-134 coordinate-offset batched rotated NMS, per-class score cut).
 * head_maps (B, n_cls*n_yaw*8, H, W) f32 = [class logits (c, yaw) | box deltas (c, dof, yaw)] channels (the
 * conv_cls | conv_reg outputs concatenated); anchors (n_cls, n_yaw, H, W, 7) f32; score_thresh_host (n_cls) on the
 * HOST.  Outputs are padded to N = B*n_cls*topk rows, sorted by decreasing score; *n_out (device i32) = rows valid.
 * Candidate order inside a group: (score descending, anchor index ascending).  No host synchronisation. */
size_t v3d_proposals_workspace(int B, int n_cls, int topk);
int v3d_proposals(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                  const float* score_thresh_host, float iou_threshold, float* out_boxes, int64_t* out_batch_idx,
                  int64_t* out_class_idx, float* out_scores, int32_t* n_out, void* workspace, size_t workspace_bytes,
                  v3d_stream_t stream);
/* Same, and the last kernel also copies one device word into n_out[1] (n_out then has TWO words): the backbone plan's
 * capacity-overflow summary (v3d_backbone_overflow_flags()[n_layers]), so that the caller's single host read of the frame --
 * the proposal count -- brings the "this frame dropped rows" verdict with it. */
int v3d_proposals_flag(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                       const float* score_thresh_host, float iou_threshold, float* out_boxes, int64_t* out_batch_idx,
                       int64_t* out_class_idx, float* out_scores, int32_t* n_out /*[2]*/, const int32_t* aux_flag,
                       void* workspace, size_t workspace_bytes, v3d_stream_t stream);
/* The first half alone: the decoded top-k candidates before NMS, (B, n_cls, topk) group-major, score descending inside a group
 * (ties: anchor index ascending): boxes (N, 7), scores (N), N = B * n_cls * topk.  What PV-RCNN's stage 2 refines
 * (vision3d_amd/detector/model.py stage1_proposals; the reference's ProposalLayer top-k + decode, detector/proposal.py:61-77).
 * Workspace: v3d_proposals_workspace. */
int v3d_proposals_topk(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                       float* boxes, float* scores, void* workspace, size_t workspace_bytes, v3d_stream_t stream);
/* The same two calls for a head with a direction classifier (cfg.DIRECTION of vision3d_amd/detector/proposal.py; the sine-error loss
 * + direction classifier of the SECOND paper, which upstream's ProposalLayer leaves out): head_maps (B, n_cls*n_yaw*9, H, W) =
 * [cls | reg | dir], the direction logit of anchor (c, yaw) in channel n_cls*n_yaw*8 + c*n_yaw + yaw.  They replace the yaw of
 * core/box_encode.py:21 (anchor yaw + residual, right only modulo pi under that loss) by
 *   remainder(anchor yaw + residual - dir_offset, pi) + dir_offset + pi * [dir logit > 0]     (strict: +-0 and NaN give 0),
 * in [dir_offset, dir_offset + 2 pi), fp32 with (float)M_PI.  Everything else -- selection, the other six components, NMS, score cut,
 * launches, workspace -- is that of v3d_proposals_flag / v3d_proposals_topk. */
int v3d_proposals_dir_flag(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                           const float* score_thresh_host, float iou_threshold, float* out_boxes, int64_t* out_batch_idx,
                           int64_t* out_class_idx, float* out_scores, int32_t* n_out /*[2]*/, const int32_t* aux_flag,
                           void* workspace, size_t workspace_bytes, v3d_stream_t stream, float dir_offset);
int v3d_proposals_dir_topk(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                           float* boxes, float* scores, void* workspace, size_t workspace_bytes, v3d_stream_t stream, float dir_offset);
/* The same two calls for a head with an IoU-aware confidence logit (cfg.IOU_HEAD of vision3d_amd/detector/proposal.py; the rectified
 * score of CIA-SSD / SECOND-IoU, which upstream's ProposalLayer does not have): head_maps (B, n_cls*n_yaw*(9 + with_dir), H, W) =
 * [cls | reg | (dir) | iou], the IoU logit of anchor (c, yaw) in channel n_cls*n_yaw*(8 + with_dir) + c*n_yaw + yaw.  They replace the
 * score of proposal.py:61-80 (the sigmoid class score) BEHIND the top-k selection, which still runs on the class score, by
 *   s' = s * q^iou_power,  q = 1 / (1 + exp(-z)) of the candidate's IoU logit z (NaN counts as -inf), iou_power in 0 .. 8 as that many
 *   successive fp32 multiplications from the left; sentinel rows (s < 0) keep their score;
 * sort, NMS order, score cut and returned scores use s', ties fall to the position in the class-score order.  iou_power = 0 reads no
 * IoU logit.  with_dir != 0: the direction rule of v3d_proposals_dir_* applies as well (else dir_offset is ignored).  _iou_flag replaces
 * v3d_proposals_flag / v3d_proposals_dir_flag, _iou_topk replaces v3d_proposals_topk / v3d_proposals_dir_topk and returns the candidates
 * of a group in the order of s'.  Launches and workspace are theirs. */
int v3d_proposals_iou_flag(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                           const float* score_thresh_host, float iou_threshold, float* out_boxes, int64_t* out_batch_idx,
                           int64_t* out_class_idx, float* out_scores, int32_t* n_out /*[2]*/, const int32_t* aux_flag,
                           void* workspace, size_t workspace_bytes, v3d_stream_t stream, float dir_offset, int with_dir, int iou_power);
int v3d_proposals_iou_topk(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                           float* boxes, float* scores, void* workspace, size_t workspace_bytes, v3d_stream_t stream, float dir_offset,
                           int with_dir, int iou_power);
/* Stage-2 tail on candidates in that layout: refined = core/box_encode.py:13-21 decode of `deltas` against `proposals` (written to
 * `refined` (N, 7) when not NULL), score = sigmoid(conf), coordinate-offset batched rotated NMS per (frame, class) group
 * (ops/iou_nms.py:90-134), per-class score cut; outputs as v3d_proposals (padded to N rows, decreasing score, *n_out valid).
 * The reference's refinement.py:32-33 raises: the definition is the repository's. */
size_t v3d_refine_nms_workspace(int B, int n_cls, int topk);
int v3d_refine_nms(const float* deltas, const float* proposals, const float* conf, int B, int n_cls, int topk,
                   const float* score_thresh_host, float iou_threshold, float* refined, float* out_boxes, int64_t* out_batch_idx,
                   int64_t* out_class_idx, float* out_scores, int32_t* n_out, void* workspace, size_t workspace_bytes,
                   v3d_stream_t stream);

/* ---- IoU-weighted box voting (cfg.BOX_VOTING of vision3d_amd/core/config.py; box voting / weighted NMS / the DI-NMS of CIA-SSD, which
 * upstream's tails -- detector/proposal.py:39-80, plain greedy NMS -- do not have).  boxes (G, T, 7) f32 = (x, y, z, w, l, h, yaw),
 * scores (G, T) f32, out (G, T, 7) f32 (not `boxes`); a group is one (frame, class).  Every candidate k is voted as a centre by the
 * candidates j of its own group (csrc/box_vote_device.h):
 *   u_j = v3d_box_iou_rotated(b_k[0,1,3,4,6], b_j[0,1,3,4,6]), centre first, that operator's bits and angle convention;
 *   j votes iff scores_j > 0, the seven components of b_j are finite and u_j >= iou_threshold (a NaN compares false);
 *   w_j = scores_j * u_j, W = sum w_j;  out[c] = b_k[c] + sum w_j (b_j[c] - b_k[c]) / W for c = 0 .. 5,
 *   out[6] = yaw_k + sum w_j wrap(yaw_j - yaw_k) / W, wrap(d) = d - pi * rintf(d / pi) with pi = (float)M_PI;
 *   W not finite or not > 0: out = b_k with its own bits (the centre votes through its IoU with itself: no special case).
 * fp32 throughout; the sums of a centre are taken in a fixed order (deterministic).  One launch, no workspace, no host
 * synchronisation.  G * T < 2^31. */
int v3d_box_voting(const float* boxes, const float* scores, int G, int T, float iou_threshold, float* out, v3d_stream_t stream);
/* The two fused tails with that vote behind their NMS, ONE more launch each.  Selection, decode, scores, NMS and score cut are those of
 * the entry without the vote and are decided on the un-voted boxes; out_batch_idx, out_class_idx, out_scores, *n_out, the order of
 * the rows and (v3d_refine_nms_vote) `refined` have the bits of that entry.  Every out_boxes row is the vote of the candidates of its
 * (frame, class) group at IoU >= vote_iou, weighted by the scores the NMS ranked by (the rectified score with_iou, sigmoid(conf) in
 * stage 2; sentinel rows, score -1, do not vote).  Voted survivors may overlap again.
 * v3d_proposals_vote_flag: head_maps of v3d_proposals_flag (with_dir = with_iou = 0), v3d_proposals_dir_flag (with_dir != 0) or
 * v3d_proposals_iou_flag (with_iou != 0, iou_power as there; with_iou = 0 ignores it).  Workspace of both: v3d_proposals_vote_workspace. */
size_t v3d_proposals_vote_workspace(int B, int n_cls, int topk);
int v3d_proposals_vote_flag(const float* head_maps, const float* anchors, int B, int n_cls, int n_yaw, int H, int W, int topk,
                            const float* score_thresh_host, float iou_threshold, float* out_boxes, int64_t* out_batch_idx,
                            int64_t* out_class_idx, float* out_scores, int32_t* n_out /*[2]*/, const int32_t* aux_flag,
                            void* workspace, size_t workspace_bytes, v3d_stream_t stream, float dir_offset, int with_dir, int with_iou,
                            int iou_power, float vote_iou);
int v3d_refine_nms_vote(const float* deltas, const float* proposals, const float* conf, int B, int n_cls, int topk,
                        const float* score_thresh_host, float iou_threshold, float* refined, float* out_boxes, int64_t* out_batch_idx,
                        int64_t* out_class_idx, float* out_scores, int32_t* n_out, void* workspace, size_t workspace_bytes,
                        v3d_stream_t stream, float vote_iou);

/* ---- Training-mode BatchNorm1d (+ ReLU) over sparse features (n, C), C a power of two in [4, 256].
 * Replaces nn.BatchNorm1d(eps, momentum) + nn.ReLU on SparseConvTensor.features (detector/sparse_cnn.py:15-30) in
 * training: forward = chunk statistics (two-pass per chunk) + Chan merge in double + fused normalise/affine/ReLU;
 * backward = chunk sums + merge + fused input gradient.  save_mean / save_invstd (C) feed the backward; var_unbiased (C)
 * is what the running_var update uses.  Deterministic.  n = 1 is served (torch refuses it): the variance is 0, so
 * y = relu(beta), var_unbiased = 0 (no n - 1 division), and the backward gives dx = 0. */
size_t v3d_sparse_bn_workspace(int n, int C);
int v3d_sparse_bn_relu_fwd(const float* x, int n, int C, const float* gamma, const float* beta, float eps, int relu, float* y,
                           float* save_mean, float* save_invstd, float* var_unbiased, float* running_mean /*nullable pair:*/,
                           float* running_var /*updated in place with `momentum`*/, float momentum,
                           int64_t* num_batches_tracked /*nullable: += 1*/, void* workspace, size_t workspace_bytes,
                           v3d_stream_t stream);
int v3d_sparse_bn_relu_bwd(const float* x, const float* dy, int n, int C, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, int relu, float* dx, float* dgamma, float* dbeta,
                           void* workspace, size_t workspace_bytes, v3d_stream_t stream);

/* ---- A13: anchor <-> ground-truth target assignment, fused around the rotated-IoU core.
 * Replaces ProposalTargetAssigner.forward (core/proposal_targets.py:10-88) + Matcher (ops/matcher.py:55-130) +
 * box_encode.encode (core/box_encode.py:26-36) without materialising the (n_gt x anchors) IoU matrix.
 * gt_boxes (n_gt,7) f32, gt_class (n_gt) i64, anchors (n_cls, A, 7) f32; iou_thresh_host (n_cls, 2) = [lo, hi] on
 * the HOST: best IoU < lo -> label 0, [lo, hi) -> ignored, >= hi -> +1; allow_low_quality: every anchor attaining
 * some ground truth's best IoU (ties included) is positive.  Outputs (n_cls, A): G_cls i8 in {0,1}, M_cls u8
 * (0 = ignored), G_reg (.,7) f32 VoxelNet encoding at positives / 0, M_reg u8 = positives; matches (nullable) i64 =
 * index of the best ground truth (first maximal in input order; 0 for a class without ground truth).  box_ignore is not an
 * input: the reference never applies it.  Any n_gt >= 0 is accepted: a class's ground truths are staged 128 at a time and a
 * larger class is walked in chunks, with the same result as one pass.  gt_class outside [0, n_cls) belongs to no class.
 * n_cls <= 16 (else V3D_EINVAL).  The workspace may be reused from call to call: nothing in it is read before it is written. */
size_t v3d_assign_targets_workspace(int n_gt, int n_cls, int anchors_per_class);
int v3d_assign_targets(const float* gt_boxes, const int64_t* gt_class, int n_gt, const float* anchors, int n_cls,
                       int anchors_per_class, const float* iou_thresh_host, int allow_low_quality, int8_t* G_cls, uint8_t* M_cls,
                       float* G_reg, uint8_t* M_reg, int64_t* matches, void* workspace, size_t workspace_bytes,
                       v3d_stream_t stream);

/* Direction targets of the anchor head (cfg.DIRECTION; no upstream counterpart -- the reference's ProposalTargetAssigner,
 * core/proposal_targets.py:10-88, emits none): one elementwise launch over the outputs of v3d_assign_targets.  matches / M_reg (n) as
 * that call wrote them, gt_boxes (n_gt, 7).  G_dir (n) i8: at M_reg the direction bit of the matched ground truth's ABSOLUTE yaw t,
 * floor(remainder(t - offset, 2 pi) / pi) in {0, 1} (fp32, (float)M_PI); 0 elsewhere and where a match is not in [0, n_gt). */
int v3d_direction_targets(const float* gt_boxes, int n_gt, const int64_t* matches, const uint8_t* M_reg, int64_t n, float offset,
                          int8_t* G_dir, v3d_stream_t stream);

/* ---- Stage-2 (RoI) targets of PV-RCNN in ONE launch, a workgroup per frame; upstream's core/refinement_targets.py raises
 * (SURVEY.md H11), so the definition is this repository's (tests/refine_targets_ref.py).  No (n x g) matrix, no workspace.
 * proposals (B, n, 7) f32, proposal_class (n) i64; the ground truth of all frames flat -- gt_boxes (n_gt, 7) f32, gt_class
 * (n_gt) i64 --, frame b owning rows [gt_offsets[b], gt_offsets[b + 1]) (gt_offsets: (B + 1) i32 on the DEVICE); draws (B, n) f32.
 * n <= 2 048 (else V3D_EUNSUPPORTED).  Unlike v3d_assign_targets there is no _workspace query: everything is staged in LDS.
 * LIMIT THE CALLER MUST CHECK: a frame may hold at most 128 ground truths.  The frame sizes live on the device (gt_offsets), so
 * the call cannot refuse a larger frame without a host synchronisation: it reads the first 128 of it and returns V3D_OK.  A
 * caller knows its frame sizes on the host (vision3d_amd.core.RefinementTargetAssigner routes such batches to its torch
 * statement).  Per RoI:
 *   iou / match  best box_iou_rotated_3d(roi, gt) over the frame's ground truths of the RoI's class (the bits of
 *                v3d_box_iou_rotated_3d) and the flat index of the first maximal one; no positive overlap: 0 and -1
 *   conf         clamp((iou - conf_lo) / (conf_hi - conf_lo), 0, 1)
 *   G_reg        box_encode.encode(gt[match], roi), yaw residual wrapped to [-pi/2, pi/2), where iou >= reg_iou; else 0
 *   M_cls        sampled: of the foreground (iou >= fg_iou) min(#fg, fg_quota), of the rest min(#bg, rois_per_frame - that), each
 *                by smallest (draw, index); rois_per_frame <= 0: every RoI.  M_reg = M_cls and a box target. */
int v3d_refine_targets(const float* proposals, const int64_t* proposal_class, int B, int n, const float* gt_boxes,
                       const int64_t* gt_class, const int32_t* gt_offsets, int n_gt, const float* draws, float conf_lo, float conf_hi,
                       float reg_iou, float fg_iou, int rois_per_frame, int fg_quota, float* iou, int64_t* match, float* conf,
                       float* G_reg, uint8_t* M_cls, uint8_t* M_reg, v3d_stream_t stream);

/* ---- f2: GT-sampling + global augmentation of one training frame, fused (two launches with sampling, one without).
 * Replaces the chain vision3d/dataset/augmentation.py:31-48 -- SampleAugmentation :117-198 (paste at float64 positions :162-166,
 * collision filter IoU > 1e-2 :140-149, scene points under the pasted rectangles removed :195), FlipAugmentation :78-95,
 * ScaleAugmentation :98-114, RotateAugmentation :51-75 -- which the reference runs in numpy.  The random draws are the caller's
 * (made on the host with the reference's numpy calls in the reference's order): k samples {int32 box_row, pt_start, pt_len, cls;
 * float64 px, py} (32 bytes each, device memory) indexing the flat database tensors db_points (P, 4) / db_boxes (K, 7), flip,
 * the scale factor, cos / sin / value of the float32 rotation angle.  Arithmetic: float64 with sampling (numpy's promotion at the
 * paste), float32 without (k == 0: out_class_idx and work are not touched; any C >= 3).  With sampling C must be 4.
 * Outputs at capacity: out_points (N + sample_points, 4), out_boxes (n + k, 7), out_class_idx (n + k); the ragged sizes are the
 * first int32 words of `work`: {kept samples, kept sample points, kept scene points}, followed by keep[k] (0 / 1 per sample).
 * Result rows: kept scene points in order, then the kept samples' points in draw order; scene boxes, then kept samples' boxes. */
size_t v3d_augment_work_bytes(int N, int n, int k);
int v3d_augment_frame(const float* points, int N, int C, const float* boxes, const int64_t* class_idx, int n,
                      const float* db_points, const float* db_boxes, const void* samples, int k, int sample_points, int flip,
                      double factor, double cos_theta, double sin_theta, double theta, float* out_points, float* out_boxes,
                      int64_t* out_class_idx, void* work, size_t work_bytes, v3d_stream_t stream);

/* ---- f2c: per-object ground-truth noise of B frames (two launches, no host read, no atomic decides a result, deterministic).
 * Replaces nothing upstream -- vision3d/dataset/augmentation.py has no such class --: it is the object noise of VoxelNet section 3.1 /
 * SECOND, defined by this repository (float64 restatement tests/object_noise_ref.py).  The frames are
 * concatenated: points (n_points, C >= 3) f32, boxes (n_boxes, 7) f32 = (x, y, z, w, l, h, yaw), frame b owning the rows
 * [point_offsets_host[b], point_offsets_host[b + 1]) / [box_offsets_host[b], box_offsets_host[b + 1]) -- (B + 1) i32 each, on the
 * HOST.  The caller's draws: trans (n_boxes, T, 3) f32, rot (n_boxes, T) f32.
 *   candidate (i, t)  centre (x_i + trans[i,t,0], y_i + trans[i,t,1]), yaw_i + rot[i,t] (one fp32 add each), size unchanged
 *   collision         the operator of v3d_box_iou_rotated (same device function, candidate first) on (x, y, w, l, yaw_deg),
 *                     yaw_deg = yaw * 57.29577951308232f (one fp32 multiply), > collision_iou: true geometry
 *   selection         per frame, sequentially in box order: chosen[i] = the smallest t whose candidate collides with no box j != i of
 *                     the frame, j < i at its already moved pose, j > i at its original pose; none: chosen[i] = -1, the box stays
 *   out_boxes         (n_boxes, 7): the chosen candidate's x, y, yaw and z_i + trans[i,t,2]; chosen = -1: copied bit for bit
 *   out_points        (n_points, C): a point belongs to the lowest-index box of its frame whose inside test passes -- the test of
 *                     v3d_points_in_boxes(use_z = 1) on the ORIGINAL boxes, same bits --; with (c, s) = (cosf, sinf)(rot[i,t]) taken
 *                     once per box and (cx, cy) the original centre, in uncontracted fp32: dx = x - cx, dy = y - cy,
 *                     x' = ((dx * c - dy * s) + cx) + trans_x, y' = ((dx * s + dy * c) + cy) + trans_y, z' = z + trans_z; columns
 *                     >= 3 and all other points copied, row order and count unchanged (out_points must not alias points)
 *   chosen            (n_boxes) i32
 * Scene points that lie where a box lands are not removed; a box may leave the grid.  Limits: at most 128 boxes per frame,
 * 1 <= T <= 256, B <= 64 -- beyond them V3D_EUNSUPPORTED (the sizes are host data: the call can refuse).  workspace: 16-byte aligned. */
size_t v3d_object_noise_workspace(int n_boxes, int T);
int v3d_object_noise(const float* points, const int32_t* point_offsets_host, const float* boxes, const int32_t* box_offsets_host,
                     int B, int C, const float* trans, const float* rot, int T, float collision_iou, float* out_points,
                     float* out_boxes, int32_t* chosen, void* workspace, size_t workspace_bytes, v3d_stream_t stream);

/* ---- f2b: the GT-sampling database cut out of a batch of annotated frames (three launches per batch, no host read).
 * Replaces DatabaseBuilder._process_item / _demean (vision3d/dataset/augmentation.py:201-243) with its PointsInCuboids call
 * (vision3d/core/geometry.py:27-48; "~10 ms for each scene" in numpy).  points (n_points, C >= 3) f32 = the frames behind each
 * other, point_offsets / box_offsets (n_frames + 1) i32 ON THE DEVICE = first point row / first box of each frame (they tile
 * [0, n_points] / [0, n_boxes]).  box_prep (n_boxes, 8) f64 = (cos yaw, sin yaw, x, y, w, l, z - h / 2, z + h / 2), evaluated by the
 * caller with numpy in the dtype of its boxes and widened (float64 annotation boxes, kitti_dataset.py:75-79: float64 cos / sin;
 * float32 boxes: float32 values, which reproduces v3d_points_in_boxes); the corners are built from it with multiplies and adds.
 * Inside test: geometry.py:37-48 in float64 (strict z limits, four strict cross products against the counter-clockwise corners).
 * A box is kept iff it holds MORE than min_pts points (:232-234).  Outputs: counts (n_boxes) = points inside each box, kept or not;
 * starts (n_boxes) = first output row of a kept box, -1 if dropped; out_points (cap, C) = the kept boxes' points behind each other
 * -- frames in batch order, boxes in annotation order, a box's points in point order, a point inside two boxes in both -- with
 * xy = float32((double)xy - (double)box xy) (:219-227) and the other columns copied; src_index (cap) = row in `points` of every output
 * row.  totals[3] = {kept boxes, output rows, flags}: flags bit 0 = the rows do not fit cap (nothing is written behind cap; counts,
 * starts and totals[1] are complete, so the caller can size and repeat), bit 1 = a frame broke a limit (below) and was skipped.
 * Limits: at most V3D_DATABASE_MAX_BOXES boxes per frame (V3D_EUNSUPPORTED where n_boxes shows it, flags bit 1 otherwise: the
 * per-frame counts are device data), n_points + 2048 n_frames < 2^31, any n_frames that fits `work`.  Deterministic: no workgroup
 * waits on another, no atomic decides a row.  work must be 4-byte aligned; C == 4 with 16-byte aligned points / out_points reads
 * and writes whole rows. */
#define V3D_DATABASE_MAX_BOXES 256
size_t v3d_database_work_bytes(int n_points, int n_boxes, int n_frames);
int v3d_database_extract(const float* points, int n_points, int C, const int32_t* point_offsets, const double* box_prep, int n_boxes,
                         const int32_t* box_offsets, int n_frames, int min_pts, int32_t* counts, int32_t* starts, int32_t* src_index,
                         float* out_points, int64_t cap, int32_t* totals, void* work, size_t work_bytes, v3d_stream_t stream);

/* ---- A11: points in cuboids / rectangles.
 * Replaces core/geometry.py:27-65 (PointsInCuboids._get_mask when use_z != 0,
 * PointsNotInRectangles._get_mask otherwise).  points (N,C>=3) f32, boxes (n,7) f32
 * (x,y,z,w,l,h,yaw_rad); mask (N,n) u8. */
int v3d_points_in_boxes(const float* points, int N, int C, const float* boxes, int n, int use_z, uint8_t* mask,
                        v3d_stream_t stream);

/* ---- T1 (+A5, A6): voxelizer fused with the VoxelFeatureExtractor mean.
 * Replaces spconv.utils.VoxelGenerator.generate as driven by core/preprocess.py:17-33 (per-frame
 * voxelisation, batch index prefixed, frames concatenated) and detector/layers.py:10-17.
 * points (n_points,C) f32 = the frames concatenated; frame_offsets_host (B+1) i32 on the HOST.
 * voxel_size_host[3] (x,y,z), bounds_host[6] (x0,y0,z0,x1,y1,z1).
 * Outputs sized for B*max_voxels rows: voxels (.,max_pts,C) f32 zero padded [may be NULL],
 * coords (.,4) i32 = (b,z,y,x), occupancy (.) i32, mean (.,C) f32 [may be NULL]; *n_voxels (device i32).
 * Order: frame-major, first-touch order of the input points within a frame; the first max_pts points
 * of a voxel (in input order) are kept -- identical to the sequential reference loop.
 * max_pts <= 8 keeps a voxel's points in registers; 9 <= max_pts <= 64 (pillars) takes a wide path of two more launches (a
 * thread per point ranks it inside its voxel; the mean is summed from the slots) that needs `voxels` (else V3D_EUNSUPPORTED)
 * and zero-fills min(n_points, B*max_voxels) rows of it. */
size_t v3d_voxelize_workspace(int n_points);
int v3d_voxelize(const float* points, int n_points, int C, const int32_t* frame_offsets_host, int B,
                 const float* voxel_size_host, const float* bounds_host, int max_pts, int max_voxels, float* voxels,
                 int32_t* coords, int32_t* occupancy, float* mean, int32_t* n_voxels, void* workspace,
                 size_t workspace_bytes, v3d_stream_t stream);

/* ---- T1d: dynamic voxelization -- no per-voxel point cap (MVF, arXiv 1910.06528).
 * Replaces nothing in the reference (which has only the hard form above); the interface is that of mmdet3d's DynamicScatter /
 * OpenPCDet's DynamicVFE with mean reduction: every in-range point counts, there is no (M, max_pts, C) slot tensor.
 * Inputs as v3d_voxelize.  Outputs sized for min(n_points, B*max_voxels) rows: coords (.,4) i32 = (b,z,y,x), occupancy (.) i32,
 * mean (.,C) f32; point_voxel (n_points) i32 [may be NULL]; n_out[2] (device i32) = {n_voxels, status}.
 * Cells, order: a point belongs to a cell by the statements of the hard voxelizer (IEEE fp32 floorf((q - lo) / vs) and its bounds
 *   test; a NaN coordinate drops the point); rows are frame-major in first-touch order, max_voxels per frame by the same
 *   "continue" rule: coords, the row order and n_voxels are bit for bit those of v3d_voxelize on the same input.
 * occupancy[v] = the TRUE number of points in the cell.  point_voxel[i] = the row of point i, -1 when it is out of bounds or its
 *   voxel was cut by max_voxels.
 * Mean, independent of any order by construction (S = 24):
 *   q_ic      = rint(double(v_ic) * 2^S)                          exact product, round half to even, int64
 *   mean[v,c] = float(double(sum_i q_ic) / (double(k) * 2^S))     the int64 sum is exact; int64 -> double, the double division and
 *                                                                 double -> float each round to nearest even
 *   At most 2^-25 + ulp_fp32(mean) / 2 from the true mean of the fp32 inputs.
 * Range: |v| < 2^16 in every channel and n_points <= 2^22 (no sum can leave int64); V3D_EUNSUPPORTED before any launch beyond
 *   that, also when the largest |bounds_host| is >= 2^16.  A kept point whose channel value is not finite or not below 2^16 in
 *   magnitude contributes nothing to that sum: the voxel's mean in that channel is NaN and bit 0 of status is set.
 * No host read anywhere. */
size_t v3d_voxelize_dynamic_workspace(int n_points);
int v3d_voxelize_dynamic(const float* points, int n_points, int C, const int32_t* frame_offsets_host, int B,
                         const float* voxel_size_host, const float* bounds_host, int max_voxels, int32_t* coords,
                         int32_t* occupancy, float* mean, int32_t* point_voxel, int32_t* n_out, void* workspace,
                         size_t workspace_bytes, v3d_stream_t stream);
/* How the int64 sums are formed (same results bit for bit; profiles/dynamic_voxelize.txt): 0 = a thread per point adds into its
 * voxel's accumulators with 64-bit integer atomics, 1 = a voxel's first point walks the voxel's point list, 2 (default) = the
 * walk for voxels of at most 32 points and the atomics for larger ones.  Sets the choice for the calls that follow in this
 * process (measurements, tests) and returns the previous one; any other value only reads it. */
int v3d_voxelize_dynamic_variant(int variant);

/* ---- T3: sparse-convolution rulebooks (spconv ops.get_indice_pairs, reached through
 * spconv.SubMConv3d / SparseConv3d at detector/sparse_cnn.py:15-30,153-175).
 * coords (cap,4) i32 (b,z,y,x); *n (device i32) active rows.  The rulebook is an output-stationary
 * neighbour table nbr (K, cap_out) i32, k-major: nbr[k*cap_out + o] = input row feeding output row o
 * through kernel offset k (k = (kz*ky_n + ky)*kx_n + kx), or -1.
 *   subm:   output sites == input sites (cap_out == cap).
 *   sparse: out sites = { (i + pad - k)/stride integral, in range }, numbered in first-touch order of
 *           the ticket sequence t = i*K + k; coords_out (cap_out,4), *n_out (device i32, clipped to
 *           cap_out; bit 0 of *overflow is set when clipped). */
size_t v3d_rulebook_workspace(int cap_in, int cap_out, int K);
int v3d_rulebook_subm(const int32_t* coords, const int32_t* n, int cap, const int32_t* spatial_shape_host,
                      const int32_t* ksize_host, int32_t* nbr, void* workspace, size_t workspace_bytes,
                      v3d_stream_t stream);
int v3d_rulebook_sparse(const int32_t* coords_in, const int32_t* n_in, int cap_in,
                        const int32_t* spatial_shape_host, const int32_t* ksize_host, const int32_t* stride_host,
                        const int32_t* padding_host, int32_t* coords_out, int32_t* n_out, int cap_out, int32_t* nbr,
                        int32_t* overflow, void* workspace, size_t workspace_bytes, v3d_stream_t stream);

/* ---- T3: sparse convolution forward (spconv ops.indice_conv) with optional fused per-channel affine
 * (BatchNorm1d in eval mode folded to scale/shift, sparse_cnn.py:18,27) and ReLU.
 * in (>=n_in,Cin) f32, weight (K,Cin,Cout) f32 [= spconv's (k0,k1,k2,Cin,Cout)], out (cap_out,Cout).
 * out[o,:] = act( (sum_k in[nbr[k,o],:] @ weight[k]) * scale + shift ).  Deterministic (no atomics).
 * algo: 0 = auto, 1 = scalar reference kernel, 3 = wave-autonomous exact-fp32 MFMA kernel (needs Cin%4==0, Cout%16==0 and a
 * compiled (Cin,Cout) instance). */
int v3d_sparse_conv_fwd(const float* in, const float* weight, const int32_t* nbr, const int32_t* n_out, int cap_out,
                        int K, int Cin, int Cout, const float* scale, const float* shift, int relu, float* out,
                        int algo, v3d_stream_t stream);

/* Split-precision variant (algo 4): operands are split into 16-bit hi + lo pieces (weights once per layer into a packed image,
 * activations in registers) and multiplied as lo*hi + hi*lo + hi*hi on the 16-bit matrix pipe with fp32 accumulation; one wave owns
 * 16 output rows with register accumulators.  Cout % 16 == 0.  Two arithmetics (`prec`):
 *   V3D_PREC_BF16X3 (0)  bf16 pieces, 2^-17 per product, scale-free (any fp32 magnitude).  What the un-suffixed entry points run.
 *   V3D_PREC_F16S   (1)  f16 pieces of x * s under a power-of-two scale s per tensor, 2^-22 per product: the result differs from
 *                        the reference's fp32 modules (detector/sparse_cnn.py:15-30 run spconv's fp32 GEMMs) by fp32's own
 *                        summation noise, at the same three MFMAs.  The weight scale is chosen by the pack call (device-side,
 *                        from max|W|); the activation scale is the caller's: `act_in` / `act_next` point at device entries
 *                        {s, 1/s, limit, 0} of the gathered tensor and (nullable) of the output -- an output magnitude beyond
 *                        `limit` = 2^15 / s raises *range_flag to 2 (atomicMax; nullable): the caller recalibrates and re-runs.
 *                        v3d_act_scale_from_rows fills an entry from the rows themselves (exact maximum: no flag needed). */
#define V3D_PREC_BF16X3 0
#define V3D_PREC_F16S 1
size_t v3d_sparse_conv_weight_image_bytes(int K, int Cin, int Cout);
/* image of `prec` (V3D_PREC_*) for the packed kernels: weight (K, Cin, Cout) fp32 -> split 16-bit fragments in MFMA order */
int v3d_sparse_conv_pack_weights(const float* weight, int K, int Cin, int Cout, int prec, void* image, v3d_stream_t stream);
/* entry[0..3] = {s, 1/s, 2^15 / s, max} for the n = min(*n_rows, cap) rows of `rows` (cap, C) [n_rows NULL: all cap rows]:
 * s = the power of two that puts the largest magnitude into [2^(13 - headroom_bits), 2^(14 - headroom_bits)).  No host
 * synchronisation.  headroom_bits in [0, 12].  scratch NULL: one workgroup.  scratch != NULL: a grid of workgroups -- two uint32
 * words in device memory that are ZERO when the launch starts (running maximum, arrival ticket); the last workgroup to arrive
 * writes the entry and zeroes them again, so one zeroed scratch serves every later call on the same stream. */
int v3d_act_scale_from_rows(const float* rows, const int32_t* n_rows, int cap, int C, int headroom_bits, float* entry,
                            uint32_t* scratch, v3d_stream_t stream);
/* rows_hint > 0: the caller's estimate of the LIVE row count (*n_out is device-side), used only to choose the kernel: 3x3x3 with
 * Cin, Cout in {32, 64}: LDS-ring kernel up to 16 384 rows, 64-row LDS-shared-weights kernel from 32 768, else the 16-row kernel;
 * 0 = unknown (ring / 16-row).  The 64 -> 64 ring kernel owns a CU per workgroup: it takes 2, 3 or 4 sixteen-row tiles per workgroup,
 * the smallest count that keeps rows_hint + 10 % inside one round of 256 workgroups (8 192 / 12 288 / 16 384 rows).
 * rows_hint < 0 FORCES a kernel (tests, benchmarks): -1 = 16-row, -5 = 64-row, -6 / -7 = offset-outer (staged / register gathers),
 * -10 = LDS ring, -16 = its register-gather form, -12 / -13 / -14 = the 64 -> 64 ring with 2 / 3 / 4 tiles per workgroup.
 * There is no process-global switch.
 * prec = the arithmetic the image was packed for; V3D_PREC_F16S needs act_in (and act_next where split rows are written); act_in /
 * act_next / range_flag are ignored (may be NULL) for V3D_PREC_BF16X3.
 * in_split / out_split (both nullable): rows ALREADY split into the arithmetic's 16-bit pieces -- a row = [hi: C x 16 bit |
 * lo: C x 16 bit], the bytes of the fp32 row; f16s: pieces of x * s of the tensor's scale entry.  in_split (then `in` may be NULL):
 * the layer gathers these and its main loop converts nothing; out_split (Cout % 8 == 0; f16s needs act_next; `out` may then be NULL):
 * the output rows once more in that form, for the next layer's in_split.  A chain of layers this way computes the same bits as
 * on fp32 rows (v3d_sparse_rows_split makes split rows from fp32 rows). */
int v3d_sparse_conv_fwd_packed(const float* in, const void* weight_image, const int32_t* nbr, const int32_t* n_out,
                               int cap_out, int K, int Cin, int Cout, const float* scale, const float* shift, int relu,
                               float* out, int rows_hint, int prec, const float* act_in, const float* act_next,
                               int32_t* range_flag, const void* in_split, void* out_split, v3d_stream_t stream);
int v3d_sparse_rows_split(const float* rows, const int32_t* n_rows, int cap, int C, int prec, const float* act_entry,
                          void* out_split, v3d_stream_t stream);
/* 1 where the MFMA kernels (v3d_sparse_conv_fwd_packed, and algo 0 / 3 of v3d_sparse_conv_fwd) exist for Cin -> Cout, 0 where only
 * the scalar kernel (algo 1) runs the layer.  The data gradient asks it for the SWAPPED pair (Cout -> Cin) before it picks a kernel. */
int v3d_sparse_conv_packed_supported(int Cin, int Cout);
/* ---- T3 over SPATIALLY ORDERED rows (csrc/brick.hip; same interface the reference reaches through spconv.SubMConv3d,
 * detector/sparse_cnn.py:15-30).  When the rows of a stage are numbered in a spatial (brick / Morton) order, the 27 x 256
 * neighbours of 256 consecutive rows are ~1.2-1.7 x 256 distinct rows: v3d_sparse_brick_plan derives, once per submanifold
 * table `nbr` (K = 27), per 256-row pass the list of those rows (`ulist`, 480 per pass; `ucnt` their number), every table entry
 * as a slot of its pass's list (`lidx`, 0xFFFF = no neighbour) and per 16-row tile the mask of offsets any of its rows has
 * (`tmask`); v3d_sparse_conv_fwd_brick (Cin -> Cout = 64 -> 64, 32 -> 32; split rows in, rows and / or split rows out) keeps a pass's
 * rows in LDS and walks the offsets without any global gather.  Correct for ANY row order (a pass with more than 480 distinct
 * neighbours gathers directly); same bits as v3d_sparse_conv_fwd_packed2 with rows_hint = -6.
 * v3d_sparse_brick_table_bytes: byte sizes of the four tables for a capacity (each a multiple of 256), returns their sum. */
size_t v3d_sparse_brick_table_bytes(int cap, int K, size_t* lidx_bytes, size_t* ulist_bytes, size_t* ucnt_bytes,
                                    size_t* tmask_bytes);
int v3d_sparse_brick_plan(const int32_t* nbr, const int32_t* n_rows, int cap, int K, uint16_t* lidx, int32_t* ulist,
                          int32_t* ucnt, uint32_t* tmask, v3d_stream_t stream);
int v3d_sparse_conv_fwd_brick(const void* in_split, const void* weight_image, const int32_t* nbr, const uint16_t* lidx,
                              const int32_t* ulist, const int32_t* ucnt, const uint32_t* tmask, const int32_t* n_out,
                              int cap, int K, int Cin, int Cout, const float* scale, const float* shift, int relu, float* out,
                              int prec, const float* act_in, const float* act_next, int32_t* range_flag, void* out_split,
                              v3d_stream_t stream);

/* ---- T3 backward (spconv indice_conv backward; the reference trains through it at train.py:65).
 * Data gradient: dX[i] = sum_k dY[nbrT[k][i]] @ W[k]^T -- the forward entry points above on the TRANSPOSED
 * rulebook (v3d_rulebook_transpose; a submanifold table is its own transpose with the offsets reversed) and the
 * transposed weights.  Weight gradient: dW[k] = sum_{pairs} X[i]^T dY[o], exact-fp32 MFMA, deterministic. */
int v3d_rulebook_transpose(const int32_t* nbr, const int32_t* n_out, int cap_out, int K, int cap_in, int32_t* nbr_t,
                           v3d_stream_t stream);
size_t v3d_sparse_conv_bwd_weight_workspace(int K, int Cin, int Cout);
int v3d_sparse_conv_bwd_weight(const float* X, const float* dY, const int32_t* nbr, const int32_t* n_out, int cap_out,
                               int K, int Cin, int Cout, float* dW, void* workspace, size_t workspace_bytes,
                               v3d_stream_t stream);

/* ---- T2: SparseConvTensor.dense() (detector/sparse_cnn.py:128-133): zero-fill + scatter.
 * feat (cap,C), coords (cap,4), *n rows -> dense (B,C,D,H,W) f32. */
int v3d_densify(const float* feat, const int32_t* coords, const int32_t* n, int cap, int B, int C,
                const int32_t* spatial_shape_host, float* dense, v3d_stream_t stream);

/* ---- T4/T5: pointnet2 ops (pointnet2_utils.furthest_point_sample / gather_operation / ball_query /
 * grouping_operation; call sites detector/model.py:46-66, detector/roi_grid_pool.py:64-72). */
size_t v3d_fps_workspace(int B, int N);
int v3d_furthest_point_sample(const float* xyz, int B, int N, int K, int32_t* idx, void* workspace,
                              size_t workspace_bytes, v3d_stream_t stream);
/* Sectorized proposal-centric keypoint sampling (csrc/keypoints.hip; definition: vision3d_amd/pointnet2/pointnet2_utils.py).  Per frame
 * the finite points within 0.5 max(w, l, h) + radius of some proposal (x, y, z, w, l, h, yaw) -- all finite points if that leaves none,
 * or with proposals == NULL / P == 0 -- are split into S azimuth sectors; sector k gets a quota proportional to its size and an
 * independent farthest-point chain (first pick = lowest index, ties -> lowest index); idx (B, K) = the sectors' picks in sector
 * order, short frames padded by idx[i] = idx[i mod filled].  points: B frames of N rows of `point_stride` >= 3 floats (x, y, z first).
 * sector_counts (B, S), optional: candidates per sector.  Five launches, no host read, capturable; any N (a sector of up to
 * 24 576 points keeps its chain in registers -- what 1 024 lanes x 128 VGPRs hold without a spill --, a larger one streams its
 * running distances through the workspace: same indices, slower steps).  workspace: 16-byte aligned scratch of v3d_keypoints_sector_workspace bytes.
 * V3D_EINVAL: S outside 1-64, P > 1024, K < 1, N < 1, point_stride < 3, short workspace. */
size_t v3d_keypoints_sector_workspace(int B, int N, int S);
int v3d_keypoints_sector(const float* points, int point_stride, int B, int N, int K, int S, const float* proposals, int P, float radius,
                         int32_t* idx, int32_t* sector_counts, void* workspace, size_t workspace_bytes, v3d_stream_t stream);
int v3d_gather_points(const float* feat, const int32_t* idx, int B, int C, int N, int K, float* out,
                      v3d_stream_t stream);
/* idx_b == NULL: one radius (radius_b / nsample_b ignored).  idx_b != NULL: two radii around the same queries in ONE scan of the
 * database (what PointnetSAModuleMSG asks for per feature source): per (query, radius) the same result as the one-radius call. */
int v3d_ball_query(const float* xyz, const float* new_xyz, int B, int N, int M, float radius_a, int nsample_a, int32_t* idx_a,
                   float radius_b, int nsample_b, int32_t* idx_b, v3d_stream_t stream);
/* The same operation through a cell grid of the database: the points are binned into (x, y) cells no smaller than the larger radius
 * (one launch), every query looks at the 3 x 3 cells around its own and reads "the first nsample hits in index order" off a
 * per-wave LDS bitmap (second launch).  Same arguments, same results as v3d_ball_query for every input (the hit test is the scan
 * kernel's expression on the same operands); ~6x faster at PV-RCNN's sizes whatever the order of the cloud.  `workspace`:
 * v3d_ball_query_grid_workspace(B, N) bytes, 16-byte aligned, scratch. */
size_t v3d_ball_query_grid_workspace(int B, int N);
int v3d_ball_query_grid(const float* xyz, const float* new_xyz, int B, int N, int M, float radius_a, int nsample_a, int32_t* idx_a,
                        float radius_b, int nsample_b, int32_t* idx_b, void* workspace, size_t workspace_bytes, v3d_stream_t stream);
/* The two halves on their own.  build: the grids of up to 8 databases in ONE launch (a workgroup per database and frame; host arrays
 * of n_db entries: xyz[i] (B, N[i], 3), radius_max[i] = the largest radius that will be asked of grid i, workspace[i] of
 * v3d_ball_query_grid_workspace(B, N[i]) bytes) -- the six databases of a PV-RCNN frame (raw points, four voxel levels, keypoints:
 * detector/model.py:58-66, roi_grid_pool.py:64-72) cost one launch instead of six.  query: any radii <= radius_max of the build,
 * as often as wanted; same results as v3d_ball_query.  V3D_EUNSUPPORTED: N too large for the query's LDS bitmaps (use the scan). */
int v3d_ball_query_grid_build(int n_db, const float* const* xyz, const int32_t* N, const float* radius_max, void* const* workspace,
                              const size_t* workspace_bytes, int B, v3d_stream_t stream);
int v3d_ball_query_grid_query(const float* new_xyz, int B, int N, int M, float radius_a, int nsample_a, int32_t* idx_a,
                              float radius_b, int nsample_b, int32_t* idx_b, const void* workspace, size_t workspace_bytes,
                              v3d_stream_t stream);
/* query_many: up to 8 queries around the SAME new_xyz (B, M, 3), each in its own database / grid with its own radii, in one launch
 * (host arrays of n_jobs entries; idx_b[i] NULL: one radius for job i) -- the five set-abstraction modules of a PV-RCNN frame all
 * ask around the frame's keypoints (detector/model.py:58-66). */
int v3d_ball_query_grid_query_many(int n_jobs, const float* new_xyz, int B, int M, const int32_t* N, const float* radius_a,
                                   const int32_t* nsample_a, int32_t* const* idx_a, const float* radius_b, const int32_t* nsample_b,
                                   int32_t* const* idx_b, const void* const* workspace, const size_t* workspace_bytes,
                                   v3d_stream_t stream);
int v3d_group_points(const float* feat, const int32_t* idx, int B, int C, int N, int M, int nsample, float* out,
                     v3d_stream_t stream);
/* Bilinear lookup of BEV features at keypoints: F.grid_sample(feature_map, grid, bilinear, zeros, align_corners=True) for a
 * (B, 1, K, 2) grid, as BEVFeatureGatherer.forward calls it (detector/layers.py:29-47).  feature_map (B, C, H, W) f32, grid
 * (B, K, 2) f32 = (x, y) in [-1, 1], out (B, C, K).  Same taps, weights and summation order as torch's kernel. */
int v3d_bev_bilinear(const float* feature_map, const float* grid, int B, int C, int H, int W, int K, float* out,
                     v3d_stream_t stream);
/* BEVFeatureGatherer.forward in one launch (detector/layers.py:29-47): grid coordinates from the keypoints by the module's own fp32
 * statements (offset / pixel = its pixel_offset and base_pixel_size * STRIDES[-1], x and y), clamp, normalise, flip, then the
 * bilinear lookup above.  keypoint_xyz (B, K, 3); out is POINT-major: out[(b * K + k) * ldo + c], ldo >= C.  Same values as
 * v3d_bev_bilinear on the module's torch-computed grid, bit for bit. */
int v3d_bev_gather_keypoints(const float* feature_map, const float* keypoint_xyz, int B, int C, int H, int W, int K, float offset_x,
                             float offset_y, float pixel_x, float pixel_y, float* out, int ldo, v3d_stream_t stream);

/* SparseCNNBase.to_global in one launch (detector/sparse_cnn.py:91-105): out (n, 3) = (x, y, z) = float(indices[:, (3, 2, 1)]) *
 * scale + offset, one conversion, one multiply and one add per coordinate; indices (n, 4) i32 = (b, z, y, x), 16-byte aligned;
 * scale = base_voxel_size * stride as the caller rounded it in fp32. */
int v3d_voxel_centers(const int32_t* indices, int n, float scale_x, float scale_y, float scale_z, float offset_x, float offset_y,
                      float offset_z, float* out, v3d_stream_t stream);
/* RoiGridPool.sample_gridpoints in one launch (detector/roi_grid_pool.py:52-62): points[b, n, j] = centre + Rz(yaw) (size * (sample - 0.5))
 * with the module's own fp32 statements, one IEEE operation each; boxes (B*n, 7) = x, y, z, w, l, h, yaw, samples (B*n, m, 3) in
 * [0, 1), cos_yaw / sin_yaw (B*n) from the caller (torch's cos / sin: the same values as the op-by-op path) or both NULL (cosf / sinf
 * of the device library inside the launch: equal to torch's on this stack, which the GPU tests check), out (B*n, m, 3). */
int v3d_roi_grid_points(const float* boxes, const float* samples, const float* cos_yaw, const float* sin_yaw, int n_boxes, int m,
                        float* out, v3d_stream_t stream);

/* ---- T5: one layer of a set-abstraction shared MLP on gathered rows, exact fp32 on the matrix cores (csrc/sa_mlp.hip).
 * Replaces, per scale of pointnet2_modules.PointnetSAModuleMSG (call sites detector/model.py:58-66, detector/roi_grid_pool.py:
 * 64-72), grouping_operation + SharedMLP (Conv2d 1x1, no bias + BatchNorm2d + ReLU per layer) + max over the samples, without the
 * grouped (B, C+3, M, ns) tensor.  Rows are (b, m, s) in that order, rows = B*M*ns.
 *   first layer  (idx != NULL): feat (B, N, Kf) POINT-major, xyz (B, N, 3), new_xyz (B, M, 3), idx (B, M, ns) i32 into N;
 *                row = [xyz[i] - new_xyz[m], 0 | feat[i, :]], W (4 + Kf, Nout) row-major (row 3 multiplies the zero);
 *   later layers (idx == NULL, xyz == new_xyz == NULL): feat (rows, Kf) = the previous layer's output, N must equal M*ns, W (Kf, Nout).
 * out[row, :] = act(row @ W + bias); pool != 0: out (B*M, Nout) = max over the ns rows of each (b, m) (ns = 16 or 32).
 * Kf % 4 == 0, Nout in {16, 32, 64, 96, 128, 192, 256}; BatchNorm(eval) is folded into W / bias by the caller.
 * ldo = row stride of `out` in floats (0: Nout), n_store = columns stored (0: Nout): a scale's pooled rows land directly in their
 * column block of the (B*M, C_total) keypoint feature matrix -- no torch.cat of the scales / sources (model.py:72-74). */
int v3d_sa_mlp_layer(const float* feat, const float* xyz, const float* new_xyz, const int32_t* idx, int B, int N, int M, int ns,
                     int Kf, const float* W, const float* bias, int Nout, int relu, int pool, float* out, int ldo, int n_store,
                     v3d_stream_t stream);
/* The first TWO layers of a scale in one launch.  The first layer is linear in [xyz[i] - new_xyz[m], 0 | feat[i]] and its feature
 * part depends on the gathered point alone: the caller computes P (B, N, K1) = feat @ W1[4:] once per DATABASE point
 * (v3d_linear_rows; N rows instead of M * ns), and this kernel rebuilds relu(P[i] + rel . W1[0:3] + b1) as the operand rows of the
 * second layer W (K1, Nout) -- 37x less matrix work at RoI-grid pooling (2 048 keypoints, 76 800 grouped rows, roi_grid_pool.py:64-72),
 * and the (rows, K1) intermediate is never written.  wx (3, K1) = W1[0:3], b1 (K1); K1 % 4 == 0, K1 <= 256; ldp = row stride of P in
 * floats (0: K1; the two scales of a module share one product with concatenated weights); the rest as above. */
int v3d_sa_mlp_pair(const float* P, const float* xyz, const float* new_xyz, const int32_t* idx, int B, int N, int M, int ns, int K1,
                    int ldp, const float* wx, const float* b1, const float* W, const float* bias, int Nout, int relu, int pool,
                    float* out, int ldo, int n_store, v3d_stream_t stream);
/* v3d_sa_mlp_pair for the two scales of a module in ONE launch (same K1 and Nout; per scale: its column block of P, neighbour list,
 * sample count, wx / b1, W / bias and the column block of `out` it writes): fills the chip where two launches left it half empty. */
int v3d_sa_mlp_pair2(const float* P_a, const float* P_b, const float* xyz, const float* new_xyz, const int32_t* idx_a, const int32_t* idx_b,
                     int B, int N, int M, int ns_a, int ns_b, int K1, int ldp, const float* wx_a, const float* b1_a, const float* wx_b,
                     const float* b1_b, const float* W_a, const float* bias_a, const float* W_b, const float* bias_b, int Nout, int relu,
                     int pool, float* out_a, float* out_b, int ldo, int n_store, v3d_stream_t stream);
/* The MLP tail of PV-RCNN on a hundred rows: out[r, n] = act(sum_k A[r * lda + k] * W[k * Nout + n] + bias[n]) for r < R,
 * n < n_store (0: Nout), out row stride ldo (0: Nout).  Replaces nn.Linear (+ bias, + ReLU) of detector/layers.py:53-73 as used by
 * the RoI-grid reduction (roi_grid_pool.py:64-72: 3 072 -> 256 -> 256) and the refinement head (refinement.py:47-50: 256 -> 128 -> 8).
 * W is the Linear's weight TRANSPOSED (K, Nout), Nout padded to a multiple of 16 by the caller, K % 4 == 0, A 16-byte aligned.
 * Exact fp32 products on the matrix cores, fixed summation order (K split over 8 waves, partial tiles added in wave order). */
int v3d_linear_rows(const float* A, int lda, int R, int K, const float* W, const float* bias, int Nout, int relu, float* out, int ldo,
                    int n_store, v3d_stream_t stream);
/* up to 8 such products in one launch (host arrays of n_jobs entries; bias / relu / ldo / n_store arrays may be NULL = none / 0). */
int v3d_linear_rows_many(int n_jobs, const float* const* A, const int32_t* lda, const int32_t* R, const int32_t* K, const float* const* W,
                         const float* const* bias, const int32_t* Nout, const int32_t* relu, float* const* out, const int32_t* ldo,
                         const int32_t* n_store, v3d_stream_t stream);

/* ---- Fused sparse-backbone plan: voxelizer -> [rulebooks + sparse conv layers] -> .dense().
 * The native form of the sparse half of Second.feature_extract (detector/second.py:20-24,41-46 over
 * detector/sparse_cnn.py:151-175): created once per model, every forward only ENQUEUES kernels on
 * `stream` -- no host synchronisation, counts stay in device memory, one coordinate hash per stage is
 * shared by the strided rulebook that creates the stage and the submanifold rulebook that follows.
 * The plan owns its arena (hipMalloc at create, hipFree at destroy) and private copies of the layer
 * parameters (set_layer copies device -> device).  Not thread-safe per plan; use one plan per stream. */
typedef struct v3d_backbone v3d_backbone;
typedef struct {
  int32_t subm;                            /* 1 = SubMConv3d, 0 = SparseConv3d */
  int32_t cin, cout;
  int32_t ksize[3], stride[3], padding[3]; /* z, y, x */
  int32_t key;                             /* >= 0: submanifold layers with equal key share a rulebook (indice_key) */
  int32_t relu;                            /* fused ReLU */
} v3d_layer_desc;
typedef struct {
  float voxel_size[3];                     /* x, y, z */
  float bounds[6];                         /* x0,y0,z0,x1,y1,z1 */
  int32_t max_pts, max_voxels;             /* per voxel / per frame; max_pts = 0: dynamic voxelization (v3d_voxelize_dynamic) */
  int32_t point_channels;                  /* C of the input points == Cin of layer 0 */
  int32_t grid_shape[3];                   /* D,H,W of the CNN input grid (sparse_cnn.py:40-45: z + 1) */
  int32_t max_batch, max_points;           /* capacities: frames per forward, total points per forward */
  int32_t n_layers;
  float growth;                            /* active-site capacity of later stages = growth * voxel capacity (<=0: 2.0) */
  int32_t conv_algo;                       /* 0 = default; 3 = fp32-MFMA wave kernel; 4 = bf16x3 row-owner kernel */
} v3d_backbone_config;
int v3d_backbone_create(const v3d_backbone_config* cfg, const v3d_layer_desc* layers, v3d_backbone** out);
void v3d_backbone_destroy(v3d_backbone* plan);
size_t v3d_backbone_arena_bytes(const v3d_backbone* plan);
int v3d_backbone_num_layers(const v3d_backbone* plan);
/* weight (K,Cin,Cout) f32; scale/shift (Cout) or both NULL (no affine). */
int v3d_backbone_set_layer(v3d_backbone* plan, int layer, const float* weight, const float* scale, const float* shift,
                           v3d_stream_t stream);
/* points (n_points,C) f32 = frames concatenated.  Outputs, any may be NULL: dense_nchw (B, Cout_last*D, H, W) f32 and / or the
 * split planes dense_hi / dense_lo ((B, H, W, Cout_last*D) 16-bit pieces of the plan's arithmetic: the dense head's input). */
int v3d_backbone_forward(v3d_backbone* plan, const float* points, int n_points, const int32_t* frame_offsets_host,
                         int B, float* dense_nchw, void* dense_hi, void* dense_lo, v3d_stream_t stream);
/* Device-resident results of the last forward: layer = -1 -> voxelizer output (mean features, coords);
 * layer >= 0 -> that layer's output rows.  *n_rows_dev is a device int32; cap = row capacity. */
int v3d_backbone_layer_output(v3d_backbone* plan, int layer, float** features, int32_t** coords,
                              int32_t** n_rows_dev, int* cap, int* channels, int32_t* shape_host);
/* Kernel-choice tuning from observed sparsity: reads the live row counts of the last forward (blocking, a few bytes)
 * and uses them as size hints for the following forwards (capacities are upper bounds).  Not capturable. */
int v3d_backbone_tune(v3d_backbone* plan);
int32_t* v3d_backbone_occupancy(v3d_backbone* plan);       /* (cap0) i32, voxel occupancies of the last forward */
int32_t* v3d_backbone_voxel_status(v3d_backbone* plan);    /* (1) i32 device status word of the last forward's dynamic voxelization
                                                              (v3d_voxelize_dynamic; stays 0 with max_pts > 0) */
int32_t* v3d_backbone_overflow_flags(v3d_backbone* plan);  /* (n_layers+1) i32 device flags of the last forward: [l] > 0 = layer l
                                                              hit its active-site capacity (rows were dropped), [n_layers] > 0 = any */

/* ---- A8/A9: dense 2-D convolutions of the BEV head on the matrix cores (csrc/dense_conv.hip).
 * Replaces nn.Conv2d + BatchNorm2d(eval) + ReLU (detector/second.py:58-94) and the 1x1 heads
 * (detector/proposal.py:19-22).  "bf16 x 3" split precision: x = hi + lo (two bf16), products evaluated as
 * hi*hi + hi*lo + lo*hi with fp32 accumulation => fp32-class accuracy.  Activations are exchanged as two
 * bf16 NHWC planes (B,H,W,C) "hi" and "lo"; weights are packed once with v3d_conv2d_pack_weights.
 * Cin % 32 == 0, ksize in {1,3} (stride 1, "same" zero padding).  Outputs: split NHWC planes (Cout % 8 == 0)
 * and/or fp32 NCHW (B,Cout,H,W). */
size_t v3d_conv2d_weight_image_bytes(int Cin, int Cout, int ksize);
/* (v3d_conv2d_pack_weights: weight (Cout,Cin,k,k) f32; optional per-output-channel scale (folded BatchNorm) multiplied in;
 *  v3d_conv2d_nhwc_split: the convolution -- both declared below, with the arithmetic's scale entries) */
/* Background skipping for the BEV head.  The BEV map of a sparse scene is mostly empty: an output pixel of layer L whose
 * receptive field through layers 1..L (`reach` pixels: +1 per 3x3 layer) contains no occupied BEV pixel sees exactly the inputs it
 * sees in an EMPTY map, so its value is the empty map's response at that position -- bit for bit, borders included.  The caller
 * computes that response once per weight set (the same convolutions on an all-zero map, occ = NULL) and passes it as bg_hi / bg_lo
 * ((H, W, Cout) split planes of ONE image); tiles whose pixels are all further than `reach` (Chebyshev) from every occupied pixel
 * become a copy of that response instead of a convolution.  Results are identical
 * to the call with occ = NULL.  Applies to the large-tile kernel with split-plane output;
 * any other configuration computes every pixel.
 * occ: BEV occupancy, one bit per pixel, INVERTED (bit cleared = occupied; a 0xFF fill = empty map), rows (b, y) of ceil(W / 32)
 * words.  A plan keeps one for its last forward (v3d_backbone_bev_occupancy: cleared by the per-frame 0xFF fill, set by the
 * densify kernel -- no extra launch); v3d_bev_occupancy_bits builds one from a site list. */
size_t v3d_bev_occupancy_words(int B, int H, int W);
int v3d_bev_occupancy_bits(const int32_t* coords /*(cap,4) b,z,y,x*/, const int32_t* n, int cap, int B, int H, int W,
                           uint32_t* occ, v3d_stream_t stream);
uint32_t* v3d_backbone_bev_occupancy(v3d_backbone* plan);
/* The plan's PERSISTENT split BEV planes ((max_batch, H, W, C_out * D) bf16 each, hi then lo, adjacent).  Passing exactly these two
 * pointers as dense_hi / dense_lo to v3d_backbone_forward / _forward_voxels / _forward_reuse makes the plan keep them zero outside
 * the occupied pixels itself: each frame clears the few thousand pixels the previous one wrote (in the launch of its per-frame fill)
 * instead of filling 2 x 9 MB per KITTI frame -- what .dense() (detector/sparse_cnn.py:128-133: zeros + scatter) costs.  Valid until the
 * next forward into them; nobody else may write them. */
int v3d_backbone_bev_planes(v3d_backbone* plan, void** hi, void** lo);
/* Kernel choice of the following forwards: on != 0 = THROUGHPUT mode, for plans whose frames run beside other frames on the same GPU
 * (one plan per frame in flight): the LDS-filling 64 -> 64 sparse kernel takes four 16-row tiles per workgroup whatever the row count --
 * fewer, fatter workgroups: ~39 % less CU-time per launch, ~20 % longer launches (results are bit-identical either way) --, and a
 * packed layer that is followed by a packed layer writes its output rows ONLY in the split form the next layer gathers
 * (v3d_backbone_set_presplit), not as fp32 rows: v3d_backbone_layer_output's feature views of such layers are then stale.
 * Default off: the shortest launch (one frame at a time), every layer's fp32 rows written. */
int v3d_backbone_set_throughput_mode(v3d_backbone* plan, int on);
/* Arithmetic of the plan's INFERENCE entry points (v3d_backbone_forward* ; the training plan is bf16x3): V3D_PREC_BF16X3 (default of
 * a new plan) or V3D_PREC_F16S.  Set it BEFORE v3d_backbone_set_layer: the weight images are packed per arithmetic.
 * f16s: v3d_backbone_act_scales() = (n_layers + 1) x {s, 1/s, limit, max} in device memory, entry l = the rows layer l gathers,
 * entry n_layers = the BEV map (the scale of the split planes).  New plans hold {1, 1, 2^15, 0}: correct for magnitudes below 2^15,
 * full precision once calibrated: v3d_backbone_set_calibrating(plan, 1) -> one forward (every layer on the exact-fp32 kernel) ->
 * v3d_backbone_calibrate(plan, headroom_bits, stream) (entries from that frame's maxima; enqueued, no host sync) ->
 * v3d_backbone_set_calibrating(plan, 0).  A later frame whose tensors exceed an entry's limit (2^(headroom_bits + 1) x the
 * calibration frame's maximum) raises v3d_backbone_overflow_flags()[n_layers] to 2: recalibrate on it and run it again. */
int v3d_backbone_set_precision(v3d_backbone* plan, int prec);
int v3d_backbone_precision(const v3d_backbone* plan);
/* on != 0 (default): a packed layer also writes its output rows split into the arithmetic's 16-bit pieces and the next packed layer
 * gathers those (no conversion work in its main loop); 0: every layer splits the fp32 rows it gathers (A/B).  Same results. */
int v3d_backbone_set_presplit(v3d_backbone* plan, int on);
float* v3d_backbone_act_scales(v3d_backbone* plan);
int v3d_backbone_set_calibrating(v3d_backbone* plan, int on);
int v3d_backbone_calibrate(v3d_backbone* plan, int headroom_bits, v3d_stream_t stream);
/* v3d_conv2d_nhwc_split arguments of the background-skipping path (all nullable / zero = every tile convolved):
 *   occ, reach, bg_hi, bg_lo  inverted BEV occupancy bitmap (v3d_backbone_bev_occupancy), the layer's reach in pixels and its
 *                             response to the empty map (planes): tiles with no occupied pixel within reach ARE that response;
 *   work        two zeroed words owned by the caller for THIS call site (one pair per layer and stream in flight).  With it the
 *               skipping kernel runs as a persistent grid that draws tiles from work[0]; the pair resets itself when the kernel ends;
 *   tile_state  with `work`, when y_hi / y_lo are PERSISTENT buffers of this call site (the same pair every frame):
 *               v3d_conv2d_bg_tiles words, nonzero = the tile holds computed values (initialise to nonzero).  A layer's empty-map
 *               response does not depend on the frame, so a background tile whose word is 0 already holds it and is not written
 *               at all; the kernel keeps the words up to date.  Reset them to nonzero when the weights (bg_hi / bg_lo) change;
 *   reset_ptr, reset_words    the counter pair reset by ANOTHER launch: reset_ptr != NULL makes this launch zero reset_words words
 *               at reset_ptr when it starts (the pairs of call sites whose launches lie behind it in stream order) and leave its
 *               own `work` pair as it ends -- some later launch of the caller's zeroes it (saves the atomic round trip every
 *               workgroup of a self-resetting launch ends on); `work` must read zero at launch;
 *   pr          NULL = bf16x3 images and planes; else the arithmetic and its scale entries (v3d_conv2d_prec below). */
int v3d_conv2d_bg_tiles(int B, int H, int W);
/* ---- the same dense head in fp32-class arithmetic (V3D_PREC_F16S; see the sparse section above for the two arithmetics).
 * The reference's RPN / heads are fp32 nn.Conv2d modules (detector/second.py:58-79, detector/proposal.py:19-22): f16s reproduces
 * them up to fp32 summation noise at the cost of bf16x3.  Planes then hold f16 pieces of x * s: every plane pair has a device entry
 * {s, 1/s, limit = 2^15 / s, ..} (set by the caller's calibration: vision3d_amd.runtime.DenseHeadPlan.calibrate; the BEV planes of
 * a plan use v3d_backbone_act_scales()[n_layers]), the weight image carries its own scale (v3d_conv2d_pack_weights), and an output
 * magnitude beyond its entry's limit raises *range_flag to 2 (atomicMax, nullable).  fp32 NCHW outputs are unscaled.
 * For v3d_conv2d_1x1_head_fused `out_entry` is the entry of the intermediate 128-channel tensor. */
typedef struct v3d_conv2d_prec {
  int32_t prec;           /* V3D_PREC_*: the arithmetic the weight image(s) were packed for */
  const float* in_entry;  /* f16s: device entry of the input planes */
  const float* out_entry; /* f16s: device entry of the output planes (NULL when only fp32 NCHW is written) */
  int32_t* range_flag;    /* f16s, nullable */
  const float* w_inv;     /* f16s, nullable: device copy of the weight image's 1 / s_w (float 1 of its 256-byte trailer) in memory the
                             caller keeps hot, e.g. beside its scale entries; NULL: read from the trailer (a cold line per launch) */
  const float* w_inv2;    /* same for the second image of v3d_conv2d_1x1_head_fused */
} v3d_conv2d_prec;
int v3d_conv2d_pack_weights(const float* weight, const float* scale, int Cout, int Cin, int ksize, int prec, void* image,
                            v3d_stream_t stream);
int v3d_conv2d_nhwc_split(const void* x_hi, const void* x_lo, const void* weight_image, const float* bias, int relu, int B,
                          int H, int W, int Cin, int Cout, int ksize, void* y_hi, void* y_lo, float* y_nchw,
                          const uint32_t* occ, int reach, const void* bg_hi, const void* bg_lo, uint32_t* work,
                          uint32_t* tile_state, uint32_t* reset_ptr, int reset_words, const v3d_conv2d_prec* pr,
                          v3d_stream_t stream);
/* A chain of 3x3 128 -> 128 background-skipping layers under ONE persistent state (work, tile_state and output planes per layer, as
 * above) with a per-frame TILE SCHEDULE: which tiles of a layer are live depends on `occ` and the layer's reach alone, so the FIRST
 * launch of the chain (list NULL, n_build = the launches behind it, <= 8) draws its own tiles as v3d_conv2d_nhwc_split does and, on
 * n_build workgroups more, writes for each later launch k its list build_list[k] (v3d_conv2d_tile_sched_words words: live count,
 * stale count, the live tiles at build_reach[k] in increasing index, the background tiles whose word in build_tile_state[k] -- that
 * layer's tile_state -- is still nonzero).  A LATER launch (list = its own, n_build 0) runs exactly those tiles: no draws, no
 * occupancy test, `work` untouched (reset_ptr / reset_words as above).  Same values as v3d_conv2d_nhwc_split with the same occ / reach.
 * build_reach / build_tile_state / build_list are host arrays.  v3d_conv2d_tile_sched_words returns 0 for a layer that takes no
 * schedule (another shape, or a map of 4 tiles per CU and more): such a chain uses v3d_conv2d_nhwc_split. */
int v3d_conv2d_tile_sched_words(int B, int H, int W, int Cin, int Cout, int ksize);
int v3d_conv2d_nhwc_split_sched(const void* x_hi, const void* x_lo, const void* weight_image, const float* bias, int relu, int B,
                                int H, int W, int Cin, int Cout, int ksize, void* y_hi, void* y_lo, const uint32_t* occ, int reach,
                                const void* bg_hi, const void* bg_lo, uint32_t* work, uint32_t* tile_state, uint32_t* reset_ptr,
                                int reset_words, const v3d_conv2d_prec* pr, const uint32_t* list, int n_build,
                                const int32_t* build_reach, const uint32_t* const* build_tile_state, uint32_t* const* build_list,
                                v3d_stream_t stream);
/* The tail of the SECOND dense head in ONE launch: RPN up-conv 1x1 128 -> 128 (+ folded BatchNorm bias + ReLU, detector/second.py:73-79)
 * followed by the fused [cls | reg] 1x1 head 128 -> Cout2 <= 16 (detector/proposal.py:19-22), split planes (B, H, W, 128) in, fp32
 * NCHW (B, Cout2, H, W) out; w1_image / w2_image from v3d_conv2d_pack_weights(.., ksize 1).  Bit-identical to v3d_conv2d_nhwc_split
 * applied twice; the intermediate planes never exist.  V3D_EUNSUPPORTED for other widths.  pr NULL = bf16x3. */
int v3d_conv2d_1x1_head_fused(const void* x_hi, const void* x_lo, const void* w1_image, const float* b1, int relu1,
                              const void* w2_image, const float* b2, int relu2, int B, int H, int W, int Cmid, int Cout2,
                              float* y_nchw, const v3d_conv2d_prec* pr, v3d_stream_t stream);
/* The same tail over the LIVE tiles only.  tile_state: the v3d_conv2d_bg_tiles(B, H, W) words the background-skipping 3x3 layer that
 * wrote x_hi / x_lo keeps (5 x 16 tiles in (b, ty, tx) order; 0 = the tile holds that layer's empty-map response).  A 1x1 layer adds
 * no reach: such a tile's head output is bg_maps (Cout2, H, W) fp32 -- v3d_conv2d_1x1_head_fused applied to that layer's empty-map
 * planes of one image -- and is copied from there; the tile's input planes are not read (f16s: the range flag covers the computed
 * tiles only).  Same bits as v3d_conv2d_1x1_head_fused on the same planes.  The launch takes at most max_workgroups CUs (0 = half
 * of them) and loops when the live tiles need more.  A map of more than 4 096 tiles computes every pixel. */
int v3d_conv2d_1x1_head_fused_tiles(const void* x_hi, const void* x_lo, const void* w1_image, const float* b1, int relu1,
                                    const void* w2_image, const float* b2, int relu2, int B, int H, int W, int Cmid, int Cout2,
                                    float* y_nchw, const v3d_conv2d_prec* pr, const uint32_t* tile_state, const float* bg_maps,
                                    int max_workgroups, v3d_stream_t stream);
/* fp32 (B, C, H, W) -> split planes (B, H, W, C) of `prec` (f16s: pieces of x * act_entry[0]; act_entry NULL for bf16x3) */
int v3d_nchw_to_split_nhwc(const float* x, int B, int C, int H, int W, void* out_hi, void* out_lo, int prec,
                           const float* act_entry, v3d_stream_t stream);
/* .dense() of the last sparse stage straight into that input format: planes (B,H,W,C*D), channel = c*D + z. */
int v3d_densify_nhwc_split(const float* feat, const int32_t* coords, const int32_t* n, int cap, int B, int C,
                           const int32_t* spatial_shape_host, void* out_hi, void* out_lo, v3d_stream_t stream);
/* ... and back: bf16 split planes (B,H,W,C) -> fp32 (B,C,H,W) = hi + lo (C even).  The gradient of the BEV map leaving
 * v3d_dense_train_backward_split for the sparse training plan, which takes fp32 NCHW. */
int v3d_split_nhwc_to_nchw(const void* x_hi, const void* x_lo, int B, int C, int H, int W, float* out, v3d_stream_t stream);
/* The convolutions (+ .dense()) of the frame the plan forwarded LAST, on the site lists and neighbour tables that call left
 * behind: no voxelizer, no rulebook build -- the "rulebooks prebuilt" timing variant.  Same outputs. */
int v3d_backbone_forward_reuse(v3d_backbone* plan, int B, float* dense_nchw, void* dense_hi, void* dense_lo, v3d_stream_t stream);

/* The same plan fed with EXISTING voxels -- voxel_mean (M, C) f32 and coords (M, 4) i32 (b, z, y, x), M <= the plan's voxel
 * capacity, rows frame-sorted as core/preprocess.py:26-33 produces them -- instead of raw points: what Second.forward(item) /
 * Second.inference(item) (detector/second.py:26-35, called by train.py:63 and inference.py:38) hold.  Two device copies replace
 * the voxelizer; everything after is v3d_backbone_forward. */
int v3d_backbone_forward_voxels(v3d_backbone* plan, const float* voxel_mean, const int32_t* coords, int n_voxels, int B,
                                float* dense_nchw, void* dense_hi, void* dense_lo, v3d_stream_t stream);

/* ---- ProposalLoss (detector/proposal.py:100-141) and its gradient with respect to the FUSED head maps (B, n_cls * n_yaw * 8, H, W:
 * class channel cls * n_yaw + yaw, box channel n_cls * n_yaw + (cls * 7 + d) * n_yaw + yaw -- ProposalLayer.reshape_cls / reshape_reg)
 * in one pass: sigmoid focal loss (ops/focal_loss.py; alpha < 0 disables the class weight) over M_cls + smooth-L1 over M_reg (yaw
 * term / pi, counted three times as upstream broadcasts it), both divided by max(#M_reg, 1).  losses[3] = cls_loss, reg_loss,
 * normalizer; dmaps = d(cls_loss)/d(maps) in the class channels, d(reg_loss)/d(maps) in the box channels; _scale multiplies the two
 * channel groups with the upstream gradients (device scalars).  fp32, bit-repeatable. */
size_t v3d_proposal_loss_workspace(void);
int v3d_proposal_loss_fwd_bwd(const float* maps, const int8_t* g_cls, const uint8_t* m_cls, const float* g_reg, const uint8_t* m_reg,
                              int B, int n_cls, int n_yaw, int H, int W, float alpha, float gamma, float* losses, float* dmaps,
                              void* workspace, size_t workspace_bytes, v3d_stream_t stream);
int v3d_proposal_loss_scale(float* dmaps, int B, int n_cls, int n_yaw, int H, int W, const float* g_cls, const float* g_reg,
                            v3d_stream_t stream);

/* The same loss for a head with a direction classifier (cfg.DIRECTION; replaces ProposalLoss.forward of vision3d_amd/detector/proposal.py
 * with DIRECTION enabled -- upstream's detector/proposal.py:100-141 has neither term): maps (B, n_cls * n_yaw * 9, H, W) = [cls | reg |
 * dir], direction channel n_cls * n_yaw * 8 + cls * n_yaw + yaw; g_dir i8 (> 0 = bit 1) in the layout of g_cls.  cls_loss as above;
 * reg_loss as above, with sin_yaw != 0 the yaw column's smooth-L1 argument is sin(P_yaw - G_yaw) (gradient smooth_l1'(sin D) cos D);
 * dir_loss = sum over M_reg of max(x, 0) - x g + log1p(exp(-|x|)) / max(#M_reg, 1), gradient sigmoid(x) - g.  losses[4] = cls_loss,
 * reg_loss, dir_loss, normalizer; dmaps = the three gradients in their channel groups.  _scale multiplies the three groups with
 * their upstream gradients (device scalars; one: a device 1.0f) -- four launches of the two-way scale kernel.  fp32, bit-repeatable. */
size_t v3d_proposal_dir_loss_workspace(void);
int v3d_proposal_dir_loss_fwd_bwd(const float* maps, const int8_t* g_cls, const uint8_t* m_cls, const float* g_reg, const uint8_t* m_reg,
                                  const int8_t* g_dir, int sin_yaw, int B, int n_cls, int n_yaw, int H, int W, float alpha, float gamma,
                                  float* losses, float* dmaps, void* workspace, size_t workspace_bytes, v3d_stream_t stream);
int v3d_proposal_dir_loss_scale(float* dmaps, int B, int n_cls, int n_yaw, int H, int W, const float* g_cls, const float* g_reg,
                                const float* g_dir, const float* one, v3d_stream_t stream);

/* The same loss for a head with an IoU-aware confidence logit (cfg.IOU_HEAD; replaces ProposalLoss.forward of
 * vision3d_amd/detector/proposal.py with IOU_HEAD enabled -- upstream's detector/proposal.py:100-141 has no such term): maps
 * (B, n_cls * n_yaw * (9 + with_dir), H, W) = [cls | reg | (dir) | iou], with_dir = (g_dir != NULL); anchors (n_cls, n_yaw, H, W, 7).
 * cls_loss, reg_loss and dir_loss are bit for bit those of v3d_proposal_loss_fwd_bwd / v3d_proposal_dir_loss_fwd_bwd on the same channels.
 * iou_loss = sum over M_reg of max(z, 0) - z t + log1p(exp(-|z|)) / max(#M_reg, 1), z the IoU logit and t = clamp(IoU3D(P, G), 0, 1) a
 * constant: the rotated 3-D IoU of v3d_iou3d_loss_fwd_bwd between the boxes decoded from the predicted residuals and from g_reg, both
 * RELATIVE to the anchor's centre (xyz = d * (diag, diag, a_h), wlh = exp(d) * a_wlh, yaw = d + a_yaw); gradient (sigmoid(z) - t) /
 * normalizer in the IoU channels at M_reg, exactly 0 elsewhere, none in the box channels.  losses[5] = cls_loss, reg_loss, dir_loss (0
 * without the group), iou_loss, normalizer; dmaps = all gradients in their channel groups; iou_target (nullable; B * n_cls * n_yaw * H * W)
 * = t at M_reg, 0 elsewhere.  _scale multiplies the four (three: g_dir NULL) groups with their upstream gradients (device scalars; one:
 * a device 1.0f).  fp32, no float atomics, bit-repeatable, no host read. */
size_t v3d_proposal_iou_loss_workspace(void);
int v3d_proposal_iou_loss_fwd_bwd(const float* maps, const float* anchors, const int8_t* g_cls, const uint8_t* m_cls, const float* g_reg,
                                  const uint8_t* m_reg, const int8_t* g_dir /*NULL: no direction group*/, int sin_yaw, int B, int n_cls,
                                  int n_yaw, int H, int W, float alpha, float gamma, float* losses, float* dmaps, float* iou_target,
                                  void* workspace, size_t workspace_bytes, v3d_stream_t stream);
int v3d_proposal_iou_loss_scale(float* dmaps, int B, int n_cls, int n_yaw, int H, int W, const float* g_cls, const float* g_reg,
                                const float* g_dir /*NULL: no direction group*/, const float* g_iou, const float* one, v3d_stream_t stream);

/* ---- RefinementLoss (PV-RCNN stage 2; this repository's definition, tests/refine_targets_ref.py) and its gradient in ONE launch.
 * rows = B * n RoIs.  R_reg: 7 residuals per row, row stride ld_reg floats; R_cls: one confidence logit per row, stride ld_cls
 * (the two halves of the head's (rows, 8) output are read in place).  G_conf (rows) soft targets, G_reg (rows, 7), M_cls / M_reg
 * (rows) u8.  losses[4] = {cls, reg, #M_cls, #M_reg}: cls = sum over M_cls of BCE-with-logits(R_cls, G_conf) / max(#M_cls, 1),
 * reg = sum over M_reg and the 7 components of smooth-L1 (beta 1) / max(#M_reg, 1).  dR_reg (rows, 7), dR_cls (rows): contiguous
 * gradients of reg / cls; _scale multiplies them with the upstream gradients (device scalars).  Double sums in a fixed order:
 * bit-repeatable.  Unlike v3d_proposal_loss_* there is no _workspace query: one workgroup reduces in LDS, nothing is staged in
 * global memory. */
int v3d_refine_loss_fwd_bwd(const float* R_reg, int ld_reg, const float* R_cls, int ld_cls, const float* G_conf, const float* G_reg,
                            const uint8_t* M_cls, const uint8_t* M_reg, int rows, float* losses, float* dR_reg, float* dR_cls,
                            v3d_stream_t stream);
int v3d_refine_loss_scale(float* dR_reg, float* dR_cls, int rows, const float* g_cls, const float* g_reg, v3d_stream_t stream);

/* ---- Rotated 3-D IoU / DIoU loss of ALIGNED box pairs with its gradient (no upstream counterpart: the reference regresses box
 * residuals under smooth-L1 only; this repository's definition, tests/iou_loss_ref.py).  Boxes (n, 7) f32 = (x, y, z, w, l, h, yaw),
 * z = centre, yaw in RADIANS read geometrically (w along (cos yaw, sin yaw), as v3d_points_in_boxes) -- NOT the reading of
 * v3d_box_iou_rotated_3d, which keeps the reference's.  Per pair: IoU = A_bev * overlap of the z extents / union of the volumes
 * (0 where the union is not positive); term = 1 - IoU (kind V3D_IOU_LOSS_IOU) or 1 - IoU + rho2 / c2 (V3D_IOU_LOSS_DIOU: squared
 * centre distance over the squared diagonal of the smallest world-aligned cuboid around both boxes).  A pair with a non-finite
 * number or a size <= 0 (or whose fp32 arithmetic overflows) has IoU 0, term 1 and zero gradient.
 * term (n), iou (n); d_pred / d_target (n, 7), each nullable: d term / d box, exact wherever term is differentiable, a finite
 * one-sided value at kinks.  Any n >= 0; one launch, per-pair outputs only: no workspace, no reduction, no host synchronisation. */
#define V3D_IOU_LOSS_IOU 0
#define V3D_IOU_LOSS_DIOU 1
int v3d_iou3d_loss_fwd_bwd(const float* pred, const float* target, int n, int kind, float* term, float* iou, float* d_pred,
                           float* d_target, v3d_stream_t stream);

/* The stage-2 IoU term of RefinementLoss (TRAIN.REFINEMENT_IOU_LOSS) and its gradient in ONE launch of one workgroup, like
 * v3d_refine_loss_fwd_bwd.  rows = B * n RoIs.  R_reg: 7 residuals per row, row stride ld_reg floats (the head's (rows, 8) output
 * read in place); proposals (rows, 7); gt_boxes (n_gt, 7); R_match (rows) i64 index into gt_boxes; M_reg (rows) u8.  Per row:
 * pred = VoxelNet decode of the residuals against the proposal (xyz = d * (diag, diag, h_p) + xyz_p, wlh = exp(d) * wlh_p,
 * yaw = d + yaw_p), term as above against gt_boxes[R_match].  Counted rows: M_reg set and 0 <= R_match < n_gt; the others add
 * nothing and get zero gradient.  losses[2] = {sum of term over the counted rows / max(count, 1), count}; dR_reg (rows, 7)
 * contiguous = d losses[0] / d R_reg through the decode (proposals and ground truths are constants); _scale multiplies it with
 * the upstream gradient (device scalar).  Double sum in a fixed order: bit-repeatable.  No workspace, no host synchronisation. */
int v3d_refine_iou_loss_fwd_bwd(const float* R_reg, int ld_reg, const float* proposals, const float* gt_boxes, int n_gt,
                                const int64_t* R_match, const uint8_t* M_reg, int rows, int kind, float* losses, float* dR_reg,
                                v3d_stream_t stream);
int v3d_refine_iou_loss_scale(float* dR_reg, int rows, const float* g, v3d_stream_t stream);

/* ---- Predicted Keypoint Weighting of PV-RCNN (arXiv 1912.13192 section 3.3; no upstream counterpart: model.py:72-74 hands every
 * keypoint to RoI-grid pooling with weight 1).  The definition is this repository's (detector/keypoint_weighting.py,
 * tests/keypoint_weighting_ref.py).  Replaces the last nn.Linear (H -> 1) of the head, the sigmoid and the broadcast multiply of
 * KeypointWeighting.forward_torch by ONE launch, a wave per row:
 *   logits[row] = hidden[row * ldh + 0..H) . w2 + b2[0]      (b2: device scalar, nullable = 0)
 *   feats[row * ldf + 0..C) *= sigmoid(logits[row])          in place: a column block of the (B * K, C_total) point-major matrix
 * H % 4 == 0, C % 4 == 0, ldh % 4 == 0, ldf % 4 == 0, hidden / w2 / feats 16-byte aligned (else V3D_EINVAL); any rows >= 0.
 * Fixed summation order (bit-repeatable); no workspace, no host synchronisation. */
int v3d_keypoint_weight(const float* hidden, int ldh, int H, const float* w2, const float* b2, float* feats, int ldf, int C,
                        int rows, float* logits, v3d_stream_t stream);

/* ---- KeypointSegLoss (the supervision of that head; this repository's definition) and its gradient in ONE launch of one
 * workgroup; replaces KeypointSegLoss.forward_torch (per frame a points-in-boxes test against the boxes and the grown boxes + the
 * focal loss of ops/focal_loss.py under autograd).  keypoints (B, K, 3) f32, logits (B, K) f32; the ground truth of all frames
 * flat -- gt_boxes (n_gt, 7) f32, gt_class (n_gt) i64, entries < 0 are skipped --, frame b owning rows [gt_offsets[b],
 * gt_offsets[b + 1]) (gt_offsets: (B + 1) i32 on the DEVICE, the convention of v3d_refine_targets; not read when n_gt == 0).
 *   labels (B, K) u8   1: inside a box of the keypoint's frame -- the test of v3d_points_in_boxes with use_z = 1, bit for bit;
 *                      255 (ignored): not 1, but inside a box whose (w, l, h) had extra_host[3] added in float32; else 0
 *   losses[3]          {sum over labels != 255 of sigmoid_focal_loss(logit, label, alpha, gamma) / max(#1, 1), #1, #255}
 *   d_logits (B, K)    gradient of losses[0]; _scale multiplies it with the upstream gradient (a device scalar)
 * logits == NULL: labels (and, when given, the counts in losses) alone.  B * K <= 2^24.  Counts in int, the loss in double, both
 * summed in a fixed order: bit-repeatable.  No _workspace query: the boxes are staged in LDS, 64 at a time, any number per frame. */
int v3d_keypoint_seg_loss_fwd_bwd(const float* keypoints, const float* logits, int B, int K, const float* gt_boxes,
                                  const int64_t* gt_class, const int32_t* gt_offsets, int n_gt, const float* extra_host, float alpha,
                                  float gamma, uint8_t* labels, float* losses, float* d_logits, v3d_stream_t stream);
int v3d_keypoint_seg_loss_scale(float* d_logits, int rows, const float* g, v3d_stream_t stream);

/* ---- Voxel RoI pooling for PV-RCNN's stage 2 (the pooling of Voxel R-CNN, arXiv 2012.15712; opt-in, cfg.VOXELPOOL; no upstream
 * counterpart).  The definition is this repository's (detector/voxel_roi_pool.py, tests/voxel_roi_pool_ref.py).
 * The voxel query of ONE level: points (rows, 3) f32 are the RoI grid points, frame of a row = row / rows_per_frame; the level is its
 * active coordinates coords (cap, 4) i32 = (b, z, y, x), 16-byte aligned, of which the first min(*n, cap) rows are live (n: DEVICE
 * int32 -- never read by the host: the call only enqueues and can be captured), its shape_host (D, H, W), scale_host (x, y, z) = base
 * voxel size * stride as the caller rounded it in fp32 and offset_host (x, y, z) = the grid origin.  Per point, all in fp32 with one
 * IEEE operation per step: home cell v = floor((p - offset) / scale); candidates v + (dz, dy, dx), |d| <= range_host (rz, ry, rx), in
 * ascending (dz, dy, dx) order; hit = inside the shape, an active site of the point's frame (b < 64), and
 * (dx^2 + dy^2) + dz^2 < radius * radius for d = ((u * scale + offset) + 0.5 * scale) - p.  idx (rows, nsample) i32 = the rows of the
 * first nsample hits in scan order, the rest repeating the first; no hit: all -1 and empty[row] = 1 (u8).  The result does not depend
 * on the order of the coordinate rows' insertion into the hash.  workspace: v3d_voxel_query_workspace(cap) bytes (the coordinate hash,
 * rebuilt by every call).  rows <= 2^22, nsample <= 64, range <= 7 per axis, cap < 2^24 - 1: beyond, V3D_EUNSUPPORTED. */
size_t v3d_voxel_query_workspace(int cap);
int v3d_voxel_query(const float* points, int rows, int rows_per_frame, const int32_t* coords, const int32_t* n, int cap,
                    const int32_t* shape_host, const float* scale_host, const float* offset_host, const int32_t* range_host,
                    float radius, int nsample, int32_t* idx, uint8_t* empty, void* workspace, size_t workspace_bytes,
                    v3d_stream_t stream);
/* The level's shared two-layer MLP and the max over the slots in one launch.  The first layer is linear in its input row
 * [centre(u) - p | feat(u)] and its feature part depends on the voxel alone: the caller computes P (cap, K1) = feat @ W1[3:] once per
 * active voxel (v3d_linear_rows; row stride ldp, ldp % 4 == 0, 16-byte aligned), and this kernel forms
 *   h[s, k] = relu(P[u_s, k] + ((r.x * wx[0, k] + r.y * wx[1, k]) + r.z * wx[2, k]) + b1[k]),   u_s = idx[row, s], r = centre(u_s) - p
 *   out[row * ldo + j] = max over s of relu(sum_k h[s, k] * W[k * Nout + j] + bias[j])           (fmaf chain, k ascending)
 * for j < Nout; a row whose idx[row, 0] < 0 (an empty point) is written as exact zeros.  wx (3, K1), b1 (K1), W (K1, Nout), bias (Nout)
 * with eval BatchNorm folded in by the caller; out is a column block of the caller's (rows, ldo) matrix, other columns untouched.
 * (K1, Nout) in {16, 32, 64}^2 except (16, 64) and (64, 16), rows <= 2^22, nsample <= 64: beyond, V3D_EUNSUPPORTED. */
int v3d_voxel_pool_pair(const float* P, int ldp, const int32_t* coords, int cap, const float* points, const int32_t* idx, int rows,
                        int nsample, const float* scale_host, const float* offset_host, int K1, const float* wx, const float* b1,
                        const float* W, const float* bias, int Nout, float* out, int ldo, v3d_stream_t stream);

/* ---- VectorPool aggregation (PV-RCNN++, arXiv 2102.00463; opt-in, cfg.VECTORPOOL; no upstream counterpart).  The definition is this
 * repository's (detector/vector_pool.py, tests/vector_pool_ref.py, csrc/vector_pool.hip).  xyz (B, N, 3) f32 support points, new_xyz
 * (B, M, 3) f32 queries, nv = vx * vy * vz sub-voxels; sub-voxel v = (i * vy + j) * vz + k has the centre c = q + off_v (one fp32 add per
 * coordinate), off_v = (((2 i + 1) / vx - 1) R, ((2 j + 1) / vy - 1) R, ((2 k + 1) / vz - 1) R) computed in double and rounded once.
 * fp32, the caller's stream, no host read, bit-repeatable; no atomic decides a result.  Limits: vx, vy, vz <= 3, B <= 64, N <= 2^20,
 * B * N <= 2^24, B * M * nv <= 2^22, Cr <= 32, CL in {16, 32} -- beyond them V3D_EUNSUPPORTED before any launch.
 * Query: per centre the three nearest rows of the query's own frame with d^2 = (dx dx + dy dy) + dz dz < R^2 (strict, fp32, not
 * contracted, dx = p.x - c.x), in ascending (d^2, row index) order; a row whose coordinates are bit-equal to those of a chosen one is
 * passed over.  idx (B * M * nv, 3) i32 frame-local rows (-1: missing), w (B * M * nv, 3) f32: u_k = 1 / (sqrtf(d^2_k) + 1e-8f),
 * w_k = u_k / ((u_1 + u_2) + u_3) over the rows found, 0 for the missing ones.  The support rows are binned into an (x, y) cell grid
 * in the workspace (v3d_vector_pool_query_workspace(B, N) bytes, 16-byte aligned, rebuilt by every call). */
size_t v3d_vector_pool_query_workspace(int B, int N);
int v3d_vector_pool_query(const float* xyz, const float* new_xyz, int B, int N, int M, int vx, int vy, int vz, float radius,
                          int32_t* idx, float* w, void* workspace, size_t workspace_bytes, v3d_stream_t stream);
/* Reduced features: out[n * Cr + j] = sum over m (ascending) of feat[n * ldf + m * Cr + j], m < C / Cr (C % Cr == 0). */
int v3d_vector_pool_reduce(const float* feat, int ldf, int rows, int C, int Cr, float* out, v3d_stream_t stream);
/* Gather, interpolation, offset columns, the sub-voxel's own linear layer, shift and ReLU in one launch.  fr (B * N, ldf) reduced
 * features, idx / w from the query.  Row of (query, v): [sum_k w_k fr[idx_k] (fmaf chain, k ascending) | c - p_1 | c - p_2 | c - p_3],
 * the columns of a missing neighbour zero;  out[row * ldo + v * CL + j] = relu(sum_i row[i] * W_local[(v * (Cr + 9) + i) * CL + j] +
 * shift[v * CL + j]) (fmaf chain, i ascending; eval BatchNorm folded in by the caller: its scale into W_local, the rest into shift).
 * out is a column block of the caller's (B * M, ldo) matrix, other columns untouched. */
int v3d_vector_pool_embed(const float* fr, int ldf, const float* xyz, const float* new_xyz, const int32_t* idx, const float* w, int B,
                          int N, int M, int vx, int vy, int vz, float radius, int Cr, int CL, const float* W_local, const float* shift,
                          float* out, int ldo, v3d_stream_t stream);

/* ---- Anchor-free centre heatmap head (CenterPoint, arXiv 2006.11275; stage 1 of PV-RCNN++; opt-in, cfg.CENTERHEAD; no upstream
 * counterpart).  The definition is this repository's (detector/center_head.py, tests/center_head_ref.py, csrc/center_head.hip).
 * Fused head maps (B, n_cls + 8, H, W) f32: channels [0, n_cls) heat logits, n_cls + j for j = 0..7 = dx, dy, z, log w, log l, log h,
 * sin yaw, cos yaw, raw.  geom_host = (px, py, x_lo, y_lo) as doubles: metres per cell and the grid origin.  Common limits: B <= 64,
 * n_cls <= 8, H * W <= 2^24, at most 128 objects per frame, topk <= 1024 -- beyond them V3D_EUNSUPPORTED before any launch (the sizes
 * are host data).  fp32, the caller's stream, no host read, bit-repeatable; no atomic decides a value.
 * Targets (ONE launch; every cell of heat is written, no clear needed): boxes (n, 7) f32 = (x, y, z, w, l, h, yaw) and classes (n) i32
 * of all frames flat, frame b owning rows [box_offsets_host[b], box_offsets_host[b + 1]).  fx = (x - x_lo) / px, fy likewise (fp32),
 * (ix, iy) = floor; an object is live when it lies inside the map, 0 <= class < n_cls and w, l, h are finite and > 0.  Radius r =
 * max(min_radius, int(min of the three CornerNet roots at min_overlap of (w / px, l / py))) in double, sigma = (2 r + 1) / 6.
 *   heat (B, n_cls, H, W) f32   max over the frame's live objects of the class whose (2 r + 1)^2 window covers the cell of
 *                               exp(-(du^2 + dv^2) / (2 sigma^2)); exactly 1 at a centre, exactly 0 outside every window
 *   ind / mask / cls (B, 128)   i32 iy * W + ix (-1: not live) / u8 live / i32 the given class (0 in the padding rows)
 *   reg (B, 128, 8) f32         (fx - ix, fy - iy, z, log w, log l, log h, sin yaw, cos yaw); zeros where not live */
int v3d_center_targets(const float* boxes, const int32_t* classes, const int32_t* box_offsets_host, int B, int n_cls, int H, int W,
                       const double* geom_host, double min_overlap, int min_radius, float* heat, int32_t* ind, uint8_t* mask,
                       int32_t* cls, float* reg, v3d_stream_t stream);
/* CenterLoss and its gradient with respect to the fused maps (three launches).  N = max(#mask, 1) over the batch, p = sigmoid(logit):
 * hm = sum over the heat cells of [heat == 1: -(1 - p)^alpha log p; else: -(1 - heat)^beta p^alpha log(1 - p)] / N (log p =
 * -softplus(-x), log(1 - p) = -softplus(x), no clamp); reg = sum over the masked objects and j of code_weights_host[j] * |map[n_cls + j]
 * at the object's cell - reg[j]| / N.  losses[3] = {hm, reg, N}; dmaps (the maps' shape) = d hm in the heat channels, d reg in the box
 * channels: objects of one cell add up in object order, every other box cell is an exact zero, sign(0) = 0.  _scale multiplies the two
 * channel groups with the upstream gradients (device scalars).  Sums in double in a fixed order.  workspace: 8-byte aligned. */
size_t v3d_center_loss_workspace(void);
int v3d_center_loss_fwd_bwd(const float* maps, const float* heat, const int32_t* ind, const uint8_t* mask, const float* reg, int B,
                            int n_cls, int H, int W, float alpha, float beta, const float* code_weights_host, float* losses,
                            float* dmaps, void* workspace, size_t workspace_bytes, v3d_stream_t stream);
int v3d_center_loss_scale(float* dmaps, int B, int n_cls, int H, int W, const float* g_hm, const float* g_reg, v3d_stream_t stream);
/* Peak decode (two launches, capturable).  A cell is a peak of its (frame, class) channel when its logit is >= that of each of its up
 * to eight in-map neighbours (a NaN logit is never a peak); per (frame, class) the topk peaks of highest logit, ties to the lower
 * cell, become boxes (B, n_cls * topk, 7) = ((ix + dx) px + x_lo, (iy + dy) py + y_lo, z, exp(log w, log l, log h), atan2(sin, cos)),
 * fp32 and uncontracted, and scores (B, n_cls * topk) = sigmoid(logit), group-major, score descending inside a group -- the layout of
 * v3d_proposals_topk.  A group with fewer peaks ends in slots of score 0 and an all-zero box.  workspace: 8-byte aligned. */
size_t v3d_center_decode_workspace(int B, int n_cls, int H, int W);
int v3d_center_decode(const float* maps, int B, int n_cls, int H, int W, const double* geom_host, int topk, float* boxes,
                      float* scores, void* workspace, size_t workspace_bytes, v3d_stream_t stream);

/* ---- Pillar feature encoder (the PFN layer of PointPillars, arXiv 1812.05784; opt-in, cfg.PILLAR; no upstream counterpart).  The
 * definition is this repository's: csrc/pillar_device.h states the arithmetic, detector/pillar.py:forward_torch restates it in torch,
 * tests/pillar_ref.py in float64.  features (M, P, C) f32 point slots (x, y, z first), occupancy (M) i32 in [1, P], coordinates (M, 4)
 * i32 (b, z, y, x); geometry_host = 6 floats (vx, vy, vz, vx / 2 + x0, vy / 2 + y0, vz / 2 + z0); W (channels, K = C + 6) f32.
 * Row p < occupancy of a pillar: f = [point | xyz - mean xyz of the pillar's points | xyz - pillar centre], rows beyond are zero;
 * y = W f (fmaf chain, k ascending); out[m][c] = max over ALL P rows of relu(fmaf(y, scale[c], shift[c])), so a pillar with fewer than
 * P points also offers relu(shift[c]).  winner (M, channels) i32: the lowest row that reaches the maximum, or -1 where the padded
 * candidate is strictly above every real row.  Limits: 1 <= P <= 64, 3 <= C <= 8, channels 64 or 128 -- beyond them V3D_EUNSUPPORTED
 * before any launch.  The caller's stream, no host read, no atomics: bit-repeatable.
 * _encode (eval, one launch): scale / shift = the folded BatchNorm (channels each) -> rows (M, channels).
 * _train_fwd (three launches): batch statistics over all M * P rows (the padded rows count, with y = 0) from the K + K (K + 1) / 2 input
 * moments accumulated in double, then the same encode.  bn (4, channels) f32 = mean, biased variance, scale = gamma / sqrt(var + eps),
 * shift = beta - mean * scale; moments (K + K (K + 1) / 2) f64 is kept for the backward.  The running statistics are the caller's.
 * _train_bwd (two launches): d_rows (M, channels) plus rows / winner / moments of the forward -> dW (channels, K), d_gamma, d_beta.
 * workspace: 8-byte aligned, v3d_pillar_train_workspace bytes (either call). */
int v3d_pillar_encode(const float* features, const int32_t* occupancy, const int32_t* coordinates, int M, int P, int C,
                      const float* geometry_host, const float* W, int channels, const float* scale, const float* shift, float* rows,
                      v3d_stream_t stream);
size_t v3d_pillar_train_workspace(int M, int P, int C, int channels);
int v3d_pillar_train_fwd(const float* features, const int32_t* occupancy, const int32_t* coordinates, int M, int P, int C,
                         const float* geometry_host, const float* W, int channels, const float* gamma, const float* beta, float eps,
                         float* rows, int32_t* winner, float* bn, double* moments, void* workspace, size_t workspace_bytes,
                         v3d_stream_t stream);
int v3d_pillar_train_bwd(const float* features, const int32_t* occupancy, const int32_t* coordinates, int M, int P, int C,
                         const float* geometry_host, const float* W, int channels, const float* gamma, float eps, const float* rows,
                         const int32_t* winner, const float* d_rows, const double* moments, float* dW, float* d_gamma, float* d_beta,
                         void* workspace, size_t workspace_bytes, v3d_stream_t stream);

/* ---- Dynamic pillar feature encoder (DynamicPillarVFE of MVF, arXiv 1910.06528; opt-in, cfg.PILLAR.DYNAMIC; no upstream counterpart):
 * the encoder above over the outputs of v3d_voxelize_dynamic -- every point of a pillar counts, there is no slot tensor and no cap.
 * The definition is this repository's: csrc/pillar_device.h "The DYNAMIC encoder", restated by DynamicPillarFeatureNet.forward_torch
 * (detector/pillar.py) in torch and by tests/pillar_dynamic_ref.py in float64.  points (n_points, C) f32 = the frames concatenated
 * (x, y, z first); point_voxel (n_points) i32 = the row of every point, any value outside [0, M) = dropped; voxel_mean (M, C) f32,
 * occupancy (M) i32 = the true counts (>= 1), coordinates (M, 4) i32 (b, z, y, x); geometry_host and W as above.
 * Kept point i of pillar v: f = [point | xyz - voxel_mean[v, :3] | xyz - pillar centre]; y = W f (fmaf chain, k ascending);
 * out[v][c] = max over the pillar's points of relu(fmaf(y, scale[c], shift[c])); no padded candidate.  winner (M, channels) i32 = the
 * FLAT index of the point that reaches the maximum, the lowest among equals: the results do not depend on the order of the points.
 * Limits: 3 <= C <= 8, channels 64 or 128, n_points and M <= 2^22 -- beyond them V3D_EUNSUPPORTED before any launch; M = 0 returns
 * V3D_OK and launches nothing.  The caller's stream, no host read, no float atomics (an integer cursor per pillar builds the point
 * lists): two runs agree bit for bit.  Inconsistent inputs (occupancy that does not match point_voxel, indices out of range) never
 * make a kernel leave its buffers: surplus points of a pillar are ignored, a pillar without a listed point gives a zero row, winner -1.
 * _encode (eval, three launches: offsets, point lists, encode): scale / shift = the folded BatchNorm; winner may be NULL.
 * _train_fwd (five launches): batch statistics over the N_kept = sum(occupancy) kept points (no padded rows) from the double moments,
 * then the same encode.  bn (4, channels) as above; moments (K + K (K + 1) / 2 + 1) f64, the LAST entry = N_kept -- known on the device
 * only, read there by the statistics and by the backward.  One kept point is legal (variance 0).
 * _train_bwd (two launches): as v3d_pillar_train_bwd with N = N_kept; a winner is followed only where point_voxel[winner] names the
 * pillar.  Gradients reach W, gamma and beta, never the points.
 * workspace: 8-byte aligned, v3d_pillar_dynamic_workspace bytes (any of the three calls). */
size_t v3d_pillar_dynamic_workspace(int n_points, int M, int C, int channels);
int v3d_pillar_dynamic_encode(const float* points, const int32_t* point_voxel, int n_points, const float* voxel_mean,
                              const int32_t* occupancy, const int32_t* coordinates, int M, int C, const float* geometry_host,
                              const float* W, int channels, const float* scale, const float* shift, float* rows, int32_t* winner,
                              void* workspace, size_t workspace_bytes, v3d_stream_t stream);
int v3d_pillar_dynamic_train_fwd(const float* points, const int32_t* point_voxel, int n_points, const float* voxel_mean,
                                 const int32_t* occupancy, const int32_t* coordinates, int M, int C, const float* geometry_host,
                                 const float* W, int channels, const float* gamma, const float* beta, float eps, float* rows,
                                 int32_t* winner, float* bn, double* moments, void* workspace, size_t workspace_bytes,
                                 v3d_stream_t stream);
int v3d_pillar_dynamic_train_bwd(const float* points, const int32_t* point_voxel, int n_points, const float* voxel_mean,
                                 const int32_t* coordinates, int M, int C, const float* geometry_host, const float* W, int channels,
                                 const float* gamma, float eps, const float* rows, const int32_t* winner, const float* d_rows,
                                 const double* moments, float* dW, float* d_gamma, float* d_beta, void* workspace,
                                 size_t workspace_bytes, v3d_stream_t stream);

/* ---- The pillar encoder writing the dense head's input itself (opt-in, cfg.PILLAR.PLAN; runtime.PillarPlan; no upstream counterpart):
 * v3d_pillar_encode whose rows never reach memory as fp32 -- no (M, channels) rows, no canvas, no v3d_nchw_to_split_nhwc.
 * features (cap, P, C), occupancy (cap), coordinates (cap, 4) as above, but the row count is *n_voxels in DEVICE memory: rows
 * m < min(max(*n_voxels, 0), cap) count (the grid is sized from cap; no host read).  For each of them the `channels` numbers are bit
 * for bit those of v3d_pillar_encode; every number is stored as the hi / lo 16-bit pieces of `prec` (csrc/split_prec.h; V3D_PREC_F16S:
 * of value * act_entry[0]) in out_hi / out_lo (B, H, W, channels) at pixel (b, y, x) = coordinates[m][0, 2, 3] -- the z index is ignored,
 * as PillarFeatureNet's canvas ignores it -- and bit (b * H + y, x) of occ, the INVERTED bitmap in the layout of
 * v3d_bev_occupancy_bits, is cleared.  V3D_PREC_F16S: a magnitude beyond act_entry[2] raises *range_flag (nullable) to 2 (atomicMax).
 * A row whose (b, y, x) lies outside the map is skipped: nothing of it is stored or marked.  Several rows on one pixel (the
 * voxelizer produces none): one of them wins each 2-byte store.  The planes are written at the rows' pixels only -- the caller
 * zeroes the rest -- and occ is the caller's to reset: v3d_pillar_planes_clear does both.
 * Limits: those of v3d_pillar_encode with channels == 128 -- beyond them V3D_EUNSUPPORTED before any launch; cap == 0 launches nothing.
 * One launch on the caller's stream.
 * _planes_clear (one launch, in front of _encode_planes on the same stream): occ back to all ones, *flag (nullable) to 0 and, where
 * prev_coordinates is not NULL, the pixels of the rows m < min(max(*prev_n, 0), cap) of that list zeroed in both planes (16-byte
 * aligned) -- the start of a frame on PERSISTENT planes, which then need no fill: a pixel of both frames ends on the new values. */
int v3d_pillar_encode_planes(const float* features, const int32_t* occupancy, const int32_t* coordinates, const int32_t* n_voxels, int cap,
                             int P, int C, const float* geometry_host, const float* W, int channels, const float* scale,
                             const float* shift, int B, int H, int Wd, int prec, const float* act_entry, int32_t* range_flag,
                             void* out_hi, void* out_lo, uint32_t* occ, v3d_stream_t stream);
int v3d_pillar_planes_clear(const int32_t* prev_coordinates, const int32_t* prev_n, int cap, int B, int H, int Wd, int channels,
                            void* out_hi, void* out_lo, uint32_t* occ, int32_t* flag, v3d_stream_t stream);

/* ---- Training plan: the sparse half of a train step (train.py:63-67 through detector/second.py:41-46 and
 * detector/sparse_cnn.py:15-30,151-175) as ONE call forwards and ONE call backwards, no host synchronisation.
 * Every layer must be conv + BatchNorm1d (training mode: batch statistics) [+ ReLU] with a power-of-two Cout in [4, 256].
 * Parameters are read from the caller's device pointers on every call (they change every optimiser step); the running
 * statistics are updated in place exactly as nn.BatchNorm1d would (momentum, unbiased variance, num_batches_tracked += 1).
 * forward:  voxel_mean (n_voxels, C) f32, coords (n_voxels, 4) i32 [b, z, y, x] (the Preprocessor's item) -> dense_out
 *           (B, Cout, D, H, W) f32 or dense_nhwc_bf16; activations needed by the backward stay in the plan's training arena (allocated by the
 *           first call: v3d_backbone_train_arena_bytes).
 * backward: grad_dense (B, Cout, D, H, W) f32 -> grad_weight (K, Cin, Cout), grad_gamma (Cout), grad_beta (Cout) of every
 *           layer.  Must follow a train_forward of the same plan; the layer array is the same (host) array of device pointers.
 * Deterministic: no atomics in any reduction. */
typedef struct {
  const float* weight;          /* (K, Cin, Cout) f32 */
  const float* gamma;           /* BatchNorm weight (Cout) */
  const float* beta;            /* BatchNorm bias (Cout) */
  float* running_mean;          /* nullable pair */
  float* running_var;
  int64_t* num_batches_tracked; /* nullable */
  float eps, momentum;
  float* grad_weight;           /* backward outputs (ignored by the forward) */
  float* grad_gamma;
  float* grad_beta;
} v3d_train_layer;
int v3d_backbone_train_forward(v3d_backbone* plan, const float* voxel_mean, const int32_t* coords, int n_voxels, int B,
                               const v3d_train_layer* layers_host, float* dense_out /*exactly one of the two outputs*/,
                               void* dense_nhwc_bf16 /*(B, H, W, Cout * D) bf16, channel = c * D + z: the BEV map as the bf16
                               autocast RPN consumes it (torch channels_last), rounded to nearest even*/,
                               v3d_stream_t stream);
int v3d_backbone_train_backward(v3d_backbone* plan, const float* grad_dense /*exactly one of the two gradients*/,
                                const void* grad_nhwc_bf16, int B, const v3d_train_layer* layers_host, v3d_stream_t stream);
size_t v3d_backbone_train_arena_bytes(const v3d_backbone* plan);
/* Coordinate-only pass + v3d_backbone_tune: builds the rulebooks for these voxels (no convolution), waits for `stream` and takes
 * the kernel-choice hints from the row counts.  Lets the FIRST training step run the kernels of all later steps (a training
 * forward cannot be repeated after tuning: it updates the running statistics).  Blocking; never during stream capture. */
int v3d_backbone_tune_from_voxels(v3d_backbone* plan, const int32_t* coords, int n_voxels, int B, v3d_stream_t stream);


/* ---- Dense TRAIN path of the BEV head (csrc/dense_train.hip): the RPN's Conv2d(128 -> 128, 3x3 pad 1 | 1x1, bias-free) +
 * BatchNorm2d (batch statistics) + ReLU layers and the fused 1x1 [cls | reg] head, forward and backward, bf16 storage / fp32
 * accumulation (the arithmetic of the reference's stack under torch autocast).  Replaces what train.py:58-66 runs through
 * cuDNN for detector/second.py:58-94 and detector/proposal.py:19-22.  All activations: bf16 NHWC (B, H, W, 128) = torch
 * channels_last bfloat16; every reduction is two-level in a fixed order (bit-repeatable).  128 channels are fixed. */
size_t v3d_dense_train_weight_image_bytes(int ksize);
/* weight (128, 128, k, k) fp32 -> bf16 fragment image; transpose = 0: forward, 1: data gradient (channels swapped, taps flipped) */
int v3d_dense_train_pack_weights(const float* weight, int ksize, int transpose, void* image, v3d_stream_t stream);
int v3d_dense_train_conv_tiles(int B, int H, int W); /* tiles of one convolution = rows of its `stats` output */
/* y = conv(x) (no bias, stride 1, pad k/2); stats (nullable): (tiles, 2, 128) fp32 per-tile channel sums / sums of squares of y */
int v3d_dense_train_conv(const void* x, const void* image, int B, int H, int W, int ksize, void* y, float* stats,
                         v3d_stream_t stream);
/* per-tile sums -> mean / invstd (biased variance, eps); running statistics (nullable pair; momentum, unbiased variance) and
 * num_batches_tracked (nullable) updated in place -- nn.BatchNorm2d's training-mode bookkeeping */
int v3d_dense_train_bn_finalize(const float* stats, int tiles, long long count, float eps, float momentum, float* mean,
                                float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                v3d_stream_t stream);
/* y = relu?((x - mean) * invstd * gamma + beta), M = B*H*W pixels */
int v3d_dense_train_bn_relu_apply(const void* x, long long M, const float* mean, const float* invstd, const float* gamma,
                                  const float* beta, int relu, void* y, v3d_stream_t stream);
size_t v3d_dense_train_bn_bwd_workspace(void);
/* x = the layer's raw convolution output, dy = gradient w.r.t. the post-ReLU output -> dx (may alias dy), dgamma, dbeta.
 * The ReLU mask is the forward's: the fp32 expression v3d_dense_train_bn_relu_apply stores, recomputed from x -- it equals
 * (y > 0) of that call's output on every element. */
int v3d_dense_train_bn_relu_bwd(const void* x, const void* dy, long long M, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, int relu, void* dx, float* dgamma, float* dbeta,
                                void* workspace, size_t workspace_bytes, v3d_stream_t stream);
/* dW (128, 128, k, k) fp32 = sum over pixels of dy (x) x shifted by the tap, straight from the NHWC tensors (x: the layer's bf16
 * input, dy: the bf16 gradient of its raw output).  Bit-repeatable (fixed-order two-level reduction). */
size_t v3d_dense_train_wgrad_workspace(int ksize);
int v3d_dense_train_wgrad(const void* x, const void* dy, int B, int H, int W, int ksize, float* dw, void* workspace,
                          size_t workspace_bytes, v3d_stream_t stream);
/* fused 1x1 head, O in {8, 16, 24, 32, 48, 64} outputs with bias: maps fp32 (B, O, H, W) */
size_t v3d_dense_train_head_workspace(int O);
int v3d_dense_train_head_fwd(const void* feat, int B, int H, int W, const float* weight, const float* bias, int O, float* maps,
                             v3d_stream_t stream);
int v3d_dense_train_head_bwd(const void* feat, const float* dmaps, int B, int H, int W, const float* weight, int O, void* dfeat,
                             float* dweight, float* dbias, void* workspace, size_t workspace_bytes, v3d_stream_t stream);
/* The whole dense half of a train step, one call per direction (n_layers x [conv + batch-statistics BatchNorm + ReLU] + head).
 * arena: a device buffer of v3d_dense_train_arena_bytes owned by the caller, cleared once by v3d_dense_train_arena_init; it
 * carries the forward's activations and statistics to the backward of the SAME step.  bev / dbev: bf16 NHWC (B, H, W, 128). */
typedef struct {
  const float* weight;               /* (128, 128, k, k) */
  const float* gamma;                /* BatchNorm2d weight / bias */
  const float* beta;
  float* running_mean;               /* nullable pair; updated by the forward */
  float* running_var;
  int64_t* num_batches_tracked;      /* nullable */
  float eps, momentum;
  int32_t ksize;                     /* 1 or 3 */
  float* grad_weight;                /* outputs of the backward (unused by the forward) */
  float* grad_gamma;
  float* grad_beta;
} v3d_dense_train_layer;
size_t v3d_dense_train_arena_bytes(int B, int H, int W, int n_layers, int O);
int v3d_dense_train_arena_init(void* arena, int B, int H, int W, int n_layers, int O, v3d_stream_t stream);
int v3d_dense_train_forward(const void* bev, int B, int H, int W, const v3d_dense_train_layer* layers, int n_layers,
                            const float* head_weight, const float* head_bias, int O, void* arena, float* maps, v3d_stream_t stream);
int v3d_dense_train_backward(const void* bev, const float* dmaps, int B, int H, int W, const v3d_dense_train_layer* layers,
                             int n_layers, const float* head_weight, int O, void* arena, float* dhead_weight, float* dhead_bias,
                             void* dbev, v3d_stream_t stream);
/* The same step in fp32-class arithmetic ("bf16x3"): what the reference's fp32 train.py:58-66 (no autocast) needs from the dense half.
 * Every tensor is a split pair of bf16 NHWC planes (value = hi + lo: 16 significant bits), every product three MFMA terms with fp32
 * accumulation (2^-17 per product; scale-free, so gradients need no calibration): convolutions and data gradients on
 * v3d_conv2d_nhwc_split, the weight gradient as three passes of the bf16 kernel over (hi, hi), (hi, lo), (lo, hi), statistics /
 * normalisation / head gradients in fp32 on hi + lo.  Same layer descriptors, same reductions (fixed order, bit-repeatable); O <= 16.
 * bev_hi / bev_lo, dbev_hi / dbev_lo: (B, H, W, 128) bf16 planes; the backward reads the SAME bev planes and arena as the forward. */
size_t v3d_dense_train_arena_bytes_split(int B, int H, int W, int n_layers, int O);
int v3d_dense_train_forward_split(const void* bev_hi, const void* bev_lo, int B, int H, int W, const v3d_dense_train_layer* layers,
                                  int n_layers, const float* head_weight, const float* head_bias, int O, void* arena, float* maps,
                                  v3d_stream_t stream);
int v3d_dense_train_backward_split(const void* bev_hi, const void* bev_lo, const float* dmaps, int B, int H, int W,
                                   const v3d_dense_train_layer* layers, int n_layers, const float* head_weight, int O, void* arena,
                                   float* dhead_weight, float* dhead_bias, void* dbev_hi, void* dbev_lo, v3d_stream_t stream);
/* The split step's weight gradient on its own: dw (128, 128, k, k) fp32 = x_hi (*) dy_hi + x_hi (*) dy_lo + x_lo (*) dy_hi (the exact
 * product of the two split tensors minus its lo * lo term), three passes of the kernel of v3d_dense_train_wgrad and ONE fixed-order
 * reduction over their slab partials.  workspace: 3 * v3d_dense_train_wgrad_workspace(ksize) bytes, V3D_EWORKSPACE below that. */
int v3d_dense_train_wgrad_split(const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, int B, int H, int W, int ksize,
                                float* dw, void* workspace, size_t workspace_bytes, v3d_stream_t stream);

/* ---- KITTI 2-D bbox, BEV and 3-D average precision and average orientation similarity (AOS) (vision3d_amd/evaluation/kitti.py;
 * the protocol is written out in its docstring).  The upstream project has no evaluator.  All frames form one ragged batch: rows
 * of frame f are [off[f], off[f+1]) of the concatenated arrays, off (n_frames + 1) i32 on the device; ov_off (n_frames + 1) i64 =
 * running sum of n_dt * n_gt.
 *   gt (G, 7) f32 = rectified-camera (x, y_bottom, z, h, w, l, ry); gt_meta (G, 2) i32 = (class code, flags): bit d set =
 *   "ignored at difficulty d" (occlusion / truncation / 2-D height rule, evaluated by the caller), bit V3D_KITTI_DONTCARE_BIT
 *   set = the ground truth is a DontCare region (it is also class code OTHER, so no combo counts it);
 *   dt (D, 8) f32 = the same 7 columns + score; dt_meta (D, 2) i32 = (class code, flags): bit d set = 2-D height below
 *   MIN_HEIGHT[d].  Class codes: V3D_KITTI_CODE_*.
 *   gt_img (G, 5), dt_img (D, 5) f32 = image box (x1, y1, x2, y2) and alpha (read by bbox combos only).
 * A combo is one (class, difficulty, metric, minimum overlap); up to V3D_KITTI_MAX_COMBOS of them, on the HOST, in one array
 * whatever their metrics (beyond it V3D_EUNSUPPORTED).  The kernels take combos by value, V3D_KITTI_COMBO_CHUNK per table:
 * pass 1 launches once per chunk of V3D_KITTI_COMBO_CHUNK combos, pass 2 once per chunk of the combos it runs generically and
 * once per 16 level families (below); thresholds and AP launch once.  Launch counts never depend on the frame count.  ov holds one overlap plane per metric, ov_plane (>= sum n_dt * n_gt) floats apart: a combo reads the
 * plane ov + metric * ov_plane (BEV, 3-D, bbox), each frame-major, row = detection, column = ground truth.
 * max_dt / max_gt (host) are the largest per-frame counts: beyond V3D_KITTI_MAX_DT / V3D_KITTI_MAX_GT every entry point
 * returns V3D_EUNSUPPORTED.  Integer counters only: results are deterministic.  No host synchronisation. */
#define V3D_KITTI_MAX_DT 1024
#define V3D_KITTI_MAX_GT 256
#define V3D_KITTI_MAX_COMBOS 1024
#define V3D_KITTI_COMBO_CHUNK 64
#define V3D_KITTI_SAMPLE_PTS 41
#define V3D_KITTI_CODE_CAR 0
#define V3D_KITTI_CODE_PEDESTRIAN 1
#define V3D_KITTI_CODE_CYCLIST 2
#define V3D_KITTI_CODE_VAN 3
#define V3D_KITTI_CODE_PERSON_SITTING 4
#define V3D_KITTI_CODE_OTHER 5 /* DontCare, Misc, Truck, Tram, ... */
#define V3D_KITTI_DONTCARE_BIT 3
#define V3D_KITTI_METRIC_BEV 0
#define V3D_KITTI_METRIC_3D 1
#define V3D_KITTI_METRIC_BBOX 2 /* 2-D bbox; AOS comes from its counts */
typedef struct {
  int32_t cls;         /* class code evaluated */
  int32_t neighbour;   /* its neighbour class code (Van for Car, Person_sitting for Pedestrian), -1: none */
  int32_t difficulty;  /* 0 easy, 1 moderate, 2 hard: the flag bit read */
  int32_t metric;      /* V3D_KITTI_METRIC_*: the overlap plane read */
  float min_overlap;   /* a pair counts when overlap > min_overlap */
} v3d_kitti_combo;
/* ov_bev, ov_3d (sum n_dt * n_gt) f32: BEV and 3-D IoU, both from ONE polygon clip per pair (rotated_iou.h).  BEV in the
 * camera's (x, z) plane, extent l along (cos ry, -sin ry). */
int v3d_kitti_eval_overlaps(const float* gt, const int32_t* gt_off, const float* dt, const int32_t* dt_off, const int64_t* ov_off,
                            int n_frames, int max_dt, int max_gt, float* ov_bev, float* ov_3d, v3d_stream_t stream);
/* ov_2d (sum n_dt * n_gt) f32: IoU of the image boxes (no +1), computed in double. */
int v3d_kitti_eval_overlaps_image(const float* gt_img, const int32_t* gt_off, const float* dt_img, const int32_t* dt_off,
                                  const int64_t* ov_off, int n_frames, int max_dt, int max_gt, float* ov_2d, v3d_stream_t stream);
/* Pass 1 (greedy assignment without false positives): appends every true positive's score to its combo's row of tp_scores
 * (n_combos, capacity) at tp_count[combo] (atomic cursor; order arbitrary, capacity >= G suffices) and adds the combo's valid
 * ground truths to n_valid[combo].  tp_count and n_valid must be zero on entry.  V3D_EINVAL for a combo metric outside 0..2. */
int v3d_kitti_eval_pass1(const int32_t* gt_meta, const int32_t* gt_off, const float* dt, const int32_t* dt_meta, const int32_t* dt_off,
                         const int64_t* ov_off, const float* ov, int64_t ov_plane, int n_frames, int max_dt, int max_gt,
                         const v3d_kitti_combo* combos_host, int n_combos, int capacity, int32_t* tp_count, float* tp_scores,
                         int32_t* n_valid, v3d_stream_t stream);
/* Score thresholds of the 41 recall positions, one lane per combo, in double: sorted_scores (n_combos, capacity) = each row of
 * tp_scores sorted in DESCENDING order (entries past tp_count[combo] are not read).  thresholds (n_combos, 41) f32, n_thresholds
 * (n_combos) i32. */
int v3d_kitti_eval_thresholds(const float* sorted_scores, int capacity, const int32_t* tp_count, const int32_t* n_valid,
                              int n_combos, float* thresholds, int32_t* n_thresholds, v3d_stream_t stream);
/* Pass 2: one lane per threshold runs the greedy assignment with false positives; counts (n_combos, 41, 3) i32 += (tp, fp, fn).
 * Bbox combos also: every counted (ignored_dt == 0), unassigned detection not under the threshold whose inter / area_dt with
 * some DontCare region exceeds min_overlap is absorbed (no FP); similarity (n_combos, 41) i64 += each frame's sum over its true
 * positives of (1 + cos(alpha_gt - alpha_dt)) / 2 (double, ground-truth order) as 32.32 fixed point, llrint(sum * 2^32), by
 * integer atomics: the total is deterministic and independent of frame order.  A frame adds < 2^40 (<= 256 true positives), so
 * the total is exact below 2^31 true positives per (combo, threshold): more than 8 million frames at the per-frame limit.
 * gt_img, dt_img and similarity may be NULL when no combo is a bbox combo; rows of other combos stay as they are.  counts and
 * similarity must be zero on entry.  V3D_EINVAL for a combo metric outside 0..2 or a bbox combo without the image arrays.
 * Level families -- combos equal in (cls, neighbour, difficulty, metric), differing in min_overlap only, grouped in combo order up
 * to 12 per family -- of 3 or more combos (a COCO-style overlap sweep) run one workgroup per (frame, family) with one wave per
 * level, reading the frame's flags, scores and (when it fits) overlap tile from LDS staged once; the rule and the data are
 * those of the per-combo kernel, so counts and similarity are bit-identical either way.  Where the staging for max_dt / max_gt
 * exceeds 64 KiB of LDS, every combo runs per combo.  max_dt / max_gt must bound every frame's counts. */
int v3d_kitti_eval_pass2(const int32_t* gt_meta, const int32_t* gt_off, const float* gt_img, const float* dt, const int32_t* dt_meta,
                         const int32_t* dt_off, const float* dt_img, const int64_t* ov_off, const float* ov, int64_t ov_plane,
                         int n_frames, int max_dt, int max_gt, const v3d_kitti_combo* combos_host, int n_combos,
                         const float* thresholds, const int32_t* n_thresholds, int32_t* counts, int64_t* similarity,
                         v3d_stream_t stream);
/* Precision per threshold, its running maximum from the right, and ap (n_combos, 2) f64 = (AP_R11, AP_R40) in percent, summed in
 * the order of the definition (bit-reproducible).  With similarity (non-NULL), aos (n_combos, 2) f64 = (AOS_R11, AOS_R40) the same
 * way from similarity * 2^-32 / (tp + fp) (0 when tp + fp == 0 and for k >= n_thresholds); meaningful for bbox combos. */
int v3d_kitti_eval_ap(const int32_t* counts, const int64_t* similarity, const int32_t* n_thresholds, int n_combos, double* ap,
                      double* aos, v3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VISION3D_HIP_H */
