// refine_targets.hip -- PV-RCNN stage-2 training: RoI <-> ground-truth targets and the refinement loss (with its gradient).
//
// Upstream has no working statement of either (core/refinement_targets.py raises): the definition is this
// repository's (tests/refine_targets_ref.py restates it in numpy; core/refinement_targets.py forward_torch and
// detector/refinement.py RefinementLoss.forward_torch in torch).
//
// v3d_refine_targets: ONE launch, one workgroup per frame, no (n x g) matrix, no workspace, no host synchronisation.
//   1. the frame's ground truths (<= 128) are prepared once into LDS;
//   2. thread = RoI (strided over the frame's <= 2 048): class-aware best 3-D IoU through rotated_iou.h:iou3_prepped_lds -- the
//      statement v3d_box_iou_rotated_3d evaluates, bit for bit --, first maximal ground truth, confidence target, box encoding;
//   3. the (draw, index) ranks of the foreground / background sampling are counted from LDS (every lane reads the same entry in
//      the same step: a broadcast), the quotas from one block-wide count.
// v3d_refine_loss_fwd_bwd: ONE launch of one workgroup (B * n is a few thousand rows): counts, both loss terms and both gradients;
// sums are accumulated in double in the fixed order of loss_device.h, so the result is bit-repeatable.
#include "loss_device.h"
#include "rotated_iou.h"
#include "v3d_internal.h"

#define RT_WAVES (V3D_BLOCK / V3D_WAVE)

// LDS of refine_targets_kernel: 72 KB of clipper slabs (4 waves x 24 points x 64 lanes x 12 B, as the other IoU kernels) + 8 KB
// draws + 2 KB flags + 5.5 KB ground truths = ~88 KB static: one workgroup per CU on gfx950 (160 KB), which is all a launch of B
// workgroups asks for.  The rank loop is n^2 / 256 LDS broadcasts per thread (16 K at the 2 048-RoI limit, 352 at n = 300).
#define RT_MAX_GT 128    // ground truths of ONE frame staged per workgroup (as TA_MAX_GT of targets.hip)
#define RT_MAX_ROI 2048  // RoIs of ONE frame whose draws / flags are kept in LDS

struct RtParams {
  int n, G;
  float conf_lo, conf_hi, reg_iou, fg_iou;
  int rois_per_frame, fg_quota;  // fg_quota = floor(rois_per_frame * fg_fraction), taken on the host
};

__device__ __forceinline__ float rt_remainder(float x, float m) {  // torch.remainder: result takes the sign of m
  float r = fmodf(x, m);
  if (r != 0.f && ((m < 0.f) != (r < 0.f))) r += m;
  return r;
}

__global__ __launch_bounds__(V3D_BLOCK) void refine_targets_kernel(const float* __restrict__ rois, const long long* __restrict__ roi_class,
                                                                   const float* __restrict__ gt, const long long* __restrict__ gt_class,
                                                                   const int* __restrict__ gt_offsets, const float* __restrict__ draws,
                                                                   const RtParams p, float* __restrict__ iou_out,
                                                                   long long* __restrict__ match_out, float* __restrict__ conf_out,
                                                                   float* __restrict__ reg_out, unsigned char* __restrict__ m_cls,
                                                                   unsigned char* __restrict__ m_reg) {
  __shared__ v3d::Box3Prep s_gt[RT_MAX_GT];
  __shared__ int s_gt_class[RT_MAX_GT];
  __shared__ v3d::P2 clip_pts[RT_WAVES][24 * 64];  // the clipper's work arrays: LDS, not scratch (rotated_iou.h)
  __shared__ float clip_dist[RT_WAVES][24 * 64];
  __shared__ float s_draw[RT_MAX_ROI];
  __shared__ unsigned char s_flag[RT_MAX_ROI];  // bit 0: foreground, bit 1: gets a box target
  __shared__ int s_red[RT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(p.n, RT_MAX_ROI);
  // the frame's slice of the flat ground-truth list, clamped to the list and to the staging limit
  int g0 = gt_offsets[b], g1 = gt_offsets[b + 1];
  g0 = max(0, min(g0, p.G));
  g1 = max(g0, min(g1, p.G));
  const int g = min(g1 - g0, RT_MAX_GT);
  for (int j = tid; j < g; j += V3D_BLOCK) {
    s_gt[j] = v3d::prep_box3(gt + 7 * (size_t)(g0 + j));
    s_gt_class[j] = (int)gt_class[g0 + j];
  }
  __syncthreads();
  v3d::P2* pts = clip_pts[tid >> 6] + (tid & 63);
  float* dist = clip_dist[tid >> 6] + (tid & 63);
  int n_fg_mine = 0;
  for (int r = tid; r < n; r += V3D_BLOCK) {
    const size_t ir = (size_t)b * p.n + r;
    const float* roi = rois + 7 * ir;
    const v3d::Box3Prep br = v3d::prep_box3(roi);
    const int c = (int)roi_class[r];
    float best = 0.f;
    int arg = -1;
    for (int j = 0; j < g; j++) {
      if (s_gt_class[j] != c) continue;
      const float q = v3d::iou3_prepped_lds(br, s_gt[j], pts, dist);  // box_iou_rotated_3d(roi, gt)[r][j]
      if (q > best) {  // strict: the FIRST maximal ground truth; an overlap of 0 matches nothing
        best = q;
        arg = j;
      }
    }
    iou_out[ir] = best;
    match_out[ir] = arg < 0 ? -1 : (long long)(g0 + arg);
    conf_out[ir] = fminf(fmaxf((best - p.conf_lo) / (p.conf_hi - p.conf_lo), 0.f), 1.f);
    const bool reg = arg >= 0 && best >= p.reg_iou;
    float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (reg) {  // box_encode.encode(gt, roi) with the yaw residual wrapped to [-pi/2, pi/2)
      const float* bx = gt + 7 * (size_t)(g0 + arg);
      const float diag = sqrtf(roi[3] * roi[3] + roi[4] * roi[4]);
      t[0] = (bx[0] - roi[0]) / diag;
      t[1] = (bx[1] - roi[1]) / diag;
      t[2] = (bx[2] - roi[2]) / roi[5];
      t[3] = logf(bx[3] / roi[3]);
      t[4] = logf(bx[4] / roi[4]);
      t[5] = logf(bx[5] / roi[5]);
      t[6] = rt_remainder((bx[6] - roi[6]) + 1.57079637050628662f, 3.14159274101257324f) - 1.57079637050628662f;
    }
#pragma unroll
    for (int q = 0; q < 7; q++) reg_out[7 * ir + q] = t[q];
    const bool fg = best >= p.fg_iou;
    s_flag[r] = (unsigned char)((fg ? 1 : 0) | (reg ? 2 : 0));
    s_draw[r] = draws[ir];
    n_fg_mine += fg;
  }
  // ---- sampling: #foreground of the frame, then every RoI's rank inside its own group by (draw, index)
  const int count_fg = v3d_block_sum<RT_WAVES>(n_fg_mine, s_red);  // (its barriers also complete s_flag / s_draw)
  const bool all = p.rois_per_frame <= 0;
  const int take_fg = min(count_fg, max(p.fg_quota, 0));
  const int take_bg = min(n - count_fg, max(p.rois_per_frame - take_fg, 0));
  for (int r = tid; r < n; r += V3D_BLOCK) {
    const size_t ir = (size_t)b * p.n + r;
    const int fg = s_flag[r] & 1;
    bool taken = true;
    if (!all) {
      const float d = s_draw[r];
      int rank = 0;
      for (int s = 0; s < n; s++) {
        const float ds = s_draw[s];
        rank += ((s_flag[s] & 1) == fg) && (ds < d || (ds == d && s < r));
      }
      taken = rank < (fg ? take_fg : take_bg);
    }
    m_cls[ir] = taken;
    m_reg[ir] = taken && (s_flag[r] & 2);
  }
}

extern "C" int v3d_refine_targets(const float* proposals, const int64_t* proposal_class, int B, int n, const float* gt_boxes,
                                  const int64_t* gt_class, const int32_t* gt_offsets, int n_gt, const float* draws, float conf_lo,
                                  float conf_hi, float reg_iou, float fg_iou, int rois_per_frame, int fg_quota, float* iou,
                                  int64_t* match, float* conf, float* G_reg, uint8_t* M_cls, uint8_t* M_reg, v3d_stream_t stream) {
  if (B < 0 || n < 0 || n_gt < 0 || !(conf_hi > conf_lo)) return V3D_EINVAL;
  if (B == 0 || n == 0) return V3D_OK;
  if (!proposals || !proposal_class || !gt_offsets || !draws || !iou || !match || !conf || !G_reg || !M_cls || !M_reg) return V3D_EINVAL;
  if (n_gt > 0 && (!gt_boxes || !gt_class)) return V3D_EINVAL;
  if (n > RT_MAX_ROI) return V3D_EUNSUPPORTED;  // (a frame with more than 128 ground truths is the caller's to route elsewhere)
  RtParams p;
  p.n = n; p.G = n_gt;
  p.conf_lo = conf_lo; p.conf_hi = conf_hi; p.reg_iou = reg_iou; p.fg_iou = fg_iou;
  p.rois_per_frame = rois_per_frame; p.fg_quota = fg_quota;
  hipLaunchKernelGGL(refine_targets_kernel, dim3(B), dim3(V3D_BLOCK), 0, (hipStream_t)stream, proposals, (const long long*)proposal_class,
                     gt_boxes, (const long long*)gt_class, gt_offsets, draws, p, iou, (long long*)match, conf, G_reg, M_cls, M_reg);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// refinement loss: soft-target binary cross-entropy on the confidence logit over M_cls, smooth-L1 (beta 1) on the 7 residuals
// over M_reg, each divided by its own count (at least 1); the gradients are written with the forward.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(V3D_BLOCK) void refine_loss_kernel(const float* __restrict__ r_reg, int ld_reg, const float* __restrict__ r_cls,
                                                                int ld_cls, const float* __restrict__ g_conf,
                                                                const float* __restrict__ g_reg, const unsigned char* __restrict__ m_cls,
                                                                const unsigned char* __restrict__ m_reg, int rows,
                                                                float* __restrict__ losses, float* __restrict__ d_reg,
                                                                float* __restrict__ d_cls) {
  __shared__ int red_i[RT_WAVES];
  __shared__ double red_d[RT_WAVES];
  const int tid = threadIdx.x;
  int c_cls = 0, c_reg = 0;
  for (int i = tid; i < rows; i += V3D_BLOCK) {
    c_cls += m_cls[i] != 0;
    c_reg += m_reg[i] != 0;
  }
  const int n_cls = v3d_block_sum<RT_WAVES>(c_cls, red_i);
  const int n_reg = v3d_block_sum<RT_WAVES>(c_reg, red_i);
  const float inv_cls = 1.f / (float)max(n_cls, 1), inv_reg = 1.f / (float)max(n_reg, 1);
  double s_cls = 0.0, s_reg = 0.0;
  for (int i = tid; i < rows; i += V3D_BLOCK) {
    float gx = 0.f;
    if (m_cls[i]) {
      const float x = r_cls[(size_t)i * ld_cls], t = g_conf[i];
      float e;
      const float prob = v3d_sigmoid(x, e);
      s_cls += (double)v3d_bce_logits(x, t, e);
      gx = (prob - t) * inv_cls;
    }
    d_cls[i] = gx;
    const bool pos = m_reg[i] != 0;
#pragma unroll
    for (int d = 0; d < 7; d++) {
      float gd = 0.f;
      if (pos) {
        float clamped;
        s_reg += (double)v3d_smooth_l1(r_reg[(size_t)i * ld_reg + d] - g_reg[(size_t)i * 7 + d], clamped);
        gd = clamped * inv_reg;
      }
      d_reg[(size_t)i * 7 + d] = gd;
    }
  }
  const double t_cls = v3d_block_sum<RT_WAVES>(s_cls, red_d);
  const double t_reg = v3d_block_sum<RT_WAVES>(s_reg, red_d);
  if (tid == 0) {
    losses[0] = (float)(t_cls / (double)max(n_cls, 1));
    losses[1] = (float)(t_reg / (double)max(n_reg, 1));
    losses[2] = (float)n_cls;
    losses[3] = (float)n_reg;
  }
}

#define RL_MAX_ROWS (1 << 24)  // (counts are reported as float)

extern "C" int v3d_refine_loss_fwd_bwd(const float* R_reg, int ld_reg, const float* R_cls, int ld_cls, const float* G_conf,
                                       const float* G_reg, const uint8_t* M_cls, const uint8_t* M_reg, int rows, float* losses,
                                       float* dR_reg, float* dR_cls, v3d_stream_t stream) {
  if (!losses || rows < 0 || rows > RL_MAX_ROWS) return V3D_EINVAL;
  if (rows > 0 && (!R_reg || !R_cls || !G_conf || !G_reg || !M_cls || !M_reg || !dR_reg || !dR_cls || ld_reg < 7 || ld_cls < 1))
    return V3D_EINVAL;
  hipLaunchKernelGGL(refine_loss_kernel, dim3(1), dim3(V3D_BLOCK), 0, (hipStream_t)stream, R_reg, ld_reg, R_cls, ld_cls, G_conf, G_reg,
                     M_cls, M_reg, rows, losses, dR_reg, dR_cls);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_refine_loss_scale(float* dR_reg, float* dR_cls, int rows, const float* g_cls, const float* g_reg,
                                     v3d_stream_t stream) {
  if (rows < 0 || rows > RL_MAX_ROWS || !g_cls || !g_reg) return V3D_EINVAL;
  if (rows == 0) return V3D_OK;
  if (!dR_reg || !dR_cls) return V3D_EINVAL;
  // d_cls *= *g_cls, d_reg *= *g_reg: one launch where the two lie as [d_cls: rows | d_reg: rows * 7] (as the autograd node
  // allocates them), else one each
  hipStream_t st = (hipStream_t)stream;
  const long long n = rows;
  if (dR_reg == dR_cls + n) return v3d_i_loss_scale(dR_cls, 1, 8 * n, n, g_cls, g_reg, 64, st);
  const int rc = v3d_i_loss_scale(dR_cls, 1, n, n, g_cls, g_cls, 64, st);
  return rc != V3D_OK ? rc : v3d_i_loss_scale(dR_reg, 1, 7 * n, 7 * n, g_reg, g_reg, 64, st);
}
