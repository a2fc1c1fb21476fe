// proposal_loss.hip -- the proposal loss of a SECOND train step and its gradient in one pass over the head maps.
//
// Reference: ProposalLoss (vision3d/detector/proposal.py:100-141): sigmoid focal loss on the class logits (ops/focal_loss.py:
// alpha 0.25, gamma 2) summed over the anchors with M_cls, smooth-L1 on the 7 box residuals (the yaw term divided by pi and, as
// upstream broadcasts it over the three columns it is added to, counted three times) summed over the anchors with M_reg, both
// divided by max(#M_reg, 1).  Through torch this is ~40 elementwise / reduction launches forward and backward (0.25 ms of a
// 7.4 ms step); here: count the positives, one pass that writes the gradient of both terms with respect to the FUSED head maps
// (B, n_cls * n_yaw * (1 + 7), H, W) and per-workgroup partial sums, one merge in a fixed order.  fp32, bit-repeatable.  The focal
// and smooth-L1 expressions and the workgroup sum are those of loss_device.h.
// With a direction classifier (cfg.DIRECTION, v3d_proposal_dir_loss_*): the same chain over (B, n_cls * n_yaw * 9, H, W) maps with a
// third term, BCE-with-logits of the direction logit over M_reg, and optionally the sine yaw argument -- pl_main_kernel<true>.
//   class channel of anchor (cls, yaw):            cls * n_yaw + yaw
//   box channel d of anchor (cls, yaw):  n_anchor + (cls * 7 + d) * n_yaw + yaw          (ProposalLayer.reshape_cls / reshape_reg)
//   direction channel of anchor (cls, yaw):        n_anchor * 8 + cls * n_yaw + yaw      (ProposalLayer.dir_from_fused)
// With an IoU-aware confidence head (cfg.IOU_HEAD, v3d_proposal_iou_loss_*): one more logit per anchor behind the groups above,
//   IoU channel of anchor (cls, yaw):              n_anchor * (8 + with_dir) + cls * n_yaw + yaw      (ProposalLayer.iou_from_fused)
// The class / box / direction terms come from the SAME pl_main_kernel (it takes the channel total as an argument, so they keep their
// bits); the IoU term is a pass of its own over the positives (pl_iou_kernel, iou_head_device.h) and one more partial per workgroup.
#include "iou_head_device.h"
#include "loss_device.h"
#include "v3d_internal.h"

#define PL_BLOCKS 512
#define PL_DOF 7
#define PL_WAVES (V3D_BLOCK / V3D_WAVE)

__global__ __launch_bounds__(V3D_BLOCK) void pl_count_kernel(const unsigned char* __restrict__ m_reg, long long n, int* __restrict__ partial) {
  __shared__ int red[PL_WAVES];
  int c = 0;
  for (long long i = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * V3D_BLOCK) c += m_reg[i] != 0;
  const int t = v3d_block_sum<PL_WAVES>(c, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void pl_count_merge_kernel(const int* __restrict__ partial, int blocks, float* __restrict__ normalizer) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    long long t = 0;
    for (int i = 0; i < blocks; i++) t += partial[i];
    *normalizer = t > 0 ? (float)t : 1.f;
  }
}

// maps / dmaps have O channels a frame, of which this kernel reads and writes the first n_anchor * (8 + DIR).
// thread = anchor (b, a = cls * n_yaw + yaw, pixel); dmaps gets d(cls_loss)/d(map) in the class channels and d(reg_loss)/d(map) in
// the box channels (each already divided by the normalizer); partial[block] = (sum of focal terms, sum of box terms) of the block.
// DIR (cfg.DIRECTION, v3d_proposal_dir_loss_fwd_bwd): the maps carry one direction logit per anchor behind the box channels
// (channel n_anchor * 8 + a); its BCE-with-logits against g_dir over M_reg is the third term of dmaps and of partial[block], and with
// sin_yaw the yaw column's smooth-L1 argument is sin(P_yaw - G_yaw) (gradient: the clamped argument times cos) -- nothing else differs.
template <bool DIR>
__global__ __launch_bounds__(V3D_BLOCK) void pl_main_kernel(const float* __restrict__ maps, const signed char* __restrict__ g_cls,
                                                            const unsigned char* __restrict__ m_cls, const float* __restrict__ g_reg,
                                                            const unsigned char* __restrict__ m_reg, const signed char* __restrict__ g_dir,
                                                            int sin_yaw, int B, int n_cls, int n_yaw, int HW, int O /*channels of maps*/,
                                                            float alpha, float gamma, const float* __restrict__ normalizer,
                                                            float* __restrict__ dmaps, float* __restrict__ partial) {
  __shared__ float red[PL_WAVES];
  constexpr int NT = DIR ? 3 : 2;  // loss terms
  const int n_anchor = n_cls * n_yaw;
  const long long total = (long long)B * n_anchor * HW;
  const float inv_n = 1.f / *normalizer;
  float s_cls = 0.f, s_reg = 0.f, s_dir = 0.f;
  for (long long i = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * V3D_BLOCK) {
    const int pix = (int)(i % HW);
    const int a = (int)((i / HW) % n_anchor), b = (int)(i / ((long long)HW * n_anchor));
    const int cls = a / n_yaw, yaw = a - cls * n_yaw;
    const size_t mb = (size_t)b * O * HW;
    // ---- focal term
    const size_t ic = mb + (size_t)a * HW + pix;
    const float x = maps[ic];
    float gx = 0.f;
    if (m_cls[i]) {
      float dx;
      s_cls += v3d_sigmoid_focal(x, g_cls[i] > 0 ? 1.f : 0.f, alpha, gamma, dx);
      gx = dx * inv_n;
    }
    dmaps[ic] = gx;
    // ---- box term
    const bool pos = m_reg[i] != 0;
    const float* g = g_reg + (size_t)i * PL_DOF;
#pragma unroll
    for (int d = 0; d < PL_DOF; d++) {
      const size_t ir = mb + ((size_t)n_anchor + (size_t)(cls * PL_DOF + d) * n_yaw + yaw) * HW + pix;
      float gd = 0.f;
      if (pos) {
        const float wd = d == PL_DOF - 1 ? 3.f / 3.14159265358979323846f : 1.f;
        float clamped;
        if (DIR && d == PL_DOF - 1 && sin_yaw) {
          const float diff = maps[ir] - g[d];
          s_reg += wd * v3d_smooth_l1(sinf(diff), clamped);
          clamped *= cosf(diff);
        } else {
          s_reg += wd * v3d_smooth_l1(maps[ir] - g[d], clamped);
        }
        gd = wd * clamped * inv_n;
      }
      dmaps[ir] = gd;
    }
    // ---- direction term
    if constexpr (DIR) {
      const size_t id = mb + ((size_t)n_anchor * (1 + PL_DOF) + a) * HW + pix;
      float gq = 0.f;
      if (pos) {
        const float xd = maps[id], t = g_dir[i] > 0 ? 1.f : 0.f;
        float e;
        const float prob = v3d_sigmoid(xd, e);
        s_dir += v3d_bce_logits(xd, t, e);
        gq = (prob - t) * inv_n;
      }
      dmaps[id] = gq;
    }
  }
  const float t_cls = v3d_block_sum<PL_WAVES>(s_cls, red);
  const float t_reg = v3d_block_sum<PL_WAVES>(s_reg, red);
  float t_dir = 0.f;
  if constexpr (DIR) t_dir = v3d_block_sum<PL_WAVES>(s_dir, red);
  if (threadIdx.x < NT) partial[blockIdx.x * NT + threadIdx.x] = threadIdx.x == 0 ? t_cls : (threadIdx.x == 1 ? t_reg : t_dir);
}

// losses[0 .. NT) = the terms' sums over the blocks (fixed order, double) / normalizer; losses[NT] = the normalizer
template <int NT>
__global__ void pl_finalize_kernel(const float* __restrict__ partial, int blocks, const float* __restrict__ normalizer,
                                   float* __restrict__ losses) {
  if (blockIdx.x == 0 && threadIdx.x < NT) {
    double t = 0.0;
    for (int i = 0; i < blocks; i++) t += (double)partial[i * NT + threadIdx.x];
    losses[threadIdx.x] = (float)(t / (double)*normalizer);
    if (threadIdx.x == 0) losses[NT] = *normalizer;
  }
}

// The backward of every fused loss: its stored gradient times the upstream gradients of its (one or two) loss terms, device scalars.
// buf = `groups` groups of `period` elements: the first `head` of a group *= *g_head, the rest *= *g_tail.  Grid: x strides over one
// group, y over the groups -- no index is divided.
__global__ __launch_bounds__(V3D_BLOCK) void loss_scale_kernel(float* __restrict__ buf, int groups, long long period, long long head,
                                                               const float* __restrict__ g_head, const float* __restrict__ g_tail) {
  const float gh = *g_head, gt = *g_tail;
  for (int g = blockIdx.y; g < groups; g += gridDim.y) {
    float* p = buf + g * period;
    for (long long i = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x; i < period; i += (long long)gridDim.x * V3D_BLOCK)
      p[i] *= i < head ? gh : gt;
  }
}

int v3d_i_loss_scale(float* buf, int groups, long long period, long long head, const float* g_head, const float* g_tail, int max_blocks,
                     hipStream_t st) {
  const int gy = std::min(groups, max_blocks);
  const int gx = (int)std::min<long long>(std::max(max_blocks / gy, 1), (period + V3D_BLOCK - 1) / V3D_BLOCK);
  hipLaunchKernelGGL(loss_scale_kernel, dim3(gx, gy), dim3(V3D_BLOCK), 0, st, buf, groups, period, head, g_head, g_tail);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" size_t v3d_proposal_loss_workspace(void) { return (size_t)PL_BLOCKS * (2 * sizeof(float) + sizeof(int)) + 256; }

// maps: fused head maps (B, n_cls * n_yaw * 8, H, W) fp32; g_cls int8 (> 0 = positive), m_cls / m_reg bytes (nonzero = counted),
// g_reg (B, n_cls, n_yaw, H, W, 7) fp32.  losses[3] = cls_loss, reg_loss, normalizer; dmaps: same shape as maps.
extern "C" int v3d_proposal_loss_fwd_bwd(const float* maps, const int8_t* g_cls, const uint8_t* m_cls, const float* g_reg,
                                         const uint8_t* m_reg, int B, int n_cls, int n_yaw, int H, int W, float alpha, float gamma,
                                         float* losses, float* dmaps, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (!maps || !g_cls || !m_cls || !g_reg || !m_reg || !losses || !dmaps || !workspace || B < 1 || n_cls < 1 || n_yaw < 1 || H < 1 || W < 1)
    return V3D_EINVAL;
  if (workspace_bytes < v3d_proposal_loss_workspace()) return V3D_EWORKSPACE;
  const long long n = (long long)B * n_cls * n_yaw * H * W;
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  int* counts = (int*)(partial + 2 * PL_BLOCKS);
  float* normalizer = losses + 2;
  const int blocks = (int)std::min<long long>(PL_BLOCKS, (n + V3D_BLOCK - 1) / V3D_BLOCK);
  hipLaunchKernelGGL(pl_count_kernel, dim3(blocks), dim3(V3D_BLOCK), 0, st, m_reg, n, counts);
  hipLaunchKernelGGL(pl_count_merge_kernel, dim3(1), dim3(64), 0, st, counts, blocks, normalizer);
  hipLaunchKernelGGL(pl_main_kernel<false>, dim3(blocks), dim3(V3D_BLOCK), 0, st, maps, (const signed char*)g_cls, m_cls, g_reg, m_reg,
                     (const signed char*)nullptr, 0, B, n_cls, n_yaw, H * W, n_cls * n_yaw * (1 + PL_DOF), alpha, gamma, normalizer, dmaps,
                     partial);
  hipLaunchKernelGGL(pl_finalize_kernel<2>, dim3(1), dim3(64), 0, st, partial, blocks, normalizer, losses);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_proposal_loss_scale(float* dmaps, int B, int n_cls, int n_yaw, int H, int W, const float* g_cls, const float* g_reg,
                                       v3d_stream_t stream) {
  if (!dmaps || !g_cls || !g_reg || B < 1 || n_cls < 1 || n_yaw < 1 || H < 1 || W < 1) return V3D_EINVAL;
  const long long head = (long long)n_cls * n_yaw * H * W, period = head * (1 + PL_DOF);
  return v3d_i_loss_scale(dmaps, B, period, head, g_cls, g_reg, 2048, (hipStream_t)stream);
}

// ---- the same loss of a head with a direction classifier (cfg.DIRECTION): maps (B, n_cls * n_yaw * 9, H, W) = [cls | reg | dir]
extern "C" size_t v3d_proposal_dir_loss_workspace(void) { return (size_t)PL_BLOCKS * (3 * sizeof(float) + sizeof(int)) + 256; }

// g_dir int8 (> 0 = bit 1) in the layout of g_cls; sin_yaw != 0: the sine yaw term.  losses[4] = cls_loss, reg_loss, dir_loss, normalizer
extern "C" int v3d_proposal_dir_loss_fwd_bwd(const float* maps, const int8_t* g_cls, const uint8_t* m_cls, const float* g_reg,
                                             const uint8_t* m_reg, const int8_t* g_dir, int sin_yaw, int B, int n_cls, int n_yaw, int H, int W,
                                             float alpha, float gamma, float* losses, float* dmaps, void* workspace, size_t workspace_bytes,
                                             v3d_stream_t stream) {
  if (!maps || !g_cls || !m_cls || !g_reg || !m_reg || !g_dir || !losses || !dmaps || !workspace || B < 1 || n_cls < 1 || n_yaw < 1 || H < 1 ||
      W < 1)
    return V3D_EINVAL;
  if (workspace_bytes < v3d_proposal_dir_loss_workspace()) return V3D_EWORKSPACE;
  const long long n = (long long)B * n_cls * n_yaw * H * W;
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  int* counts = (int*)(partial + 3 * PL_BLOCKS);
  float* normalizer = losses + 3;
  const int blocks = (int)std::min<long long>(PL_BLOCKS, (n + V3D_BLOCK - 1) / V3D_BLOCK);
  hipLaunchKernelGGL(pl_count_kernel, dim3(blocks), dim3(V3D_BLOCK), 0, st, m_reg, n, counts);
  hipLaunchKernelGGL(pl_count_merge_kernel, dim3(1), dim3(64), 0, st, counts, blocks, normalizer);
  hipLaunchKernelGGL(pl_main_kernel<true>, dim3(blocks), dim3(V3D_BLOCK), 0, st, maps, (const signed char*)g_cls, m_cls, g_reg, m_reg,
                     (const signed char*)g_dir, sin_yaw, B, n_cls, n_yaw, H * W, n_cls * n_yaw * (2 + PL_DOF), alpha, gamma, normalizer, dmaps,
                     partial);
  hipLaunchKernelGGL(pl_finalize_kernel<3>, dim3(1), dim3(64), 0, st, partial, blocks, normalizer, losses);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// Three channel groups, three upstream gradients, on the two-way loss_scale_kernel: each call multiplies one group by its factor and
// the rest by *one (a device 1.0f of the caller: x * 1 is exact), so every element meets exactly one factor other than 1.  The class
// and direction groups are the head and the tail of a frame's period.  The box group lies in between: it is the head of the periods
// that start one class group later, of which the last one would end behind the buffer -- that frame's box group is a call of its own.
extern "C" int v3d_proposal_dir_loss_scale(float* dmaps, int B, int n_cls, int n_yaw, int H, int W, const float* g_cls, const float* g_reg,
                                           const float* g_dir, const float* one, v3d_stream_t stream) {
  if (!dmaps || !g_cls || !g_reg || !g_dir || !one || B < 1 || n_cls < 1 || n_yaw < 1 || H < 1 || W < 1) return V3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long a = (long long)n_cls * n_yaw * H * W, box = a * PL_DOF, period = a + box + a;
  int rc = v3d_i_loss_scale(dmaps, B, period, a, g_cls, one, 2048, st);
  if (rc == V3D_OK) rc = v3d_i_loss_scale(dmaps, B, period, a + box, one, g_dir, 2048, st);
  if (rc == V3D_OK && B > 1) rc = v3d_i_loss_scale(dmaps + a, B - 1, period, box, g_reg, one, 2048, st);
  if (rc == V3D_OK) rc = v3d_i_loss_scale(dmaps + (B - 1) * period + a, 1, box, box, g_reg, g_reg, 2048, st);
  return rc;
}

// ---- the same loss of a head with an IoU-aware confidence logit (cfg.IOU_HEAD): maps (B, n_cls * n_yaw * (9 + with_dir), H, W) =
// [cls | reg | (dir) | iou].  The IoU term: at a positive anchor t = clamp(IoU3D(box(P_reg), box(G_reg)), 0, 1), both boxes decoded
// relative to the anchor's centre (iou_head_device.h), a constant of the loss; term = soft-target BCE-with-logits(z, t), gradient
// (sigmoid(z) - t) / normalizer in the IoU channel, exactly 0 off the positives.  Positives are a fraction of a percent of the
// anchors: a wave ballots M_reg and skips the clipper when it has none (the common case); else its positive lanes run it on the
// per-wave LDS slab (P2View stride 64: 8 KB a wave, 32 KB a workgroup -> 4 workgroups = 16 waves a CU, which 512 workgroups never ask
// for).  A lane touches only its own column of the slab, so no barrier guards it.
#define PL_IOU_SLAB (2 * V3D_IOU_LOSS_POLY * 64)  // points of one wave's slab

__global__ __launch_bounds__(V3D_BLOCK) void pl_iou_kernel(const float* __restrict__ maps, const float* __restrict__ anchors,
                                                           const float* __restrict__ g_reg, const unsigned char* __restrict__ m_reg, int B,
                                                           int n_cls, int n_yaw, int HW, int O, int iou_base,
                                                           const float* __restrict__ normalizer, float* __restrict__ dmaps,
                                                           float* __restrict__ iou_target, float* __restrict__ partial) {
  __shared__ v3d::P2 slab[PL_WAVES][PL_IOU_SLAB];
  __shared__ float red[PL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_anchor = n_cls * n_yaw;
  const long long per_frame = (long long)n_anchor * HW, total = (long long)B * per_frame;
  const float inv_n = 1.f / *normalizer;
  float s_iou = 0.f;
  // (the trip count is uniform over the workgroup: the ballot below sees whole waves)
  for (long long i0 = (long long)blockIdx.x * V3D_BLOCK; i0 < total; i0 += (long long)gridDim.x * V3D_BLOCK) {
    const long long i = i0 + threadIdx.x;
    const bool in = i < total, pos = in && m_reg[i] != 0;
    float gz = 0.f, t = 0.f;
    size_t iz = 0;
    if (in) {
      const int pix = (int)(i % HW), a = (int)((i / HW) % n_anchor), b = (int)(i / per_frame);
      iz = ((size_t)b * O + iou_base + a) * HW + pix;
    }
    if (__ballot(pos) != 0ull) {
      if (pos) {
        const int pix = (int)(i % HW), a = (int)((i / HW) % n_anchor), b = (int)(i / per_frame);
        const int cls = a / n_yaw, yaw = a - cls * n_yaw;
        const size_t mb = (size_t)b * O * HW;
        float p[PL_DOF], g[PL_DOF], an[PL_DOF];
#pragma unroll
        for (int d = 0; d < PL_DOF; d++) {
          p[d] = maps[mb + ((size_t)n_anchor + (size_t)(cls * PL_DOF + d) * n_yaw + yaw) * HW + pix];
          g[d] = g_reg[(size_t)i * PL_DOF + d];
          an[d] = anchors[(size_t)(i % per_frame) * PL_DOF + d];
        }
        t = v3d::ih_target_lds(p, g, an, slab[wave] + lane);
        float dz;
        s_iou += v3d::ih_soft_bce(maps[iz], t, dz);
        gz = dz * inv_n;
      }
    }
    if (in) {
      dmaps[iz] = gz;
      if (iou_target) iou_target[i] = t;
    }
  }
  const float t_iou = v3d_block_sum<PL_WAVES>(s_iou, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t_iou;
}

// losses[0 .. NT) as pl_finalize_kernel<NT> gives them (the same sums in the same order), losses[2] = 0 for NT == 2, losses[3] = the
// IoU term's sum over its blocks / normalizer, losses[4] = the normalizer
__global__ void pl_iou_finalize_kernel(const float* __restrict__ partial, int NT, int blocks, const float* __restrict__ partial_iou,
                                       const float* __restrict__ normalizer, float* __restrict__ losses) {
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    const int k = threadIdx.x;
    double t = 0.0;
    if (k < NT)
      for (int i = 0; i < blocks; i++) t += (double)partial[i * NT + k];
    else if (k == 3)
      for (int i = 0; i < blocks; i++) t += (double)partial_iou[i];
    losses[k] = (k < NT || k == 3) ? (float)(t / (double)*normalizer) : 0.f;
    if (k == 0) losses[4] = *normalizer;
  }
}

extern "C" size_t v3d_proposal_iou_loss_workspace(void) { return (size_t)PL_BLOCKS * (4 * sizeof(float) + sizeof(int)) + 256; }

// anchors (n_cls, n_yaw, H, W, 7) fp32; g_dir NULL: the maps have no direction group (sin_yaw is then ignored).  losses[5] = cls_loss,
// reg_loss, dir_loss (0 without the group), iou_loss, normalizer.  iou_target (nullable, (B, n_cls, n_yaw, H, W)): t at the positives,
// 0 elsewhere.  dmaps: every channel is written.
extern "C" int v3d_proposal_iou_loss_fwd_bwd(const float* maps, const float* anchors, const int8_t* g_cls, const uint8_t* m_cls,
                                             const float* g_reg, const uint8_t* m_reg, const int8_t* g_dir, int sin_yaw, int B, int n_cls,
                                             int n_yaw, int H, int W, float alpha, float gamma, float* losses, float* dmaps, float* iou_target,
                                             void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (!maps || !anchors || !g_cls || !m_cls || !g_reg || !m_reg || !losses || !dmaps || !workspace || B < 1 || n_cls < 1 || n_yaw < 1 ||
      H < 1 || W < 1)
    return V3D_EINVAL;
  if (workspace_bytes < v3d_proposal_iou_loss_workspace()) return V3D_EWORKSPACE;
  const long long n = (long long)B * n_cls * n_yaw * H * W;
  hipStream_t st = (hipStream_t)stream;
  const int with_dir = g_dir ? 1 : 0, NT = 2 + with_dir, n_anchor = n_cls * n_yaw;
  const int iou_base = n_anchor * (1 + PL_DOF + with_dir), O = iou_base + n_anchor;
  float* partial = (float*)workspace;
  float* partial_iou = partial + 3 * PL_BLOCKS;
  int* counts = (int*)(partial + 4 * PL_BLOCKS);
  float* normalizer = losses + 4;
  const int blocks = (int)std::min<long long>(PL_BLOCKS, (n + V3D_BLOCK - 1) / V3D_BLOCK);
  hipLaunchKernelGGL(pl_count_kernel, dim3(blocks), dim3(V3D_BLOCK), 0, st, m_reg, n, counts);
  hipLaunchKernelGGL(pl_count_merge_kernel, dim3(1), dim3(64), 0, st, counts, blocks, normalizer);
  if (with_dir)
    hipLaunchKernelGGL(pl_main_kernel<true>, dim3(blocks), dim3(V3D_BLOCK), 0, st, maps, (const signed char*)g_cls, m_cls, g_reg, m_reg,
                       (const signed char*)g_dir, sin_yaw, B, n_cls, n_yaw, H * W, O, alpha, gamma, normalizer, dmaps, partial);
  else
    hipLaunchKernelGGL(pl_main_kernel<false>, dim3(blocks), dim3(V3D_BLOCK), 0, st, maps, (const signed char*)g_cls, m_cls, g_reg, m_reg,
                       (const signed char*)nullptr, 0, B, n_cls, n_yaw, H * W, O, alpha, gamma, normalizer, dmaps, partial);
  hipLaunchKernelGGL(pl_iou_kernel, dim3(blocks), dim3(V3D_BLOCK), 0, st, maps, anchors, g_reg, m_reg, B, n_cls, n_yaw, H * W, O, iou_base,
                     normalizer, dmaps, iou_target, partial_iou);
  hipLaunchKernelGGL(pl_iou_finalize_kernel, dim3(1), dim3(64), 0, st, partial, NT, blocks, partial_iou, normalizer, losses);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// Four channel groups (three without the direction group: g_dir NULL), one upstream gradient each, on the two-way loss_scale_kernel in
// the manner of v3d_proposal_dir_loss_scale: a call multiplies one group by its factor and the rest by *one.  The class and IoU groups
// are the head and the tail of a frame's period; a group in between is the head of the periods that start where it starts, of which
// the last would end behind the buffer -- that frame's group is a call of its own.
extern "C" int v3d_proposal_iou_loss_scale(float* dmaps, int B, int n_cls, int n_yaw, int H, int W, const float* g_cls, const float* g_reg,
                                           const float* g_dir, const float* g_iou, const float* one, v3d_stream_t stream) {
  if (!dmaps || !g_cls || !g_reg || !g_iou || !one || B < 1 || n_cls < 1 || n_yaw < 1 || H < 1 || W < 1) return V3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long a = (long long)n_cls * n_yaw * H * W, box = a * PL_DOF, dir = g_dir ? a : 0, period = a + box + dir + a;
  int rc = v3d_i_loss_scale(dmaps, B, period, a, g_cls, one, 2048, st);
  if (rc == V3D_OK) rc = v3d_i_loss_scale(dmaps, B, period, period - a, one, g_iou, 2048, st);
  if (rc == V3D_OK && B > 1) rc = v3d_i_loss_scale(dmaps + a, B - 1, period, box, g_reg, one, 2048, st);
  if (rc == V3D_OK) rc = v3d_i_loss_scale(dmaps + (B - 1) * period + a, 1, box, box, g_reg, g_reg, 2048, st);
  if (rc == V3D_OK && g_dir && B > 1) rc = v3d_i_loss_scale(dmaps + a + box, B - 1, period, a, g_dir, one, 2048, st);
  if (rc == V3D_OK && g_dir) rc = v3d_i_loss_scale(dmaps + (B - 1) * period + a + box, 1, a, a, g_dir, g_dir, 2048, st);
  return rc;
}
