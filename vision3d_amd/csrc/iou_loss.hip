// iou_loss.hip -- rotated 3-D IoU / DIoU loss of aligned box pairs with its gradient (iou_loss_device.h states the pair function).
//
// No upstream counterpart: the reference regresses box residuals under smooth-L1 only.  The definition is this repository's
// (tests/iou_loss_ref.py in float64, ops/iou_loss.py:iou3d_loss_torch in torch).
//
// v3d_iou3d_loss_fwd_bwd: one lane per pair on a grid of workgroups; per-pair outputs only, so nothing is reduced.
// v3d_refine_iou_loss_fwd_bwd: the stage-2 term in ONE launch of one workgroup, like v3d_refine_loss_fwd_bwd (B * n is a few
//   thousand rows): per row the VoxelNet decode of the residuals against the proposal, the pair function against the matched
//   ground truth, the mask, and the chain rule back through the decode; the sum in double in the fixed order of loss_device.h,
//   so the result is bit-repeatable.  No workspace, no host synchronisation.
// Both keep the clipper's two polygons in a lane-interleaved LDS slab per wave (2 x 8 points x 64 lanes x 8 B = 8 KB a wave,
// 32 KB a workgroup) instead of scratch; a lane touches only its own column, so no barrier guards the slab.
#include "iou_loss_device.h"
#include "loss_device.h"
#include "v3d_internal.h"

#define IL_WAVES (V3D_BLOCK / V3D_WAVE)
#define IL_SLAB (2 * V3D_IOU_LOSS_POLY * 64)  // points of one wave's slab

__global__ __launch_bounds__(V3D_BLOCK) void iou3d_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target, int n,
                                                               int kind, float* __restrict__ term, float* __restrict__ iou,
                                                               float* __restrict__ d_pred, float* __restrict__ d_target) {
  __shared__ v3d::P2 slab[IL_WAVES][IL_SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long i = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * V3D_BLOCK) {
    float a[7], b[7], da[7], db[7], t, u;
#pragma unroll
    for (int k = 0; k < 7; k++) {
      a[k] = pred[i * 7 + k];
      b[k] = target[i * 7 + k];
    }
    v3d::iou3d_loss_pair_lds(a, b, kind, slab[wave] + lane, t, u, da, db);
    term[i] = t;
    iou[i] = u;
#pragma unroll
    for (int k = 0; k < 7; k++) {
      if (d_pred) d_pred[i * 7 + k] = da[k];
      if (d_target) d_target[i * 7 + k] = db[k];
    }
  }
}

extern "C" int v3d_iou3d_loss_fwd_bwd(const float* pred, const float* target, int n, int kind, float* term, float* iou, float* d_pred,
                                      float* d_target, v3d_stream_t stream) {
  if (n < 0 || (kind != V3D_IOU_LOSS_IOU && kind != V3D_IOU_LOSS_DIOU)) return V3D_EINVAL;
  if (n == 0) return V3D_OK;
  if (!pred || !target || !term || !iou) return V3D_EINVAL;
  const int blocks = std::min((n + V3D_BLOCK - 1) / V3D_BLOCK, 2048);
  hipLaunchKernelGGL(iou3d_loss_kernel, dim3(blocks), dim3(V3D_BLOCK), 0, (hipStream_t)stream, pred, target, n, kind, term, iou, d_pred,
                     d_target);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// stage-2 term: pred = decode(R_reg, proposal) (core/box_encode.py: xyz = d * (diag, diag, h_p) + xyz_p, wlh = exp(d) * wlh_p,
// yaw = d + yaw_p), target = gt_boxes[R_match]; counted rows = M_reg set and 0 <= R_match < n_gt.
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool il_counted(const unsigned char* m_reg, const long long* match, int n_gt, int i) {
  const long long g = match[i];
  return m_reg[i] != 0 && g >= 0 && g < (long long)n_gt;
}

__global__ __launch_bounds__(V3D_BLOCK) void refine_iou_loss_kernel(const float* __restrict__ r_reg, int ld_reg,
                                                                    const float* __restrict__ proposals, const float* __restrict__ gt,
                                                                    int n_gt, const long long* __restrict__ match,
                                                                    const unsigned char* __restrict__ m_reg, int rows, int kind,
                                                                    float* __restrict__ losses, float* __restrict__ d_reg) {
  __shared__ v3d::P2 slab[IL_WAVES][IL_SLAB];
  __shared__ int red_i[IL_WAVES];
  __shared__ double red_d[IL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int c = 0;
  for (int i = tid; i < rows; i += V3D_BLOCK) c += il_counted(m_reg, match, n_gt, i);
  const int count = v3d_block_sum<IL_WAVES>(c, red_i);
  const float inv = 1.f / (float)max(count, 1);
  double s = 0.0;
  for (int i = tid; i < rows; i += V3D_BLOCK) {
    float g[7];
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = 0.f;
    if (il_counted(m_reg, match, n_gt, i)) {
      float d[7], p[7], b[7], a[7], e[3], da[7], db[7], t, u;
      const long long m = match[i];
#pragma unroll
      for (int k = 0; k < 7; k++) {
        d[k] = r_reg[(size_t)i * ld_reg + k];
        p[k] = proposals[(size_t)i * 7 + k];
        b[k] = gt[(size_t)m * 7 + k];
      }
      const float diag = sqrtf(p[3] * p[3] + p[4] * p[4]);
      const float scale[3] = {diag, diag, p[5]};
#pragma unroll
      for (int k = 0; k < 3; k++) {
        a[k] = d[k] * scale[k] + p[k];
        e[k] = expf(d[3 + k]);
        a[3 + k] = e[k] * p[3 + k];
      }
      a[6] = d[6] + p[6];
      v3d::iou3d_loss_pair_lds(a, b, kind, slab[wave] + lane, t, u, da, db);
      s += (double)t;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        g[k] = (da[k] * inv) * scale[k];
        const float gs = (da[3 + k] * inv) * p[3 + k];
        g[3 + k] = gs != 0.f ? gs * e[k] : 0.f;  // (a bad row has zero gradient even where its exp overflowed: no 0 * inf)
      }
      g[6] = da[6] * inv;
    }
#pragma unroll
    for (int k = 0; k < 7; k++) d_reg[(size_t)i * 7 + k] = g[k];
  }
  const double total = v3d_block_sum<IL_WAVES>(s, red_d);
  if (tid == 0) {
    losses[0] = (float)(total / (double)max(count, 1));
    losses[1] = (float)count;
  }
}

#define IL_MAX_ROWS (1 << 24)  // (the count is reported as float)

extern "C" int v3d_refine_iou_loss_fwd_bwd(const float* R_reg, int ld_reg, const float* proposals, const float* gt_boxes, int n_gt,
                                           const int64_t* R_match, const uint8_t* M_reg, int rows, int kind, float* losses,
                                           float* dR_reg, v3d_stream_t stream) {
  if (!losses || rows < 0 || rows > IL_MAX_ROWS || n_gt < 0 || (kind != V3D_IOU_LOSS_IOU && kind != V3D_IOU_LOSS_DIOU)) return V3D_EINVAL;
  if (rows > 0 && (!R_reg || !proposals || !R_match || !M_reg || !dR_reg || ld_reg < 7 || (n_gt > 0 && !gt_boxes))) return V3D_EINVAL;
  hipLaunchKernelGGL(refine_iou_loss_kernel, dim3(1), dim3(V3D_BLOCK), 0, (hipStream_t)stream, R_reg, ld_reg, proposals, gt_boxes, n_gt,
                     (const long long*)R_match, M_reg, rows, kind, losses, dR_reg);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_refine_iou_loss_scale(float* dR_reg, int rows, const float* g, v3d_stream_t stream) {
  if (rows < 0 || rows > IL_MAX_ROWS || !g) return V3D_EINVAL;
  if (rows == 0) return V3D_OK;
  if (!dR_reg) return V3D_EINVAL;
  return v3d_i_loss_scale(dR_reg, 1, 7LL * rows, 7LL * rows, g, g, 64, (hipStream_t)stream);  // dR_reg *= *g
}
