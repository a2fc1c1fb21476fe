// keypoint_weight.hip -- PV-RCNN's Predicted Keypoint Weighting (arXiv 1912.13192, section 3.3; opt-in: cfg.PKW): a small foreground
// head scores every keypoint, the keypoint's feature row is multiplied with that score before RoI-grid pooling, and the head is
// supervised by whether the keypoint lies inside a ground-truth box.  Upstream has no statement of it: the definition is this
// repository's (detector/keypoint_weighting.py forward_torch in torch, tests/keypoint_weighting_ref.py in numpy).
//
// v3d_keypoint_weight: the tail of the head in ONE launch, a wave per keypoint row: the last layer's dot product (H -> 1; a
//   butterfly over the wave, so every lane holds the sum and the order is fixed), the sigmoid, and the row of the point-major
//   keypoint feature matrix scaled in place with 16-byte loads and stores.  Memory-bound: the row is read and written once.
// v3d_keypoint_seg_loss_fwd_bwd: labels, focal loss and its gradient in ONE launch of one workgroup (B * K is a few tens of thousands
//   of rows): the frame's ground truths prepared into LDS with pib_device.h -- the test of v3d_points_in_boxes, bit for bit --,
//   thread = keypoint (strided); counts in int, the loss in double, both summed in the fixed order of loss_device.h: bit-repeatable.
#include "loss_device.h"
#include "pib_device.h"
#include "v3d_internal.h"

#define KW_WAVES (V3D_BLOCK / V3D_WAVE)  // rows of one workgroup

__global__ __launch_bounds__(V3D_BLOCK) void keypoint_weight_kernel(const float* __restrict__ hidden, int ldh, int H,
                                                                    const float* __restrict__ w2, const float* __restrict__ b2,
                                                                    float* __restrict__ feats, int ldf, int C, int rows,
                                                                    float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * KW_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;  // (wave-uniform; no barrier below)
  const float* h = hidden + (size_t)row * ldh;
  float acc = 0.f;
  for (int k = 4 * lane; k < H; k += 4 * V3D_WAVE) {
    const float4 a = *reinterpret_cast<const float4*>(h + k);
    const float4 w = *reinterpret_cast<const float4*>(w2 + k);
    acc += (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  const float logit = acc + (b2 ? b2[0] : 0.f);
  const float s = 1.f / (1.f + expf(-logit));
  if (lane == 0) logits[row] = logit;
  float* f = feats + (size_t)row * ldf;
  for (int c = 4 * lane; c < C; c += 4 * V3D_WAVE) {
    float4 v = *reinterpret_cast<const float4*>(f + c);
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    *reinterpret_cast<float4*>(f + c) = v;
  }
}

extern "C" int v3d_keypoint_weight(const float* hidden, int ldh, int H, const float* w2, const float* b2, float* feats, int ldf, int C,
                                   int rows, float* logits, v3d_stream_t stream) {
  if (rows < 0 || H < 4 || (H & 3) || C < 4 || (C & 3) || ldh < H || (ldh & 3) || ldf < C || (ldf & 3)) return V3D_EINVAL;
  if (rows == 0) return V3D_OK;
  if (!hidden || !w2 || !feats || !logits) return V3D_EINVAL;
  if (((uintptr_t)hidden & 15) || ((uintptr_t)w2 & 15) || ((uintptr_t)feats & 15)) return V3D_EINVAL;  // 16-byte loads and stores
  hipLaunchKernelGGL(keypoint_weight_kernel, dim3(v3d_ceil_div(rows, KW_WAVES)), dim3(V3D_BLOCK), 0, (hipStream_t)stream, hidden, ldh, H,
                     w2, b2, feats, ldf, C, rows, logits);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// keypoint segmentation loss: label 1 inside a ground-truth box (class >= 0) of the keypoint's own frame, 255 (ignored) inside
// such a box grown by `extra`, else 0; sigmoid focal loss (ops/focal_loss.py: loss_device.h v3d_sigmoid_focal) over the
// labels != 255, divided by max(#label 1, 1); the gradient is written with the forward.
// ------------------------------------------------------------------------------------------------------------------------------
#define KS_MAX_GT 64  // ground truths staged per pass over a frame's keypoints (a frame with more takes several passes)

struct KsParams {
  int B, K, G;
  float extra[3];
  float alpha, gamma;
};

// every thread keeps ITS rows (tid, tid + 256, ... of every frame) through both passes: it reads back only labels it wrote itself
__global__ __launch_bounds__(V3D_BLOCK) void keypoint_seg_loss_kernel(const float* __restrict__ keypoints, const float* __restrict__ logits,
                                                                      const float* __restrict__ gt, const long long* __restrict__ gt_class,
                                                                      const int* __restrict__ gt_offsets, const KsParams p,
                                                                      unsigned char* labels, float* __restrict__ losses,
                                                                      float* __restrict__ d_logits) {
  __shared__ PibBox s_in[KS_MAX_GT], s_out[KS_MAX_GT];
  __shared__ int s_use[KS_MAX_GT];
  __shared__ int red_i[KW_WAVES];
  __shared__ double red_d[KW_WAVES];
  const int tid = threadIdx.x;
  int c_fg = 0, c_ign = 0;
  for (int b = 0; b < p.B; b++) {
    // the frame's slice of the flat ground-truth list, clamped to the list (uniform over the workgroup)
    int g0 = p.G > 0 ? gt_offsets[b] : 0, g1 = p.G > 0 ? gt_offsets[b + 1] : 0;
    g0 = max(0, min(g0, p.G));
    g1 = max(g0, min(g1, p.G));
    for (int r = tid; r < p.K; r += V3D_BLOCK) labels[(size_t)b * p.K + r] = 0;
    for (int c0 = g0; c0 < g1; c0 += KS_MAX_GT) {
      const int nb = min(KS_MAX_GT, g1 - c0);
      __syncthreads();  // (the previous pass still reads the staged boxes)
      if (tid < nb) {
        const float* bx = gt + 7 * (size_t)(c0 + tid);
        float grown[7];
#pragma unroll
        for (int q = 0; q < 7; q++) grown[q] = bx[q];
#pragma unroll
        for (int q = 0; q < 3; q++) grown[3 + q] = bx[3 + q] + p.extra[q];  // float32 sum, then the same test
        s_in[tid] = pib_prep(bx);
        s_out[tid] = pib_prep(grown);
        s_use[tid] = gt_class[c0 + tid] >= 0;
      }
      __syncthreads();
      for (int r = tid; r < p.K; r += V3D_BLOCK) {
        const size_t i = (size_t)b * p.K + r;
        int lab = labels[i];
        if (lab == 1) continue;
        const float px = keypoints[3 * i], py = keypoints[3 * i + 1], pz = keypoints[3 * i + 2];
        for (int j = 0; j < nb; j++) {
          if (!s_use[j]) continue;
          if (pib_inside(s_in[j], px, py, pz, true)) {
            lab = 1;
            break;
          }
          if (lab == 0 && pib_inside(s_out[j], px, py, pz, true)) lab = 255;
        }
        labels[i] = (unsigned char)lab;
      }
    }
    for (int r = tid; r < p.K; r += V3D_BLOCK) {
      const int lab = labels[(size_t)b * p.K + r];
      c_fg += lab == 1;
      c_ign += lab == 255;
    }
  }
  const int n_fg = v3d_block_sum<KW_WAVES>(c_fg, red_i);
  const int n_ign = v3d_block_sum<KW_WAVES>(c_ign, red_i);
  if (!logits) {  // labels alone (uniform over the workgroup)
    if (tid == 0 && losses) {
      losses[0] = 0.f;
      losses[1] = (float)n_fg;
      losses[2] = (float)n_ign;
    }
    return;
  }
  const float inv_n = 1.f / (float)max(n_fg, 1);
  const float alpha = p.alpha, gamma = p.gamma;
  double s = 0.0;
  for (int b = 0; b < p.B; b++)
    for (int r = tid; r < p.K; r += V3D_BLOCK) {
      const size_t i = (size_t)b * p.K + r;
      const int lab = labels[i];
      float gx = 0.f;
      if (lab != 255) {
        float dx;
        s += (double)v3d_sigmoid_focal(logits[i], lab == 1 ? 1.f : 0.f, alpha, gamma, dx);
        gx = dx * inv_n;
      }
      d_logits[i] = gx;
    }
  const double total = v3d_block_sum<KW_WAVES>(s, red_d);
  if (tid == 0) {
    losses[0] = (float)(total / (double)max(n_fg, 1));
    losses[1] = (float)n_fg;
    losses[2] = (float)n_ign;
  }
}

#define KS_MAX_ROWS (1 << 24)  // (counts are reported as float)

extern "C" int v3d_keypoint_seg_loss_fwd_bwd(const float* keypoints, const float* logits, int B, int K, const float* gt_boxes,
                                             const int64_t* gt_class, const int32_t* gt_offsets, int n_gt, const float* extra_host,
                                             float alpha, float gamma, uint8_t* labels, float* losses, float* d_logits,
                                             v3d_stream_t stream) {
  if (B < 0 || K < 0 || n_gt < 0 || (long long)B * K > KS_MAX_ROWS || !extra_host) return V3D_EINVAL;
  if (logits && (!losses || !d_logits)) return V3D_EINVAL;
  if ((long long)B * K > 0 && (!keypoints || !labels)) return V3D_EINVAL;
  if (n_gt > 0 && (!gt_boxes || !gt_class || !gt_offsets)) return V3D_EINVAL;
  if ((long long)B * K == 0 && !losses) return V3D_OK;
  KsParams p;
  p.B = B; p.K = K; p.G = n_gt;
  for (int q = 0; q < 3; q++) p.extra[q] = extra_host[q];
  p.alpha = alpha; p.gamma = gamma;
  hipLaunchKernelGGL(keypoint_seg_loss_kernel, dim3(1), dim3(V3D_BLOCK), 0, (hipStream_t)stream, keypoints, logits, gt_boxes,
                     (const long long*)gt_class, gt_offsets, p, labels, losses, d_logits);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_keypoint_seg_loss_scale(float* d_logits, int rows, const float* g, v3d_stream_t stream) {
  if (rows < 0 || rows > KS_MAX_ROWS || !g) return V3D_EINVAL;
  if (rows == 0) return V3D_OK;
  if (!d_logits) return V3D_EINVAL;
  return v3d_i_loss_scale(d_logits, 1, rows, rows, g, g, 64, (hipStream_t)stream);  // d_logits *= *g
}
