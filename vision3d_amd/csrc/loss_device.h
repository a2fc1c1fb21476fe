// loss_device.h -- the arithmetic the fused training losses share (proposal_loss.hip, refine_targets.hip, keypoint_weight.hip,
// center_head.hip), stated once: the fixed-order workgroup sum (v3d_block_sum: scan_device.h), the logistic front end, BCE-with-logits, the sigmoid focal loss
// (ops/focal_loss.py) and smooth-L1, each with its gradient.  fp32, one IEEE operation per operator as written (-ffp-contract=off
// is project-wide, so inlining changes no rounding): the float64 restatements under tests/ check these expressions.
#pragma once
#include <hip/hip_runtime.h>

#include "scan_device.h"  // v3d_block_sum: the fixed-order workgroup sum

// The logistic front end: e = expf(-|x|) never overflows; sigmoid(x) from it by one division.
__device__ __forceinline__ float v3d_sigmoid(float x, float& e) {
  e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// The same with q = 1 - sigmoid(x) free of cancellation: one reciprocal, p and q as its products (for x < 0 p may differ from
// v3d_sigmoid in the last place: e * (1 / (1 + e)) against e / (1 + e)).
__device__ __forceinline__ void v3d_sigmoid_pq(float x, float& e, float& p, float& q) {
  e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  p = x >= 0.f ? inv : e * inv;
  q = x >= 0.f ? e * inv : inv;
}

// softplus(x) = log(1 + exp(x)) with e = expf(-|x|): -log(1 - sigmoid(x)); softplus(-x) (same e) = -log sigmoid(x)
__device__ __forceinline__ float v3d_softplus(float x, float e) { return fmaxf(x, 0.f) + log1pf(e); }

// binary cross-entropy of the logit x against the (soft) target t, e = expf(-|x|); d/dx = sigmoid(x) - t
__device__ __forceinline__ float v3d_bce_logits(float x, float t, float e) { return fmaxf(x, 0.f) - x * t + log1pf(e); }

// Sigmoid focal loss w (1 - p_t)^gamma bce(x, t) of a hard target t in {0, 1}; w = alpha t + (1 - alpha)(1 - t), 1 for alpha < 0.
// -> the value; dx = d value / dx (bce' = prob - t, p_t' = prob (1 - prob) (2 t - 1)).  gamma == 2 takes no powf.
__device__ __forceinline__ float v3d_sigmoid_focal(float x, float t, float alpha, float gamma, float& dx) {
  float e;
  const float prob = v3d_sigmoid(x, e);
  const float bce = v3d_bce_logits(x, t, e);
  const float p_t = prob * t + (1.f - prob) * (1.f - t);
  const float q = 1.f - p_t;
  const float w = alpha >= 0.f ? alpha * t + (1.f - alpha) * (1.f - t) : 1.f;
  const float qg = gamma == 2.f ? q * q : powf(q, gamma);
  const float qg1 = gamma == 2.f ? q : powf(q, gamma - 1.f);
  dx = w * ((prob - t) * qg - bce * gamma * qg1 * prob * (1.f - prob) * (2.f * t - 1.f));
  return w * bce * qg;
}

// smooth-L1 (beta 1) of a residual -> the value; grad = the residual clamped to [-1, 1].  Weights are the caller's.
__device__ __forceinline__ float v3d_smooth_l1(float diff, float& grad) {
  const float ad = fabsf(diff);
  grad = fminf(fmaxf(diff, -1.f), 1.f);
  return ad < 1.f ? 0.5f * diff * diff : ad - 0.5f;
}
