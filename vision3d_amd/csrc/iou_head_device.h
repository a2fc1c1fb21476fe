// iou_head_device.h -- the per-anchor expressions of the IoU-aware confidence head of the SECOND anchor head (cfg.IOU_HEAD): the
// decode of a residual relative to its anchor's centre, the IoU target of a positive anchor, and the soft-target BCE-with-logits
// with its gradient.  fp32, one IEEE operation per operator as written; compiled by hipcc for the kernels (proposal_loss.hip) and
// by g++ for the CPU suite (tests/host/iou_head_host_shim.cpp).  The definition is this repository's;
// tests/iou_head_ref.py restates it in float64.
//
//   box(d)  = (d_x diag, d_y diag, d_z a_h, exp(d_w) a_w, exp(d_l) a_l, exp(d_h) a_h, d_yaw + a_yaw),  diag = sqrt(a_w^2 + a_l^2)
//             -- core/box_encode.py:13-21 WITHOUT the anchor's centre: the IoU is translation invariant, and adding a 70 m coordinate
//             in fp32 would cost ~1e-5 of IoU for nothing
//   t       = clamp(IoU3D(box(P_reg), box(G_reg)), 0, 1), the IoU of iou_loss_device.h (true geometry, z = centre; a bad row -- a
//             non-finite number, a size <= 0, e.g. an exp that overflowed -- has IoU 0).  t is a constant of the loss.
//   bce     = max(z, 0) - z t + log1p(exp(-|z|)),  d bce / dz = sigmoid(z) - t      (the expressions of loss_device.h for a soft t)
#pragma once
#include "iou_loss_device.h"

namespace v3d {

// residual d[7] against anchor an[7] -> box[7], relative to the anchor's centre
V3D_HD void ih_decode_rel(const float* d, const float* an, float* box) {
  const float diag = sqrtf(an[3] * an[3] + an[4] * an[4]);
  box[0] = d[0] * diag;
  box[1] = d[1] * diag;
  box[2] = d[2] * an[5];
  box[3] = expf(d[3]) * an[3];
  box[4] = expf(d[4]) * an[4];
  box[5] = expf(d[5]) * an[5];
  box[6] = d[6] + an[6];
}

// The IoU target of one positive anchor: p = predicted residuals, gt = G_reg, an = the anchor; P, Q = the clipper's work space.
template <class A>
V3D_HD float ih_target(const float* p, const float* gt, const float* an, A P, A Q) {
  float a[7], b[7], da[7], db[7], term, iou;
  ih_decode_rel(p, an, a);
  ih_decode_rel(gt, an, b);
  iou3d_loss_pair(a, b, V3D_IOU_LOSS_IOU, P, Q, term, iou, da, db);
  return fminf(fmaxf(iou, 0.f), 1.f);
}

V3D_HD float ih_target_local(const float* p, const float* gt, const float* an) {
  P2 u[V3D_IOU_LOSS_POLY], v[V3D_IOU_LOSS_POLY];
  return ih_target(p, gt, an, P2View<1>{u}, P2View<1>{v});
}

// `slab` = the wave's slab (2 * 8 * 64 points) + this lane's index
V3D_HD float ih_target_lds(const float* p, const float* gt, const float* an, P2* slab) {
  return ih_target(p, gt, an, P2View<64>{slab}, P2View<64>{slab + V3D_IOU_LOSS_POLY * 64});
}

// soft-target BCE-with-logits of the logit z against t in [0, 1] -> the value; grad = sigmoid(z) - t
V3D_HD float ih_soft_bce(float z, float t, float& grad) {
  const float e = expf(-fabsf(z));
  const float prob = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  grad = prob - t;
  return fmaxf(z, 0.f) - z * t + log1pf(e);
}

}  // namespace v3d
