// box_vote_device.h -- the per-pair and per-centre expressions of IoU-weighted box voting behind the rotated NMS tails
// (cfg.BOX_VOTING; box voting / weighted NMS / the DI-NMS of CIA-SSD): which candidates of a (frame, class) group vote for a centre,
// with what weight, how a yaw difference is wrapped, and the final division with its "keep the centre" fallback.  fp32, one IEEE
// operation per operator as written; compiled by hipcc for the kernel (box_voting.hip) and by g++ for the CPU suite
// (tests/host/box_voting_host_shim.cpp).  The definition is this repository's; tests/box_voting_ref.py
// restates it in float64.
//
//   u_j     = box_iou_rotated(b_k[0,1,3,4,6], b_j[0,1,3,4,6])          centre first, on the unshifted boxes (rotated_iou.h: the bits
//             of v3d_box_iou_rotated, which reads the yaw the way that operator reads it)
//   member  : s_j > 0, the seven components of b_j finite, u_j >= iou  (a NaN on either side of a comparison: not a member)
//   w_j     = s_j * u_j,  W = sum of w_j over the members
//   out[c]  = b_k[c] + (sum of w_j (b_j[c] - b_k[c])) / W              c = 0 .. 5; the offset form keeps the digits at 70 m
//   out[6]  = yaw_k + (sum of w_j wrap(yaw_j - yaw_k)) / W,            wrap(d) = d - pi rint(d / pi), pi = (float)M_PI, round half even
//   W not finite or not > 0: out = b_k with its own bits
#pragma once
#include "rotated_iou.h"

namespace v3d {

#define V3D_VOTE_SUMS 8  // W and the seven weighted offset sums

V3D_HD bool bv_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // false for NaN and both infinities

// what of the membership test does not need the IoU: checked first, so that a sentinel row never reaches the clipper
V3D_HD bool bv_candidate(const float* b, float s) {
  bool ok = s > 0.f;
#pragma unroll
  for (int c = 0; c < 7; c++) ok = ok && bv_finite(b[c]);
  return ok;
}

V3D_HD bool bv_member(bool candidate, float u, float iou) { return candidate && u >= iou; }

V3D_HD float bv_weight(float s, float u) { return s * u; }

// the BEV rectangle of a 3-D box without its trigonometry (prep_box evaluates sin / cos in double: only pairs that pass the
// centre-distance test pay for it -- iou_needs_clip reads the centre, the size and the area)
V3D_HD BoxPrep bv_prep_flat(const float* b) {
  BoxPrep r;
  r.x = b[0];
  r.y = b[1];
  r.w = b[3];
  r.h = b[4];
  r.c2 = 0.f;
  r.s2 = 0.f;
  r.area = b[3] * b[4];
  return r;
}

V3D_HD BoxPrep bv_prep(const float* b) {
  const float bev[5] = {b[0], b[1], b[3], b[4], b[6]};
  return prep_box(bev);
}

// u_j of one pair: `centre` prepared once per centre (bv_prep), b = the candidate's seven components.  The value of
// iou_prepped(bv_prep(centre), bv_prep(b)) bit for bit -- a pair the centre-distance test rejects has IoU +0.0f there too.
V3D_HD float bv_iou_local(const BoxPrep& centre, const float* b) {
  BoxPrep bc = bv_prep_flat(b);
  if (!iou_needs_clip(centre, bc)) return 0.f;
  half_trig(b[6], bc.c2, bc.s2);
  return iou_prepped(centre, bc);
}

// the same with the clipper's work arrays in a lane-interleaved slab (pts: 24 * 64 P2, dist: 24 * 64 floats, + this lane's index)
V3D_HD float bv_iou_lds(const BoxPrep& centre, const float* b, P2* pts, float* dist) {
  BoxPrep bc = bv_prep_flat(b);
  if (!iou_needs_clip(centre, bc)) return 0.f;
  half_trig(b[6], bc.c2, bc.s2);
  return iou_prepped_lds(centre, bc, pts, dist);
}

// a yaw difference to its representative nearest zero modulo pi: a candidate turned by pi is the same rectangle and pulls nothing
V3D_HD float bv_wrap_yaw(float d) {
  const float pi = 3.14159274101257324f;  // (float)M_PI
  return d - pi * rintf(d / pi);
}

// one member's terms added to acc[V3D_VOTE_SUMS] = {W, sums of w * offset}
V3D_HD void bv_accumulate(const float* centre, const float* b, float w, float* acc) {
  acc[0] += w;
#pragma unroll
  for (int c = 0; c < 6; c++) acc[1 + c] += w * (b[c] - centre[c]);
  acc[7] += w * bv_wrap_yaw(b[6] - centre[6]);
}

// the voted box of a centre from the finished sums
V3D_HD void bv_finish(const float* centre, const float* acc, float* out) {
  const float W = acc[0];
  const bool vote = bv_finite(W) && W > 0.f;
#pragma unroll
  for (int c = 0; c < 7; c++) out[c] = vote ? centre[c] + acc[1 + c] / W : centre[c];
}

}  // namespace v3d
