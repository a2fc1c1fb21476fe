// Host-side compile of vision3d_amd/csrc/box_vote_device.h + rotated_iou.h (the per-pair and per-centre expressions of IoU-weighted
// box voting) so that the CPU test-suite can check them against tests/box_voting_ref.py without a GPU.  Test infrastructure only.
#include <cstddef>
#include "../../vision3d_amd/csrc/box_vote_device.h"

// boxes (G, T, 7), scores (G, T) -> iou (G, T, T) with iou[g, k, j] = IoU(centre k, candidate j) for EVERY pair (also the pairs the
// vote does not ask for: the float64 restatement is fed this matrix), out (G, T, 7) = every candidate voted as a centre, the sums in
// candidate order.  strided != 0: the clipper's work arrays lane-interleaved in a 64-lane slab, as the kernel keeps them in LDS; must
// equal the plain form bit for bit.
extern "C" void host_box_voting(const float* boxes, const float* scores, int G, int T, float iou_threshold, int strided, float* iou,
                                float* out) {
  static v3d::P2 pts[24 * 64];
  static float dist[24 * 64];
  for (int g = 0; g < G; g++) {
    const float* gb = boxes + (size_t)g * T * 7;
    const float* gs = scores + (size_t)g * T;
    for (int k = 0; k < T; k++) {
      const float* centre = gb + (size_t)k * 7;
      const v3d::BoxPrep ck = v3d::bv_prep(centre);
      float acc[V3D_VOTE_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < T; j++) {
        const float* b = gb + (size_t)j * 7;
        const float u = strided ? v3d::bv_iou_lds(ck, b, pts + (j & 63), dist + (j & 63)) : v3d::bv_iou_local(ck, b);
        iou[((size_t)g * T + k) * T + j] = u;
        if (v3d::bv_member(v3d::bv_candidate(b, gs[j]), u, iou_threshold)) v3d::bv_accumulate(centre, b, v3d::bv_weight(gs[j], u), acc);
      }
      v3d::bv_finish(centre, acc, out + ((size_t)g * T + k) * 7);
    }
  }
}

// the IoU of the operator itself on the same pairs, without the vote's shortcut around the trigonometry: iou_prepped(prep(k), prep(j))
extern "C" void host_box_voting_plain_iou(const float* boxes, int G, int T, float* iou) {
  for (int g = 0; g < G; g++)
    for (int k = 0; k < T; k++)
      for (int j = 0; j < T; j++) {
        const v3d::BoxPrep a = v3d::bv_prep(boxes + ((size_t)g * T + k) * 7), b = v3d::bv_prep(boxes + ((size_t)g * T + j) * 7);
        iou[((size_t)g * T + k) * T + j] = v3d::iou_prepped(a, b);
      }
}
