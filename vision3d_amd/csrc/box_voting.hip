// box_voting.hip -- IoU-weighted box voting (cfg.BOX_VOTING; box voting / weighted NMS / the DI-NMS of CIA-SSD) for gfx950.
//
// After greedy NMS the detectors that rank by an IoU-aware confidence do not throw the suppressed candidates away: a surviving box is
// replaced by the confidence- and IoU-weighted mean of the candidates of its (frame, class) group that overlap it.  The expressions
// are box_vote_device.h's (definition: DESIGN.md section 7); this file is the launch.  Upstream has no such step.
//
// Shape (wave64): one wave per centre, V3D_BLOCK / 64 centres per workgroup.  The lanes stride over the T candidates of the centre's
// group; each lane keeps W and the seven weighted offset sums in registers, one DPP reduction finishes them, lane 0 writes the seven
// floats.  The clipper's work arrays live in a per-wave LDS slab (rotated_iou.h: as locals they would be scratch): 24 * 64 * (8 + 4) B
// = 18 KB per wave, 72 KB per workgroup -- two workgroups share a CU's 160 KB, and the G * T <= 1024 centres of a fused tail are 256
// workgroups, one per CU.  Most pairs never reach the clipper: the centre-distance test (iou_needs_clip) rejects them before the
// candidate's sin / cos are evaluated.  Every centre is voted, survivors and suppressed candidates alike: the tails (proposal.hip)
// launch this beside the NMS, which then needs no map from a survivor back to its candidate row and no count.
#include "v3d_common.h"
#include "box_vote_device.h"
#include "dpp_device.h"
#include "v3d_internal.h"

#define VOTE_WAVES (V3D_BLOCK / V3D_WAVE)

__global__ __launch_bounds__(V3D_BLOCK) void box_vote_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             long long n_centres, int T, float iou, float* __restrict__ out) {
  __shared__ v3d::P2 clip_pts[VOTE_WAVES][24 * 64];
  __shared__ float clip_dist[VOTE_WAVES][24 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long k = (long long)blockIdx.x * VOTE_WAVES + wave;
  if (k >= n_centres) return;  // wave-uniform; no workgroup barrier below
  const long long first = k / T * T;  // row of the group's first candidate
  float centre[7];
#pragma unroll
  for (int c = 0; c < 7; c++) centre[c] = boxes[k * 7 + c];  // same address in every lane: one broadcast load
  const v3d::BoxPrep ck = v3d::bv_prep(centre);
  float acc[V3D_VOTE_SUMS];
#pragma unroll
  for (int c = 0; c < V3D_VOTE_SUMS; c++) acc[c] = 0.f;
  for (int j = lane; j < T; j += 64) {
    const long long row = first + j;
    float b[7];
#pragma unroll
    for (int c = 0; c < 7; c++) b[c] = boxes[row * 7 + c];
    const float s = scores[row];
    if (!v3d::bv_candidate(b, s)) continue;
    const float u = v3d::bv_iou_lds(ck, b, clip_pts[wave] + lane, clip_dist[wave] + lane);
    if (v3d::bv_member(true, u, iou)) v3d::bv_accumulate(centre, b, v3d::bv_weight(s, u), acc);
  }
  // (the lanes have converged again: the DPP steps read every lane of the wave)
#pragma unroll
  for (int c = 0; c < V3D_VOTE_SUMS; c++) acc[c] = v3d_dpp_sum_f32(acc[c]);
  if (lane == 0) {
    float r[7];
    v3d::bv_finish(centre, acc, r);
#pragma unroll
    for (int c = 0; c < 7; c++) out[k * 7 + c] = r[c];
  }
}

// boxes (G, T, 7), scores (G, T) -> out (G, T, 7): every candidate voted as a centre by the candidates of its own group.  No
// workspace, no host synchronisation.  The caller has checked the pointers.
int v3d_i_box_voting(const float* boxes, const float* scores, int G, int T, float iou, float* out, hipStream_t st) {
  if (G < 0 || T < 0) return V3D_EINVAL;
  const long long n = (long long)G * T;
  if (n == 0) return V3D_OK;
  if (n > (long long)0x7FFFFFFF) return V3D_EUNSUPPORTED;  // the grid's x extent, with VOTE_WAVES centres per workgroup to spare
  hipLaunchKernelGGL(box_vote_kernel, dim3((unsigned)((n + VOTE_WAVES - 1) / VOTE_WAVES)), dim3(V3D_BLOCK), 0, st, boxes, scores, n, T, iou,
                     out);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_box_voting(const float* boxes, const float* scores, int G, int T, float iou_threshold, float* out, v3d_stream_t stream) {
  if (G < 0 || T < 0) return V3D_EINVAL;
  if ((long long)G * T == 0) return V3D_OK;
  if (!boxes || !scores || !out || boxes == out) return V3D_EINVAL;  // (in place: a centre would read rows other waves have voted)
  return v3d_i_box_voting(boxes, scores, G, T, iou_threshold, out, (hipStream_t)stream);
}
