// object_noise.hip -- per-object ground-truth noise of B training frames in TWO launches (VoxelNet 3.1 / SECOND's object noise).
//
// Replaces nothing upstream: vision3d/dataset/augmentation.py has GT sampling and the global flip / scale / rotation, not this.
// The definition is the repository's own (restated in float64 by tests/object_noise_ref.py):
//   inputs per frame   points (N, C >= 3) f32, boxes (n, 7) f32 = (x, y, z, w, l, h, yaw), the caller's draws trans (n, T, 3) f32 and
//                      rot (n, T) f32 (host draws, like every draw of the package).
//   candidate (i, t)   centre (x_i + trans[i,t,0], y_i + trans[i,t,1]), yaw_i + rot[i,t] -- one fp32 add each --, size unchanged.
//   collision          the rotated-IoU operator of v3d_box_iou_rotated (the same device function, candidate = first argument) on
//                      (x, y, w, l, yaw_deg), yaw_deg = yaw * 57.29577951308232f (one fp32 multiply, not contracted), compared
//                      > collision_iou.  True geometry: the radians-read-as-degrees quirk is kept where the reference
//                      has a call site to match; there is none here.
//   selection          sequentially in box order: chosen[i] = the smallest t whose candidate collides with no box j != i, box j at
//                      its already moved pose for j < i and at its original pose for j > i; none: chosen[i] = -1, the box stays.
//   output boxes       the chosen candidate's x, y, yaw and z_i + trans[i,t,2]; chosen = -1: copied bit for bit.
//   points             a point belongs to the lowest-index box whose inside test passes -- the test of v3d_points_in_boxes(use_z = 1)
//                      on the ORIGINAL boxes (pib_device.h, same bits).  With (c, s) = (cosf, sinf)(rot[i,t]), taken once per box,
//                      and (cx, cy) the original centre, in fp32 and uncontracted:
//                          dx = x - cx, dy = y - cy;  x' = ((dx * c - dy * s) + cx) + trans_x;  y' = ((dx * s + dy * c) + cy) + trans_y;
//                          z' = z + trans_z.   Columns >= 3 and every other point are copied; row order and count are unchanged.
//   not done           scene points that lie where a box lands stay; a box may leave the grid bounds.
//
// on_select_kernel: one workgroup per frame -- the sequence over i is a true dependency.  All n * T candidates are prepared first
// (x, y and the half-extent cosines of rotated_iou.h: one double cos / sin per candidate, n * T / 512 per lane, where evaluating them
// inside the rounds would cost every lane one per round) into the caller's workspace.  Then, for box i, the tries are examined in
// ascending chunks; lanes = (try in chunk) x (other box j), lane -> j fixed for the whole kernel, so each lane keeps the CURRENT pose
// of its box j in registers and nothing but the collision flags crosses lanes.  A colliding lane raises its try's flag in LDS (plain
// stores of the same 1: no atomic decides anything), one barrier, every wave reads the chunk's flags with one ballot and takes the
// lowest free try.  The flag rows rotate through three buffers so that clearing the next one needs no second barrier.
// The chunk size (tries per round) only sets how many tries are looked at together: chunks ascend and the first chunk holding a free
// try yields its smallest, which is the smallest free try overall -- the result does not depend on the chunk size.
// The clipper's work arrays take 18 KB of LDS per wave (24 * 64 points + distances): 8 waves = 144 KB of the CU's 160 KB, plus the
// staged boxes and the flags -- that, not the 1 024-thread limit, sizes the workgroup.
// on_points_kernel: grid over the points of all frames; the frame's boxes (corners, centre, cos / sin / translation of the chosen
// try) sit in LDS; C == 4 rows move whole when 16-byte aligned.
#include "v3d_common.h"
#include "rotated_iou.h"
#include "pib_device.h"

using v3d::BoxPrep;

#define ON_MAX_BOXES 128
#define ON_MAX_TRIES 256
#define ON_MAX_FRAMES 64
#define ON_WAVES 8
#define ON_THREADS (ON_WAVES * V3D_WAVE)
#define ON_CHUNK 64  // most tries per round: their flags are read with one ballot
#define ON_CLIP (24 * 64)
#define ON_SEL_SMEM (ON_WAVES * ON_CLIP * (int)(sizeof(v3d::P2) + sizeof(float)) + ON_MAX_BOXES * 7 * 4 + 3 * ON_CHUNK * 4)

struct OnFrames {  // host offsets, passed by value: first point row / first box / first point block of each frame
  int pt[ON_MAX_FRAMES + 1], bx[ON_MAX_FRAMES + 1], blk[ON_MAX_FRAMES + 1];
  int B;
};

__global__ __launch_bounds__(ON_THREADS) void on_select_kernel(const float* __restrict__ boxes, const OnFrames fr,
                                                               const float* __restrict__ trans, const float* __restrict__ rot, int T,
                                                               float thr, float4* cand, float* __restrict__ out_boxes,
                                                               int* __restrict__ chosen) {
  extern __shared__ __attribute__((aligned(16))) unsigned char on_smem[];
  v3d::P2* clip_pts = reinterpret_cast<v3d::P2*>(on_smem);              // [ON_WAVES][ON_CLIP]
  float* clip_dist = reinterpret_cast<float*>(clip_pts + ON_WAVES * ON_CLIP);  // [ON_WAVES][ON_CLIP]
  float* sbox = clip_dist + ON_WAVES * ON_CLIP;                         // [ON_MAX_BOXES][7]
  int* coll = reinterpret_cast<int*>(sbox + ON_MAX_BOXES * 7);          // [3][ON_CHUNK]
  const int tid = threadIdx.x, lane = tid & 63;
  const int b0 = fr.bx[blockIdx.x], n = fr.bx[blockIdx.x + 1] - b0;
  if (n <= 0) return;
  for (int k = tid; k < 7 * n; k += ON_THREADS) sbox[k] = boxes[7 * (size_t)b0 + k];
  for (int k = tid; k < 3 * ON_CHUNK; k += ON_THREADS) coll[k] = 0;
  // ---- every candidate, prepared once: (x, y, cos / 2, sin / 2)
  for (int q = tid; q < n * T; q += ON_THREADS) {
    const size_t g = (size_t)b0 * T + q;
    const float* bx = boxes + 7 * (size_t)(b0 + q / T);
    const float yaw = bx[6] + rot[g];
    const float deg = yaw * 57.29577951308232f;
    float c2, s2;
    v3d::half_trig(deg, c2, s2);
    cand[g] = make_float4(bx[0] + trans[3 * g], bx[1] + trans[3 * g + 1], c2, s2);
  }
  __syncthreads();
  // ---- lane -> (try in chunk, other box j); the lane's box j at its current pose
  const int chunk = min(ON_CHUNK, ON_THREADS / n);  // >= 4
  const int tl = tid / n, j = tid - tl * n;
  const bool active = tl < chunk;
  BoxPrep cur;
  {
    const float* bj = sbox + 7 * j;
    const float bev[5] = {bj[0], bj[1], bj[3], bj[4], bj[6] * 57.29577951308232f};
    cur = v3d::prep_box(bev);
  }
  v3d::P2* pts = clip_pts + (tid >> 6) * ON_CLIP + lane;
  float* dist = clip_dist + (tid >> 6) * ON_CLIP + lane;
  int round = 0;
  for (int i = 0; i < n; i++) {
    const float* bi = sbox + 7 * i;
    const float4* ci = cand + (size_t)(b0 + i) * T;
    BoxPrep a;
    a.w = bi[3], a.h = bi[4], a.area = bi[3] * bi[4];
    int pick = -1;
    for (int t0 = 0; t0 < T; t0 += chunk, round++) {
      int* flags = coll + (round % 3) * ON_CHUNK;
      if (tid < ON_CHUNK) coll[((round + 1) % 3) * ON_CHUNK + tid] = 0;  // read last two barriers ago, raised after the next one
      if (active && j != i && t0 + tl < T) {
        const float4 c = ci[t0 + tl];
        a.x = c.x, a.y = c.y, a.c2 = c.z, a.s2 = c.w;
        if (v3d::iou_prepped_lds(a, cur, pts, dist) > thr) flags[tl] = 1;
      }
      __syncthreads();
      int hit = 1;
      if (lane < chunk && t0 + lane < T) hit = flags[lane];
      const unsigned long long free_tries = __ballot(hit == 0);
      if (free_tries != 0ull) {  // (the same flags in every wave: uniform over the workgroup)
        pick = t0 + __ffsll((long long)free_tries) - 1;
        round++;
        break;
      }
    }
    if (pick >= 0 && j == i) {  // the lanes that hold box i: from here on it stands at its moved pose
      const float4 c = ci[pick];
      cur.x = c.x, cur.y = c.y, cur.c2 = c.z, cur.s2 = c.w;
    }
    if (tid == 0) {
      float* o = out_boxes + 7 * (size_t)(b0 + i);
      const size_t g = (size_t)(b0 + i) * T + (pick >= 0 ? pick : 0);
      chosen[b0 + i] = pick;
      o[0] = pick >= 0 ? ci[pick].x : bi[0];
      o[1] = pick >= 0 ? ci[pick].y : bi[1];
      o[2] = pick >= 0 ? bi[2] + trans[3 * g + 2] : bi[2];
      o[3] = bi[3], o[4] = bi[4], o[5] = bi[5];
      o[6] = pick >= 0 ? bi[6] + rot[g] : bi[6];
    }
  }
}

struct OnPointBox {
  PibBox pb;
  float cx, cy, c, s, tx, ty, tz;
  int moved;
};

__global__ __launch_bounds__(V3D_BLOCK) void on_points_kernel(const float* __restrict__ points, int C, const float* __restrict__ boxes,
                                                              const OnFrames fr, const float* __restrict__ trans,
                                                              const float* __restrict__ rot, int T, const int* __restrict__ chosen,
                                                              float* __restrict__ out_points, int rows4) {
  __shared__ OnPointBox sb[ON_MAX_BOXES];
  const int tid = threadIdx.x;
  int f = 0;
  while (f + 1 < fr.B && (int)blockIdx.x >= fr.blk[f + 1]) f++;
  const int b0 = fr.bx[f], n = fr.bx[f + 1] - b0;
  const int local = ((int)blockIdx.x - fr.blk[f]) * V3D_BLOCK + tid;
  const bool valid = local < fr.pt[f + 1] - fr.pt[f];
  if (tid < n) {
    const float* bx = boxes + 7 * (size_t)(b0 + tid);
    OnPointBox ob;
    ob.pb = pib_prep(bx);
    ob.cx = bx[0], ob.cy = bx[1];
    const int t = chosen[b0 + tid];
    ob.moved = t >= 0;
    const size_t g = (size_t)(b0 + tid) * T + (t >= 0 ? t : 0);
    const float r = rot[g];
    ob.c = cosf(r), ob.s = sinf(r);
    ob.tx = trans[3 * g], ob.ty = trans[3 * g + 1], ob.tz = trans[3 * g + 2];
    sb[tid] = ob;
  }
  __syncthreads();
  if (!valid) return;
  const size_t row = (size_t)fr.pt[f] + local;
  float x, y, z, w = 0.f;
  if (rows4) {
    const float4 p = reinterpret_cast<const float4*>(points)[row];
    x = p.x, y = p.y, z = p.z, w = p.w;
  } else {
    const float* p = points + row * C;
    x = p[0], y = p[1], z = p[2];
  }
  int owner = -1;
  for (int k = 0; k < n; k++) {
    if (pib_inside(sb[k].pb, x, y, z, true)) {
      owner = k;
      break;
    }
  }
  if (owner >= 0 && sb[owner].moved) {
    const OnPointBox& ob = sb[owner];
    const float dx = x - ob.cx, dy = y - ob.cy;
    const float rx = dx * ob.c - dy * ob.s, ry = dx * ob.s + dy * ob.c;
    x = (rx + ob.cx) + ob.tx;
    y = (ry + ob.cy) + ob.ty;
    z = z + ob.tz;
  }
  if (rows4) {
    reinterpret_cast<float4*>(out_points)[row] = make_float4(x, y, z, w);
  } else {
    const float* p = points + row * C;
    float* o = out_points + row * C;
    o[0] = x, o[1] = y, o[2] = z;
    for (int c = 3; c < C; c++) o[c] = p[c];
  }
}

extern "C" size_t v3d_object_noise_workspace(int n_boxes, int T) {
  if (n_boxes < 0 || T < 1) return 0;
  return v3d_align((size_t)(n_boxes > 0 ? n_boxes : 1) * T * sizeof(float4));
}

extern "C" int v3d_object_noise(const float* points, const int32_t* point_offsets_host, const float* boxes,
                                const int32_t* box_offsets_host, int B, int C, const float* trans, const float* rot, int T,
                                float collision_iou, float* out_points, float* out_boxes, int32_t* chosen, void* workspace,
                                size_t workspace_bytes, v3d_stream_t stream) {
  if (B < 0 || C < 3 || T < 1 || !point_offsets_host || !box_offsets_host) return V3D_EINVAL;
  if (B > ON_MAX_FRAMES || T > ON_MAX_TRIES) return V3D_EUNSUPPORTED;
  if (B == 0) return V3D_OK;
  if (point_offsets_host[0] < 0 || box_offsets_host[0] < 0) return V3D_EINVAL;
  OnFrames fr;
  fr.B = B;
  long long blocks = 0;
  for (int b = 0; b <= B; b++) {
    fr.pt[b] = point_offsets_host[b < B ? b : B];
    fr.bx[b] = box_offsets_host[b < B ? b : B];
    fr.blk[b] = (int)blocks;
    if (b == B) break;
    const long long np = (long long)point_offsets_host[b + 1] - point_offsets_host[b];
    const long long nb = (long long)box_offsets_host[b + 1] - box_offsets_host[b];
    if (np < 0 || nb < 0) return V3D_EINVAL;
    if (nb > ON_MAX_BOXES) return V3D_EUNSUPPORTED;
    blocks += (np + V3D_BLOCK - 1) / V3D_BLOCK;
    if (blocks > 0x7fffffffLL) return V3D_EUNSUPPORTED;
  }
  for (int b = B + 1; b <= ON_MAX_FRAMES; b++) fr.pt[b] = fr.pt[B], fr.bx[b] = fr.bx[B], fr.blk[b] = fr.blk[B];
  const int n_points = fr.pt[B], n_boxes = fr.bx[B];
  if ((n_points && (!points || !out_points)) || (n_boxes && (!boxes || !out_boxes || !chosen || !trans || !rot || !workspace)))
    return V3D_EINVAL;
  if (n_boxes && workspace_bytes < v3d_object_noise_workspace(n_boxes, T)) return V3D_EWORKSPACE;
  if (n_boxes && ((uintptr_t)workspace & 15)) return V3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (n_boxes) {
    static V3dPerDeviceFlag raised;
    V3D_CHECK_HIP(v3d_set_max_lds(raised, (const void*)on_select_kernel, ON_SEL_SMEM));
    hipLaunchKernelGGL(on_select_kernel, dim3(B), dim3(ON_THREADS), ON_SEL_SMEM, st, boxes, fr, trans, rot, T, collision_iou,
                       (float4*)workspace, out_boxes, (int*)chosen);
    V3D_CHECK_LAUNCH();
  }
  if (blocks) {
    const int rows4 = C == 4 && !((uintptr_t)points & 15) && !((uintptr_t)out_points & 15);
    hipLaunchKernelGGL(on_points_kernel, dim3((unsigned)blocks), dim3(V3D_BLOCK), 0, st, points, C, boxes, fr, trans, rot, T,
                       (const int*)chosen, out_points, rows4);
    V3D_CHECK_LAUNCH();
  }
  return V3D_OK;
}
