// voxel_pool.hip -- voxel RoI pooling for PV-RCNN's stage 2 (the pooling of Voxel R-CNN, arXiv 2012.15712; opt-in: cfg.VOXELPOOL): the
// regular grid points of every RoI query the sparse backbone's own voxels by integer coordinates, and a small PointNet pools the
// voxels found -- no keypoints, no furthest-point sampling, no set abstraction.  Upstream has no statement of it: the definition is
// this repository's (detector/voxel_roi_pool.py in torch, tests/voxel_roi_pool_ref.py in numpy float64).
//
// v3d_voxel_query: one level.  The coordinate hash of the level's active sites is built in the workspace (v3d_i_hash_build: sized by
//   the capacity, the live row count stays in device memory -- no host read, the call can be captured), then a WAVE per grid point
//   walks the point's index window in scan order, 64 candidates at a time: lane = candidate, one hash probe each (a latency-bound
//   gather: 75 or 125 probes per point, all of a round in flight at once), hit = active site of the RoI's own frame with
//   |centre - p|^2 < r^2 in fp32; a ballot and a popcount below the lane give the hit's rank in scan order, so the first NSAMPLE hits
//   are taken whatever the hash's insertion order was.  Four points per workgroup; nothing is shared between the waves (no LDS, no
//   barrier), so the occupancy is bounded by registers alone and the chip hides the probe latency with waves.
// v3d_voxel_pool_pair: the shared two-layer MLP of a level and the max over the slots in one launch, a wave per grid point.  The
//   first layer's feature part P = feat @ W1[3:] comes from the caller, once per ACTIVE VOXEL (v3d_linear_rows); lane = (slot, column
//   quarter) rebuilds h = relu(P[u] + (centre(u) - p) . W1[0:3] + b1) of its slot value by value and multiplies it with its quarter of the
//   second layer's weight (LDS, broadcast reads), and a butterfly over the 16 lanes of a quarter takes the max.  Plain fp32 fmaf chains
//   in index order (K <= 64): bit-repeatable.  354 MFLOP per level at 21 600 points: the launch is bound by the gather of P, not by
//   arithmetic, which is why the matrix cores are not used here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/vision3d_hip.h"
#include "rb_device.h"

#define VP_WAVES (V3D_BLOCK / V3D_WAVE)  // grid points of one workgroup
#define VP_MAX_ROWS (1 << 22)            // B * n_roi * G^3
#define VP_MAX_NSAMPLE 64                // the padding slots are written by one round of lanes
#define VP_MAX_RANGE 7                   // half-width of the index window per axis

struct VpGeom {
  int shape[3];                       // D, H, W of the level
  float size[3], off[3], half[3];     // x, y, z: voxel size of the level (base * stride, rounded once on the host), grid origin, size / 2
  int wz, wy, wx, rz, ry, rx;         // window widths (2 r + 1) and half-widths
  float r2;
};

__device__ __forceinline__ int vp_home(float p, float off, float size) {
  const float f = floorf((p - off) / size);
  return (int)fminf(fmaxf(f, -1073741824.f), 1073741824.f);  // (a point far outside, or NaN: no candidate lies inside the shape)
}

__global__ __launch_bounds__(V3D_BLOCK) void voxel_query_kernel(const float* __restrict__ points, int rows, int rows_per_frame,
                                                                const V3dHash h, const VpGeom g, int ns, int* __restrict__ idx,
                                                                unsigned char* __restrict__ empty) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * VP_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;  // (wave-uniform; no barrier below)
  const int b = row / rows_per_frame;
  const float px = points[3 * (size_t)row], py = points[3 * (size_t)row + 1], pz = points[3 * (size_t)row + 2];
  const int vx = vp_home(px, g.off[0], g.size[0]), vy = vp_home(py, g.off[1], g.size[1]), vz = vp_home(pz, g.off[2], g.size[2]);
  const int nwin = g.wz * g.wy * g.wx;
  int* out = idx + (size_t)row * ns;
  int base = 0, first = -1;
  for (int c0 = 0; c0 < nwin && base < ns; c0 += V3D_WAVE) {
    const int c = c0 + lane;
    const int z = vz + c / (g.wy * g.wx) - g.rz, y = vy + (c / g.wx) % g.wy - g.ry, x = vx + c % g.wx - g.rx;
    int r = -1;
    if (c < nwin && (unsigned)b < (unsigned)RB_MAX_BATCH && z >= 0 && z < g.shape[0] && y >= 0 && y < g.shape[1] && x >= 0 && x < g.shape[2])
      r = v3d_site_find_row(h, rb_key(b, z, y, x, g.shape));
    bool hit = false;
    if (r >= 0) {
      const float dx = (((float)x * g.size[0] + g.off[0]) + g.half[0]) - px;
      const float dy = (((float)y * g.size[1] + g.off[1]) + g.half[1]) - py;
      const float dz = (((float)z * g.size[2] + g.off[2]) + g.half[2]) - pz;
      hit = (dx * dx + dy * dy) + dz * dz < g.r2;
    }
    const unsigned long long m = __ballot(hit);
    const int rank = base + __popcll(m & ((1ull << lane) - 1ull));
    if (hit && rank < ns) out[rank] = r;
    if (base == 0 && m != 0ull) first = __shfl(r, __ffsll((long long)m) - 1);
    base += __popcll(m);
  }
  for (int s = min(base, ns) + lane; s < ns; s += V3D_WAVE) out[s] = first;  // fewer hits than slots: the first hit again; none: -1
  if (lane == 0) empty[row] = base == 0;
}

// lane = quarter * 16 + slot: the slot's hidden row in registers, NOUT / 4 output columns per lane
template <int K1, int NOUT>
__global__ __launch_bounds__(V3D_BLOCK) void voxel_pool_pair_kernel(const float* __restrict__ P, int ldp, const int4* __restrict__ coords,
                                                                    int cap, const float* __restrict__ points, const int* __restrict__ idx,
                                                                    int rows, int ns, const VpGeom g, const float* __restrict__ wx,
                                                                    const float* __restrict__ b1, const float* __restrict__ W,
                                                                    const float* __restrict__ bias, float* __restrict__ out, int ldo) {
  constexpr int NJ = NOUT / 4;
  __shared__ float sW[K1 * NOUT];
  __shared__ float sX[4 * K1];  // rows x, y, z of the first layer's weight, then its bias
  __shared__ float sB[NOUT];
  for (int e = threadIdx.x; e < K1 * NOUT; e += V3D_BLOCK) sW[e] = W[e];
  for (int e = threadIdx.x; e < 4 * K1; e += V3D_BLOCK) sX[e] = e < 3 * K1 ? wx[e] : b1[e - 3 * K1];
  for (int e = threadIdx.x; e < NOUT; e += V3D_BLOCK) sB[e] = bias[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, slot = lane & 15, quarter = lane >> 4;
  const int row = blockIdx.x * VP_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;  // (wave-uniform; no barrier below)
  const int* ix = idx + (size_t)row * ns;
  float* o = out + (size_t)row * ldo;
  if (ix[0] < 0) {  // an empty point pools to exact zeros
    for (int j = lane; j < NOUT; j += V3D_WAVE) o[j] = 0.f;
    return;
  }
  const float px = points[3 * (size_t)row], py = points[3 * (size_t)row + 1], pz = points[3 * (size_t)row + 2];
  float best[NJ];
#pragma unroll
  for (int j = 0; j < NJ; j++) best[j] = 0.f;  // (behind a ReLU: nothing is below 0)
  for (int s = slot; s < ns; s += 16) {
    const int u = ix[s];
    if ((unsigned)u >= (unsigned)cap) continue;
    const int4 c = coords[u];
    const float rx = (((float)c.w * g.size[0] + g.off[0]) + g.half[0]) - px;
    const float ry = (((float)c.z * g.size[1] + g.off[1]) + g.half[1]) - py;
    const float rz = (((float)c.y * g.size[2] + g.off[2]) + g.half[2]) - pz;
    const float* p = P + (size_t)u * ldp;
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < K1; k += 4) {
      const float4 p4 = *reinterpret_cast<const float4*>(p + k);
      const float pv[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const float h = fmaxf(pv[q] + ((rx * sX[k + q] + ry * sX[K1 + k + q]) + rz * sX[2 * K1 + k + q]) + sX[3 * K1 + k + q], 0.f);
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[j] = fmaf(h, sW[(k + q) * NOUT + quarter * NJ + j], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) best[j] = fmaxf(best[j], acc[j] + sB[quarter * NJ + j]);
  }
#pragma unroll
  for (int j = 0; j < NJ; j++) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) best[j] = fmaxf(best[j], __shfl_xor(best[j], off));
    if (slot == 0) o[quarter * NJ + j] = best[j];
  }
}

static int vp_geom(VpGeom& g, const int32_t* shape, const float* scale, const float* offset, const int32_t* range, float radius) {
  if (!shape || !scale || !offset) return V3D_EINVAL;
  for (int j = 0; j < 3; j++) {
    g.shape[j] = shape[j];
    g.size[j] = scale[j];
    g.off[j] = offset[j];
    g.half[j] = 0.5f * scale[j];
    if (shape[j] < 1 || !(scale[j] > 0.f)) return V3D_EINVAL;
  }
  if ((long long)shape[0] * shape[1] * shape[2] >= (1ll << 34)) return V3D_EUNSUPPORTED;  // (the key bits of a site table: rb_device.h)
  g.rz = range ? range[0] : 0;
  g.ry = range ? range[1] : 0;
  g.rx = range ? range[2] : 0;
  if (g.rz < 0 || g.ry < 0 || g.rx < 0) return V3D_EINVAL;
  if (g.rz > VP_MAX_RANGE || g.ry > VP_MAX_RANGE || g.rx > VP_MAX_RANGE) return V3D_EUNSUPPORTED;
  g.wz = 2 * g.rz + 1;
  g.wy = 2 * g.ry + 1;
  g.wx = 2 * g.rx + 1;
  g.r2 = radius * radius;
  return V3D_OK;
}

extern "C" size_t v3d_voxel_query_workspace(int cap) {
  if (cap < 0) return 0;
  const size_t hcap = v3d_hash_capacity(cap);
  return v3d_align(hcap * 8) + v3d_align(hcap * 4);
}

extern "C" int v3d_voxel_query(const float* points, int rows, int rows_per_frame, const int32_t* coords, const int32_t* n, int cap,
                               const int32_t* shape_host, const float* scale_host, const float* offset_host, const int32_t* range_host,
                               float radius, int nsample, int32_t* idx, uint8_t* empty, void* workspace, size_t workspace_bytes,
                               v3d_stream_t stream) {
  if (rows < 0 || rows_per_frame < 1 || cap < 0 || nsample < 1 || !range_host || !(radius > 0.f)) return V3D_EINVAL;
  if (rows > VP_MAX_ROWS || nsample > VP_MAX_NSAMPLE || cap > V3D_SITE_MAX_ROWS) return V3D_EUNSUPPORTED;
  VpGeom g;
  int rc = vp_geom(g, shape_host, scale_host, offset_host, range_host, radius);
  if (rc) return rc;
  if (rows == 0) return V3D_OK;
  if (!points || !idx || !empty || !workspace || (cap > 0 && (!coords || !n))) return V3D_EINVAL;
  if ((uintptr_t)coords & 15) return V3D_EINVAL;
  if (workspace_bytes < v3d_voxel_query_workspace(cap)) return V3D_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned hcap = v3d_hash_capacity(cap);
  V3dArena arena(workspace, workspace_bytes);
  V3dRbHash hash;
  hash.keys = arena.take<v3d_key_t>(hcap);
  hash.vals = arena.take<int>(hcap);
  hash.hcap = hcap;
  if (!arena.ok()) return V3D_EWORKSPACE;
  if (cap > 0) {
    rc = v3d_i_hash_build(coords, n, cap, g.shape, hash, 1, st);
    if (rc) return rc;
  } else {
    V3D_CHECK_HIP(v3d_fill_async(hash.keys, 0xFF, (size_t)hcap * 8, st));  // a level without rows: every probe misses
  }
  hipLaunchKernelGGL(voxel_query_kernel, dim3(v3d_ceil_div(rows, VP_WAVES)), dim3(V3D_BLOCK), 0, st, points, rows, rows_per_frame,
                     v3d_make_hash(hash.keys, hcap), g, nsample, idx, empty);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

template <int K1, int NOUT>
static int vp_launch_pair(const float* P, int ldp, const int32_t* coords, int cap, const float* points, const int32_t* idx, int rows, int ns,
                          const VpGeom& g, const float* wx, const float* b1, const float* W, const float* bias, float* out, int ldo,
                          hipStream_t st) {
  hipLaunchKernelGGL((voxel_pool_pair_kernel<K1, NOUT>), dim3(v3d_ceil_div(rows, VP_WAVES)), dim3(V3D_BLOCK), 0, st, P, ldp,
                     (const int4*)coords, cap, points, idx, rows, ns, g, wx, b1, W, bias, out, ldo);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_voxel_pool_pair(const float* P, int ldp, const int32_t* coords, int cap, const float* points, const int32_t* idx,
                                   int rows, int nsample, const float* scale_host, const float* offset_host, int K1, const float* wx,
                                   const float* b1, const float* W, const float* bias, int Nout, float* out, int ldo,
                                   v3d_stream_t stream) {
  if (rows < 0 || cap < 0 || nsample < 1 || ldp < K1 || (ldp & 3) || ldo < Nout) return V3D_EINVAL;
  if (rows > VP_MAX_ROWS || nsample > VP_MAX_NSAMPLE) return V3D_EUNSUPPORTED;
  const int32_t ones[3] = {1, 1, 1};
  VpGeom g;
  int rc = vp_geom(g, ones, scale_host, offset_host, nullptr, 1.f);
  if (rc) return rc;
  if (rows == 0) return V3D_OK;
  if (!points || !idx || !wx || !b1 || !W || !bias || !out || (cap > 0 && (!P || !coords))) return V3D_EINVAL;
  if (((uintptr_t)P & 15) || ((uintptr_t)coords & 15)) return V3D_EINVAL;  // 16-byte loads
  hipStream_t st = (hipStream_t)stream;
#define VP_CASE(k, n) \
  if (K1 == k && Nout == n) return vp_launch_pair<k, n>(P, ldp, coords, cap, points, idx, rows, nsample, g, wx, b1, W, bias, out, ldo, st)
  VP_CASE(16, 16);
  VP_CASE(16, 32);
  VP_CASE(32, 16);
  VP_CASE(32, 32);
  VP_CASE(32, 64);
  VP_CASE(64, 32);
  VP_CASE(64, 64);
#undef VP_CASE
  return V3D_EUNSUPPORTED;
}
