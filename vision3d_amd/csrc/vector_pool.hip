// vector_pool.hip -- VectorPool aggregation of PV-RCNN++ (arXiv 2102.00463; opt-in: cfg.VECTORPOOL): the space around a query is cut
// into vx * vy * vz sub-voxels, the three nearest support points of every sub-voxel CENTRE are interpolated into one row per
// sub-voxel, and every sub-voxel multiplies its row with a weight of its own.  Upstream has no statement of it: the definition is this
// repository's (detector/vector_pool.py in torch, tests/vector_pool_ref.py in numpy float64).
//
// v3d_vector_pool_query: the support points of every frame are binned into (x, y) cells by the shared builder (cell_grid.hip; layout
//   and shape rule: cell_grid_device.h) with cells no smaller than the reach R (2 - 1 / max(vx, vy)) and no index chunks: one launch,
//   no host read.  A WAVE per query then walks the cell rows its reach touches, keeps the records inside the reach box in LDS (ballot
//   compaction, VPQ_STAGE at a time) and one LANE per sub-voxel centre inserts the staged candidates into its sorted list of three.
//   The list is ordered by (d^2, row index) and holds one row per set of bit-equal coordinates (the lowest index), so it is the same
//   whatever order the candidates arrive in: the scatter's atomics place the records of a cell, they decide no result.
// v3d_vector_pool_embed: a workgroup per (block of queries, sub-voxel): the sub-voxel's weight (Cr + 9, CL) and shift in LDS, the
//   rows [sum_k w_k fr[idx_k] | c - p_1 | c - p_2 | c - p_3] of 256 / CL queries at a time built in LDS, then a thread per (query,
//   column): an fmaf chain over the row in index order, + shift, ReLU, written into the sub-voxel's column block.
// v3d_vector_pool_reduce: fr[n, j] = sum_m feat[n, m * Cr + j], m ascending, a thread per value.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/vision3d_hip.h"
#include "v3d_internal.h"
#include "cell_grid_device.h"

#define VPQ_MAX_AXIS 3         // sub-voxels per axis
#define VPQ_MAX_NV 27
#define VPQ_MAX_B 64
#define VPQ_MAX_N (1 << 20)    // support rows of a frame
#define VPQ_MAX_BN (1 << 24)   // support rows of a call
#define VPQ_MAX_CENTRES (1 << 22)
#define VPQ_STAGE 512          // staged candidates of a wave
#define VPQ_WAVES (V3D_BLOCK / V3D_WAVE)
#define VPE_MAX_CR 32
#define VPE_MAX_K (VPE_MAX_CR + 9)

struct VpqOffsets {
  float o[VPQ_MAX_NV][3];  // sub-voxel centre offsets: computed in double on the host, rounded once
};

// the sorted list of three of one centre: (d, i) ascending, empty slots (inf, INT_MAX); x / y / z bits of the chosen rows
struct VpqTop {
  float d0, d1, d2;
  int i0, i1, i2;
  int x0, y0, z0, x1, y1, z1, x2, y2, z2;
};

__device__ __forceinline__ bool vpq_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

#define VPQ_SWAP(a, b) \
  {                    \
    auto t_ = a;       \
    a = b;             \
    b = t_;            \
  }
#define VPQ_SWAP_SLOTS(A, B)                                                                        \
  {                                                                                                 \
    VPQ_SWAP(t.d##A, t.d##B) VPQ_SWAP(t.i##A, t.i##B) VPQ_SWAP(t.x##A, t.x##B) VPQ_SWAP(t.y##A, t.y##B) \
    VPQ_SWAP(t.z##A, t.z##B)                                                                        \
  }

__device__ __forceinline__ void vpq_insert(VpqTop& t, float d, int i, int xb, int yb, int zb) {
  // a row with the coordinates of a listed one (the same d^2): the lower index stays, and moves up among equal distances
  if (t.x0 == xb && t.y0 == yb && t.z0 == zb && t.i0 != INT_MAX) {
    t.i0 = min(t.i0, i);
    return;
  }
  if (t.x1 == xb && t.y1 == yb && t.z1 == zb && t.i1 != INT_MAX) {
    t.i1 = min(t.i1, i);
    if (vpq_less(t.d1, t.i1, t.d0, t.i0)) VPQ_SWAP_SLOTS(0, 1)
    return;
  }
  if (t.x2 == xb && t.y2 == yb && t.z2 == zb && t.i2 != INT_MAX) {
    t.i2 = min(t.i2, i);
    if (vpq_less(t.d2, t.i2, t.d1, t.i1)) VPQ_SWAP_SLOTS(1, 2)
    if (vpq_less(t.d1, t.i1, t.d0, t.i0)) VPQ_SWAP_SLOTS(0, 1)
    return;
  }
  if (!vpq_less(d, i, t.d2, t.i2)) return;
  t.d2 = d, t.i2 = i, t.x2 = xb, t.y2 = yb, t.z2 = zb;
  if (vpq_less(t.d2, t.i2, t.d1, t.i1)) VPQ_SWAP_SLOTS(1, 2)
  if (vpq_less(t.d1, t.i1, t.d0, t.i0)) VPQ_SWAP_SLOTS(0, 1)
}

__global__ __launch_bounds__(V3D_BLOCK) void vpq_query_kernel(const float* __restrict__ new_xyz, int rows, int M, int N, int nv,
                                                              const VpqOffsets offs, float reach_x, float reach_y, float reach_z,
                                                              float r2, const unsigned char* __restrict__ ws /*B frames of cg_frame_bytes(N)*/,
                                                              int* __restrict__ idx, float* __restrict__ w) {
  __shared__ float4 stage[VPQ_WAVES][VPQ_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * VPQ_WAVES + wave;
  if (row >= rows) return;  // (wave-uniform; the LDS stage is a wave's own: no barrier below)
  const int b = row / M;
  const float qx = new_xyz[3 * (size_t)row], qy = new_xyz[3 * (size_t)row + 1], qz = new_xyz[3 * (size_t)row + 2];
  const unsigned char* frame = ws + (size_t)b * cg_frame_bytes(N);
  CgHeader h = {};  // (N = 0: nothing was built, nx = 0)
  if (N > 0) h = *reinterpret_cast<const CgHeader*>(frame);
  const float inf = __builtin_inff();
  const int v = min(lane, nv - 1);
  const float cx = qx + offs.o[v][0], cy = qy + offs.o[v][1], cz = qz + offs.o[v][2];
  VpqTop t;
  t.d0 = t.d1 = t.d2 = inf;
  t.i0 = t.i1 = t.i2 = INT_MAX;
  t.x0 = t.y0 = t.z0 = t.x1 = t.y1 = t.z1 = t.x2 = t.y2 = t.z2 = 0;
  float4* st = stage[wave];
  int staged = 0;
  auto drain = [&]() {
    __builtin_amdgcn_wave_barrier();  // (the wave's own stage: its writes above are ordered before the reads below)
    if (lane < nv) {
      for (int s = 0; s < staged; s++) {
        const float4 p = st[s];  // (every lane reads the same word: a broadcast)
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < r2) vpq_insert(t, d, __float_as_int(p.w), __float_as_int(p.x), __float_as_int(p.y), __float_as_int(p.z));
      }
    }
    __builtin_amdgcn_wave_barrier();
    staged = 0;
  };
  const bool live = h.nx > 0 && fabsf(qx) < inf && fabsf(qy) < inf && fabsf(qz) < inf;
  if (live) {
    const float fx0 = cg_cell(qx - reach_x, h.x0, h.inv_c), fx1 = cg_cell(qx + reach_x, h.x0, h.inv_c);
    const float fy0 = cg_cell(qy - reach_y, h.y0, h.inv_c), fy1 = cg_cell(qy + reach_y, h.y0, h.inv_c);
    // (the window is clamped into the grid, which holds every point; a window that ends before the first cell holds no point: every
    // point lies at or above the frame's minimum)
    if (fx1 >= 0.f && fy1 >= 0.f) {
      const int x0 = (int)fminf(fmaxf(fx0, 0.f), (float)(h.nx - 1)), x1 = (int)fminf(fx1, (float)(h.nx - 1));
      const int y0 = (int)fminf(fmaxf(fy0, 0.f), (float)(h.ny - 1)), y1 = (int)fminf(fy1, (float)(h.ny - 1));
      const int* start = reinterpret_cast<const int*>(frame + CG_HEADER_BYTES);
      const float4* sorted = reinterpret_cast<const float4*>(frame + cg_record_offset());
      for (int y = y0; y <= y1; y++) {
        const int beg = start[y * h.nx + x0], end = min(start[y * h.nx + x1 + 1], N);  // the cells of a row lie back to back
        for (int r0 = beg; r0 < end; r0 += V3D_WAVE) {
          if (staged + V3D_WAVE > VPQ_STAGE) drain();
          const int r = r0 + lane;
          float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
          bool in = false;
          if (r < end) {
            p = sorted[r];
            in = fabsf(p.x - qx) <= reach_x && fabsf(p.y - qy) <= reach_y && fabsf(p.z - qz) <= reach_z;
          }
          const unsigned long long m = __ballot(in);
          if (in) st[staged + __popcll(m & ((1ull << lane) - 1ull))] = p;
          staged += __popcll(m);
        }
      }
      drain();
    }
  }
  if (lane < nv) {
    int* oi = idx + ((size_t)row * nv + lane) * 3;
    float* ow = w + ((size_t)row * nv + lane) * 3;
    const bool f0 = t.i0 != INT_MAX, f1 = t.i1 != INT_MAX, f2 = t.i2 != INT_MAX;
    const float u0 = f0 ? 1.f / (sqrtf(t.d0) + 1e-8f) : 0.f;
    const float u1 = f1 ? 1.f / (sqrtf(t.d1) + 1e-8f) : 0.f;
    const float u2 = f2 ? 1.f / (sqrtf(t.d2) + 1e-8f) : 0.f;
    const float sum = (u0 + u1) + u2;
    oi[0] = f0 ? t.i0 : -1, oi[1] = f1 ? t.i1 : -1, oi[2] = f2 ? t.i2 : -1;
    ow[0] = f0 ? u0 / sum : 0.f, ow[1] = f1 ? u1 / sum : 0.f, ow[2] = f2 ? u2 / sum : 0.f;
  }
}

__global__ __launch_bounds__(V3D_BLOCK) void vp_reduce_kernel(const float* __restrict__ feat, int ldf, long long rows, int C, int Cr,
                                                              float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x;
  if (t >= rows * Cr) return;
  const long long r = t / Cr;
  const int j = (int)(t - r * Cr);
  const float* f = feat + (size_t)r * ldf + j;
  float acc = f[0];
  for (int m = Cr; m < C; m += Cr) acc += f[m];
  out[t] = acc;
}

// grid (query blocks, nv); CL columns of VPE_QPP = 256 / CL queries per pass, VPE_PASSES passes per workgroup
#define VPE_PASSES 8
template <int CL>
__global__ __launch_bounds__(V3D_BLOCK) void vp_embed_kernel(const float* __restrict__ fr, int ldf, const float* __restrict__ xyz,
                                                             const float* __restrict__ new_xyz, const int* __restrict__ idx,
                                                             const float* __restrict__ w, int rows, int N, int M, int nv, int Cr,
                                                             const VpqOffsets offs, const float* __restrict__ W_local,
                                                             const float* __restrict__ shift, float* __restrict__ out, int ldo) {
  constexpr int QPP = V3D_BLOCK / CL;
  __shared__ float sW[VPE_MAX_K * CL];
  __shared__ float sShift[CL];
  __shared__ float sRow[QPP][VPE_MAX_K + 1];
  const int v = blockIdx.y, K = Cr + 9;
  for (int e = threadIdx.x; e < K * CL; e += V3D_BLOCK) sW[e] = W_local[(size_t)v * K * CL + e];
  if (threadIdx.x < CL) sShift[threadIdx.x] = shift[v * CL + threadIdx.x];
  const int s = threadIdx.x / CL, col = threadIdx.x % CL;
  const float ox = offs.o[v][0], oy = offs.o[v][1], oz = offs.o[v][2];
  for (int pass = 0; pass < VPE_PASSES; pass++) {
    const int row = (blockIdx.x * VPE_PASSES + pass) * QPP + s;
    __syncthreads();  // (the weights are in; the previous pass has read its rows)
    if (row < rows) {
      const int b = row / M;
      const size_t e = ((size_t)row * nv + v) * 3;
      const int i0 = idx[e], i1 = idx[e + 1], i2 = idx[e + 2];
      const bool f0 = (unsigned)i0 < (unsigned)N, f1 = (unsigned)i1 < (unsigned)N, f2 = (unsigned)i2 < (unsigned)N;
      const float w0 = w[e], w1 = w[e + 1], w2 = w[e + 2];
      const size_t base = (size_t)b * N;
      for (int j = col; j < K; j += CL) {
        float val = 0.f;
        if (j < Cr) {
          if (f0) val = fmaf(w0, fr[(base + i0) * ldf + j], val);
          if (f1) val = fmaf(w1, fr[(base + i1) * ldf + j], val);
          if (f2) val = fmaf(w2, fr[(base + i2) * ldf + j], val);
        } else {
          const int k = (j - Cr) / 3, a = (j - Cr) % 3;
          const int i = k == 0 ? i0 : k == 1 ? i1 : i2;
          if ((unsigned)i < (unsigned)N) {
            const float c = new_xyz[3 * (size_t)row + a] + (a == 0 ? ox : a == 1 ? oy : oz);
            val = c - xyz[3 * (base + i) + a];
          }
        }
        sRow[s][j] = val;
      }
    }
    __syncthreads();
    if (row < rows) {
      float acc = 0.f;
      for (int j = 0; j < K; j++) acc = fmaf(sRow[s][j], sW[j * CL + col], acc);
      out[(size_t)row * ldo + v * CL + col] = fmaxf(acc + sShift[col], 0.f);
    }
  }
}

static int vp_offsets(VpqOffsets& o, int vx, int vy, int vz, float radius) {
  if (vx < 1 || vy < 1 || vz < 1 || !(radius > 0.f) || !std::isfinite(radius)) return V3D_EINVAL;
  if (vx > VPQ_MAX_AXIS || vy > VPQ_MAX_AXIS || vz > VPQ_MAX_AXIS) return V3D_EUNSUPPORTED;
  const double R = (double)radius;
  for (int i = 0; i < vx; i++)
    for (int j = 0; j < vy; j++)
      for (int k = 0; k < vz; k++) {
        float* p = o.o[(i * vy + j) * vz + k];
        p[0] = (float)(((2 * i + 1) / (double)vx - 1.0) * R);
        p[1] = (float)(((2 * j + 1) / (double)vy - 1.0) * R);
        p[2] = (float)(((2 * k + 1) / (double)vz - 1.0) * R);
      }
  return V3D_OK;
}

extern "C" size_t v3d_vector_pool_query_workspace(int B, int N) {
  if (B < 0 || N < 0) return 0;
  return (size_t)B * cg_frame_bytes(N);
}

extern "C" int v3d_vector_pool_query(const float* xyz, const float* new_xyz, int B, int N, int M, int vx, int vy, int vz, float radius,
                                     int32_t* idx, float* w, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (B < 0 || N < 0 || M < 0) return V3D_EINVAL;
  VpqOffsets offs = {};
  int rc = vp_offsets(offs, vx, vy, vz, radius);
  if (rc) return rc;
  const int nv = vx * vy * vz;
  if (B > VPQ_MAX_B || N > VPQ_MAX_N || (long long)B * N > VPQ_MAX_BN || (long long)B * M * nv > VPQ_MAX_CENTRES) return V3D_EUNSUPPORTED;
  if (B == 0 || M == 0) return V3D_OK;
  if (!new_xyz || !idx || !w || !workspace || (N > 0 && !xyz) || ((uintptr_t)workspace & 15)) return V3D_EINVAL;
  if (workspace_bytes < v3d_vector_pool_query_workspace(B, N)) return V3D_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // a neighbour of a centre lies within R of it and the centre within (1 - 1 / v) R of the query, per axis; the slack covers the
  // roundings of q + off and of the differences (coordinates of a few hundred metres: 3e-5 m)
  float reach[3];
  const int vs[3] = {vx, vy, vz};
  for (int a = 0; a < 3; a++) reach[a] = (float)((double)radius * (2.0 - 1.0 / vs[a]) * (1.0 + 1e-5) + 1e-3);
  if (N > 0) {  // cells of the reach, records sorted by cell alone
    const V3dCellGridJob job = {xyz, workspace, N, std::max(reach[0], reach[1]), 1};
    rc = v3d_i_cell_grid_build(1, &job, B, st);
    if (rc) return rc;
  }
  const int rows = B * M;
  hipLaunchKernelGGL(vpq_query_kernel, dim3(v3d_ceil_div(rows, VPQ_WAVES)), dim3(V3D_BLOCK), 0, st, new_xyz, rows, M, N, nv, offs, reach[0],
                     reach[1], reach[2], radius * radius, (const unsigned char*)workspace, idx, w);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_vector_pool_reduce(const float* feat, int ldf, int rows, int C, int Cr, float* out, v3d_stream_t stream) {
  if (rows < 0 || C < 1 || Cr < 1 || C % Cr || ldf < C) return V3D_EINVAL;
  if (rows == 0) return V3D_OK;
  if (!feat || !out) return V3D_EINVAL;
  hipLaunchKernelGGL(vp_reduce_kernel, dim3(v3d_ceil_div((long long)rows * Cr, V3D_BLOCK)), dim3(V3D_BLOCK), 0, (hipStream_t)stream, feat,
                     ldf, (long long)rows, C, Cr, out);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_vector_pool_embed(const float* fr, int ldf, const float* xyz, const float* new_xyz, const int32_t* idx, const float* w,
                                     int B, int N, int M, int vx, int vy, int vz, float radius, int Cr, int CL, const float* W_local,
                                     const float* shift, float* out, int ldo, v3d_stream_t stream) {
  if (B < 0 || N < 0 || M < 0 || Cr < 1 || ldf < Cr) return V3D_EINVAL;
  VpqOffsets offs = {};
  int rc = vp_offsets(offs, vx, vy, vz, radius);
  if (rc) return rc;
  const int nv = vx * vy * vz;
  if (ldo < nv * CL) return V3D_EINVAL;
  if (B > VPQ_MAX_B || N > VPQ_MAX_N || (long long)B * N > VPQ_MAX_BN || (long long)B * M * nv > VPQ_MAX_CENTRES || Cr > VPE_MAX_CR ||
      (CL != 16 && CL != 32))
    return V3D_EUNSUPPORTED;
  if (B == 0 || M == 0) return V3D_OK;
  if (!new_xyz || !idx || !w || !W_local || !shift || !out || (N > 0 && (!fr || !xyz))) return V3D_EINVAL;
  const int rows = B * M;
  hipStream_t st = (hipStream_t)stream;
  if (CL == 16) {
    hipLaunchKernelGGL(vp_embed_kernel<16>, dim3(v3d_ceil_div(rows, VPE_PASSES * (V3D_BLOCK / 16)), nv), dim3(V3D_BLOCK), 0, st, fr, ldf, xyz,
                       new_xyz, idx, w, rows, N, M, nv, Cr, offs, W_local, shift, out, ldo);
  } else {
    hipLaunchKernelGGL(vp_embed_kernel<32>, dim3(v3d_ceil_div(rows, VPE_PASSES * (V3D_BLOCK / 32)), nv), dim3(V3D_BLOCK), 0, st, fr, ldf, xyz,
                       new_xyz, idx, w, rows, N, M, nv, Cr, offs, W_local, shift, out, ldo);
  }
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
