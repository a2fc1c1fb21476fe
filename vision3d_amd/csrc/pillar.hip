// pillar.hip -- the pillar feature encoder (PointPillars' PFN layer: linear, BatchNorm, ReLU, max over a pillar's points), forward
// and backward; pillar_device.h states the arithmetic.  No upstream counterpart: the definition is this repository's
// (detector/pillar.py:forward_torch in torch, tests/pillar_ref.py in float64).
//
// Every kernel gives a pillar to a wave: lane p loads point slot p, the pillar's xyz go through a 16-float LDS row per slot for the
// mean in row order, then lane p writes its feature row there.
//   pillar_encode_kernel   a lane owns channels lane (+ 64), their K weights in registers; it sweeps the pillar's n feature rows as
//                          LDS broadcasts and stores its channels: the wave writes the pillar's output row as 256-byte runs.
//   pillar_moments_kernel  training: lane p adds its row into K + K (K + 1) / 2 double moments in registers; one partial per workgroup.
//   pillar_stats_kernel    one workgroup: partials in workgroup order -> moments -> mean, biased variance, scale, shift per channel.
//   pillar_bwd_kernel      a lane reads its channels' winner rows from LDS and adds g, g y, g f into doubles it alone owns (no
//                          reduction across lanes); the four waves' sums are added in wave order: one partial per workgroup.
//   pillar_bwd_final_kernel  a workgroup per channel: partials in workgroup order, then the closed forms of pillar_device.h.
// No atomics: every sum has one fixed order for a given M, so two runs agree bit for bit.  No host synchronisation.
// The dynamic encoder (cfg.PILLAR.DYNAMIC: the pillars of the dynamic voxelizer, every point counts) follows behind them, and the
// plan's front (cfg.PILLAR.PLAN: the hard encoder writing the dense head's split planes itself) at the end of the file.
#include "pillar_device.h"
#include "pillar_plane_device.h"
#include "scan_device.h"
#include "split_prec.h"
#include "v3d_internal.h"

#define PL_WAVES (V3D_BLOCK / V3D_WAVE)
#define PL_ROW 16            // floats of a slot's LDS row (K <= 14), so a row is read as float4s
#define PL_MAX_GROUPS 256    // workgroups of the two kernels that leave per-workgroup partials
#define PL_MAX_ENCODE_GROUPS 4096

namespace {

using v3d::PillarGeom;

// The pillar of this wave: n (0 for a wave without one), the lane's point and the pillar's centre.  Returns with the lane's feature
// row in `f` (lanes >= n: untouched) and every live row in slab[p * PL_ROW ..].  Called by all threads of the workgroup at a
// workgroup-uniform point; on return the rows may be read, and the caller puts a barrier behind its reads.
template <int C>
__device__ __forceinline__ int pl_stage(const float* __restrict__ feat, const int32_t* __restrict__ occ, const int32_t* __restrict__ coords,
                                        int m, int M, int P, const PillarGeom& g, float* slab, float* f) {
  const int lane = threadIdx.x & 63;
  int n = 0;
  float pt[C], centre[3];
  if (m < M) {
    n = min(max(occ[m], 0), P);
#pragma unroll
    for (int k = 0; k < 3; k++) centre[k] = v3d::pillar_centre(coords[(size_t)m * 4 + 3 - k], g.v[k], g.o[k]);
  }
  if (lane < n) {
#pragma unroll
    for (int k = 0; k < C; k++) pt[k] = feat[((size_t)m * P + lane) * C + k];
#pragma unroll
    for (int k = 0; k < 3; k++) slab[lane * PL_ROW + k] = pt[k];
  }
  __syncthreads();
  float mean[3] = {0.f, 0.f, 0.f};
  if (n > 0) v3d::pillar_mean(slab, PL_ROW, n, mean);
  __syncthreads();
  if (lane < n) {
    v3d::pillar_feature_row<C>(pt, mean, centre, f);
#pragma unroll
    for (int k = 0; k < C + 6; k++) slab[lane * PL_ROW + k] = f[k];
  }
  __syncthreads();
  return n;
}

template <int K>
__device__ __forceinline__ void pl_read_row(const float* slab, int p, float* f) {
  const float4* row = reinterpret_cast<const float4*>(slab + p * PL_ROW);
  float t[PL_ROW];
#pragma unroll
  for (int q = 0; q < (K + 3) / 4; q++) {
    const float4 v = row[q];
    t[4 * q] = v.x;
    t[4 * q + 1] = v.y;
    t[4 * q + 2] = v.z;
    t[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int k = 0; k < K; k++) f[k] = t[k];
}

// The maximum of a staged pillar (n live rows in the slab, P slots) over the NCH channels a lane owns: rows 0 .. n-1 in order, then the
// padded candidate where n < P (pillar_device.h, the winner rule).
template <int K, int NCH>
__device__ __forceinline__ void pl_pillar_max(const float* slab, int n, int P, const float (*w)[K], const float* sc, const float* sh, float* best,
                                              int* win) {
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    best[j] = -1.f;
    win[j] = -1;
  }
  for (int p = 0; p < n; p++) {
    float f[K];
    pl_read_row<K>(slab, p, f);
    v3d::pillar_offer_row<K, NCH>(f, p, w, sc, sh, best, win);
  }
  if (n < P) {
#pragma unroll
    for (int j = 0; j < NCH; j++) v3d::pillar_offer(v3d::pillar_activation(0.f, sc[j], sh[j]), -1, best[j], win[j]);
  }
}

template <int C, int NCH>
__global__ __launch_bounds__(V3D_BLOCK) void pillar_encode_kernel(const float* __restrict__ feat, const int32_t* __restrict__ occ,
                                                                  const int32_t* __restrict__ coords, int M, int P, PillarGeom g,
                                                                  const float* __restrict__ W, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, float* __restrict__ rows,
                                                                  int32_t* __restrict__ winner) {
  constexpr int K = C + 6, CH = 64 * NCH;
  __shared__ float4 slabs[PL_WAVES][64 * PL_ROW / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* slab = reinterpret_cast<float*>(slabs[wave]);
  float w[NCH][K], sc[NCH], sh[NCH];
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    const int c = lane + 64 * j;
#pragma unroll
    for (int k = 0; k < K; k++) w[j][k] = W[c * K + k];
    sc[j] = scale[c];
    sh[j] = shift[c];
  }
  for (int base = blockIdx.x * PL_WAVES; base < M; base += gridDim.x * PL_WAVES) {
    const int m = base + wave;
    float f[K];
    const int n = pl_stage<C>(feat, occ, coords, m, M, P, g, slab, f);
    if (m < M) {
      float best[NCH];
      int win[NCH];
      pl_pillar_max<K, NCH>(slab, n, P, w, sc, sh, best, win);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        rows[(size_t)m * CH + lane + 64 * j] = best[j];
        if (winner) winner[(size_t)m * CH + lane + 64 * j] = win[j];
      }
    }
    __syncthreads();  // the next pillar's rows overwrite the slab
  }
}

template <int C>
__global__ __launch_bounds__(V3D_BLOCK) void pillar_moments_kernel(const float* __restrict__ feat, const int32_t* __restrict__ occ,
                                                                   const int32_t* __restrict__ coords, int M, int P, PillarGeom g,
                                                                   double* __restrict__ partials) {
  constexpr int K = C + 6, NM = K + K * (K + 1) / 2;
  __shared__ float4 slabs[PL_WAVES][64 * PL_ROW / 4];
  __shared__ double red[PL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* slab = reinterpret_cast<float*>(slabs[wave]);
  double S[NM];
#pragma unroll
  for (int i = 0; i < NM; i++) S[i] = 0.0;
  for (int base = blockIdx.x * PL_WAVES; base < M; base += gridDim.x * PL_WAVES) {
    float f[K];
    const int n = pl_stage<C>(feat, occ, coords, base + wave, M, P, g, slab, f);
    if (lane < n) v3d::pillar_moments_add<K>(f, S);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NM; i++) {
    const double t = v3d_block_sum<PL_WAVES>(S[i], red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * NM + i] = t;
  }
}

// One workgroup.  bn (4, CH): mean, biased variance, scale, shift.  counted (the dynamic encoder): every partial, and `moments`, end
// in one more double, the number of rows behind the sums, and that sum is N -- the host does not know it.
__global__ __launch_bounds__(V3D_BLOCK) void pillar_stats_kernel(const double* __restrict__ partials, int groups, int K, int CH, double N,
                                                                 int counted, const float* __restrict__ W, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, double* __restrict__ moments,
                                                                 float* __restrict__ bn) {
  __shared__ double S[V3D_PILLAR_MAX_MOMENTS + 1];
  const int nm = v3d::pillar_moments(K), entries = nm + (counted ? 1 : 0);
  for (int i = threadIdx.x; i < entries; i += V3D_BLOCK) {
    double t = 0.0;
    for (int b = 0; b < groups; b++) t += partials[(size_t)b * entries + i];
    S[i] = t;
    moments[i] = t;
  }
  __syncthreads();
  if (counted) N = S[nm];
  for (int c = threadIdx.x; c < CH; c += V3D_BLOCK) {
    double mean, var, scale, shift;
    v3d::pillar_bn_stats(K, S, N, W + (size_t)c * K, mean, var);
    if (counted)
      v3d::pillar_fold_counted(N, mean, var, (double)gamma[c], (double)beta[c], (double)eps, scale, shift);
    else
      v3d::pillar_fold(mean, var, (double)gamma[c], (double)beta[c], (double)eps, scale, shift);
    bn[c] = (float)mean;
    bn[CH + c] = (float)var;
    bn[2 * CH + c] = (float)scale;
    bn[3 * CH + c] = (float)shift;
  }
}

// partials (groups, CH, K + 2) double: G0, Gy, Gf[0..K) per channel.
template <int C, int NCH>
__global__ __launch_bounds__(V3D_BLOCK) void pillar_bwd_kernel(const float* __restrict__ feat, const int32_t* __restrict__ occ,
                                                               const int32_t* __restrict__ coords, int M, int P, PillarGeom g,
                                                               const float* __restrict__ W, const float* __restrict__ rows,
                                                               const int32_t* __restrict__ winner, const float* __restrict__ d_rows,
                                                               double* __restrict__ partials) {
  constexpr int K = C + 6, CH = 64 * NCH, Q = K + 2;
  __shared__ float4 slabs[PL_WAVES][64 * PL_ROW / 4];
  __shared__ double red[PL_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* slab = reinterpret_cast<float*>(slabs[wave]);
  float w[NCH][K];
  double G[NCH][Q];
#pragma unroll
  for (int j = 0; j < NCH; j++) {
#pragma unroll
    for (int k = 0; k < K; k++) w[j][k] = W[(lane + 64 * j) * K + k];
#pragma unroll
    for (int q = 0; q < Q; q++) G[j][q] = 0.0;
  }
  for (int base = blockIdx.x * PL_WAVES; base < M; base += gridDim.x * PL_WAVES) {
    const int m = base + wave;
    float f[K];
    const int n = pl_stage<C>(feat, occ, coords, m, M, P, g, slab, f);
    if (m < M) {
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const size_t at = (size_t)m * CH + lane + 64 * j;
        const int win = winner[at];
        const float go = rows[at] > 0.f && win >= -1 && win < n ? d_rows[at] : 0.f;  // (an index outside the pillar: no gradient)
        float y = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) f[k] = 0.f;
        if (win >= 0 && win < n) {
          pl_read_row<K>(slab, win, f);
          y = v3d::pillar_dot<K>(w[j], f);
        }
        const double gd = (double)go;
        G[j][0] += gd;
        G[j][1] += gd * (double)y;
#pragma unroll
        for (int k = 0; k < K; k++) G[j][2 + k] += gd * (double)f[k];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NCH; j++) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      __syncthreads();
      red[wave][lane] = G[j][q];
      __syncthreads();
      if (wave == 0) {
        double t = red[0][lane];
#pragma unroll
        for (int v = 1; v < PL_WAVES; v++) t += red[v][lane];
        partials[((size_t)blockIdx.x * CH + lane + 64 * j) * Q + q] = t;
      }
    }
  }
}

// A workgroup of 64 threads per channel.  counted: N is the double behind the moments (pillar_stats_kernel).
__global__ __launch_bounds__(64) void pillar_bwd_final_kernel(const double* __restrict__ partials, int groups, int K, int CH, double N,
                                                              int counted, const double* __restrict__ moments, const float* __restrict__ W,
                                                              const float* __restrict__ gamma, float eps, float* __restrict__ dW,
                                                              float* __restrict__ d_gamma, float* __restrict__ d_beta) {
  __shared__ double Gs[V3D_PILLAR_MAX_K + 2];
  const int c = blockIdx.x, Q = K + 2;
  if (counted) N = moments[v3d::pillar_moments(K)];
  if ((int)threadIdx.x < Q) {
    double t = 0.0;
    for (int b = 0; b < groups; b++) t += partials[((size_t)b * CH + c) * Q + threadIdx.x];
    Gs[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double dw[V3D_PILLAR_MAX_K], dg, db;
    if (counted)
      v3d::pillar_bwd_channel_counted(K, moments, N, W + (size_t)c * K, (double)gamma[c], (double)eps, Gs[0], Gs[1], Gs + 2, dw, dg, db);
    else
      v3d::pillar_bwd_channel(K, moments, N, W + (size_t)c * K, (double)gamma[c], (double)eps, Gs[0], Gs[1], Gs + 2, dw, dg, db);
    for (int k = 0; k < K; k++) dW[(size_t)c * K + k] = (float)dw[k];
    d_gamma[c] = (float)dg;
    d_beta[c] = (float)db;
  }
}

int pl_groups(int M, int cap) { return std::min(v3d_ceil_div(M, PL_WAVES), cap); }

bool pl_supported(int P, int C, int CH) {
  return P >= 1 && P <= V3D_PILLAR_MAX_P && C >= V3D_PILLAR_MIN_C && C <= V3D_PILLAR_MAX_C && (CH == 64 || CH == 128);
}

PillarGeom pl_geom(const float* h) {
  PillarGeom g;
  for (int k = 0; k < 3; k++) {
    g.v[k] = h[k];
    g.o[k] = h[3 + k];
  }
  return g;
}

// Runs the statements with PC = the compile-time C.
#define PL_DISPATCH_C(C_, ...)                            \
  switch (C_) {                                           \
    case 3: { constexpr int PC = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int PC = 4; __VA_ARGS__; } break; \
    case 5: { constexpr int PC = 5; __VA_ARGS__; } break; \
    case 6: { constexpr int PC = 6; __VA_ARGS__; } break; \
    case 7: { constexpr int PC = 7; __VA_ARGS__; } break; \
    default: { constexpr int PC = 8; __VA_ARGS__; } break; \
  }

int pl_launch_encode(const float* feat, const int32_t* occ, const int32_t* coords, int M, int P, int C, const PillarGeom& g, const float* W,
                     int CH, const float* scale, const float* shift, float* rows, int32_t* winner, hipStream_t st) {
  const dim3 grid(pl_groups(M, PL_MAX_ENCODE_GROUPS)), block(V3D_BLOCK);
  PL_DISPATCH_C(C, {
    if (CH == 64)
      hipLaunchKernelGGL((pillar_encode_kernel<PC, 1>), grid, block, 0, st, feat, occ, coords, M, P, g, W, scale, shift, rows, winner);
    else
      hipLaunchKernelGGL((pillar_encode_kernel<PC, 2>), grid, block, 0, st, feat, occ, coords, M, P, g, W, scale, shift, rows, winner);
  });
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

size_t pl_fwd_partials_bytes(int M, int C) { return v3d_align((size_t)pl_groups(M, PL_MAX_GROUPS) * v3d::pillar_moments(C + 6) * sizeof(double)); }

}  // namespace

extern "C" int v3d_pillar_encode(const float* features, const int32_t* occupancy, const int32_t* coordinates, int M, int P, int C,
                                 const float* geometry_host, const float* W, int channels, const float* scale, const float* shift,
                                 float* rows, v3d_stream_t stream) {
  if (M < 0 || !geometry_host) return V3D_EINVAL;
  if (!pl_supported(P, C, channels)) return V3D_EUNSUPPORTED;
  if (M == 0) return V3D_OK;
  if (!features || !occupancy || !coordinates || !W || !scale || !shift || !rows) return V3D_EINVAL;
  return pl_launch_encode(features, occupancy, coordinates, M, P, C, pl_geom(geometry_host), W, channels, scale, shift, rows, nullptr,
                          (hipStream_t)stream);
}

extern "C" size_t v3d_pillar_train_workspace(int M, int P, int C, int channels) {
  if (M <= 0 || !pl_supported(P, C, channels)) return 256;
  const size_t fwd = pl_fwd_partials_bytes(M, C);
  const size_t bwd = v3d_align((size_t)pl_groups(M, PL_MAX_GROUPS) * channels * (C + 8) * sizeof(double));
  return std::max(fwd, bwd);
}

extern "C" int v3d_pillar_train_fwd(const float* features, const int32_t* occupancy, const int32_t* coordinates, int M, int P, int C,
                                    const float* geometry_host, const float* W, int channels, const float* gamma, const float* beta,
                                    float eps, float* rows, int32_t* winner, float* bn, double* moments, void* workspace,
                                    size_t workspace_bytes, v3d_stream_t stream) {
  if (M < 0 || !geometry_host) return V3D_EINVAL;
  if (!pl_supported(P, C, channels)) return V3D_EUNSUPPORTED;
  if (M == 0) return V3D_OK;
  if (!features || !occupancy || !coordinates || !W || !gamma || !beta || !rows || !winner || !bn || !moments || !workspace) return V3D_EINVAL;
  if (workspace_bytes < pl_fwd_partials_bytes(M, C) || ((uintptr_t)workspace & 7) || ((uintptr_t)moments & 7)) return V3D_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const PillarGeom g = pl_geom(geometry_host);
  const int groups = pl_groups(M, PL_MAX_GROUPS);
  double* partials = (double*)workspace;
  PL_DISPATCH_C(C, { hipLaunchKernelGGL((pillar_moments_kernel<PC>), dim3(groups), dim3(V3D_BLOCK), 0, st, features, occupancy, coordinates, M, P, g, partials); });
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(pillar_stats_kernel, dim3(1), dim3(V3D_BLOCK), 0, st, (const double*)partials, groups, C + 6, channels,
                     (double)M * (double)P, 0, W, gamma, beta, eps, moments, bn);
  V3D_CHECK_LAUNCH();
  return pl_launch_encode(features, occupancy, coordinates, M, P, C, g, W, channels, bn + 2 * channels, bn + 3 * channels, rows, winner, st);
}

extern "C" int v3d_pillar_train_bwd(const float* features, const int32_t* occupancy, const int32_t* coordinates, int M, int P, int C,
                                    const float* geometry_host, const float* W, int channels, const float* gamma, float eps,
                                    const float* rows, const int32_t* winner, const float* d_rows, const double* moments, float* dW,
                                    float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (M <= 0 || !geometry_host) return V3D_EINVAL;
  if (!pl_supported(P, C, channels)) return V3D_EUNSUPPORTED;
  if (!features || !occupancy || !coordinates || !W || !gamma || !rows || !winner || !d_rows || !moments || !dW || !d_gamma || !d_beta ||
      !workspace)
    return V3D_EINVAL;
  const int groups = pl_groups(M, PL_MAX_GROUPS);
  if (workspace_bytes < (size_t)groups * channels * (C + 8) * sizeof(double) || ((uintptr_t)workspace & 7) || ((uintptr_t)moments & 7))
    return V3D_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const PillarGeom g = pl_geom(geometry_host);
  double* partials = (double*)workspace;
  PL_DISPATCH_C(C, {
    if (channels == 64)
      hipLaunchKernelGGL((pillar_bwd_kernel<PC, 1>), dim3(groups), dim3(V3D_BLOCK), 0, st, features, occupancy, coordinates, M, P, g, W, rows, winner, d_rows, partials);
    else
      hipLaunchKernelGGL((pillar_bwd_kernel<PC, 2>), dim3(groups), dim3(V3D_BLOCK), 0, st, features, occupancy, coordinates, M, P, g, W, rows, winner, d_rows, partials);
  });
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(pillar_bwd_final_kernel, dim3(channels), dim3(64), 0, st, (const double*)partials, groups, C + 6, channels,
                     (double)M * (double)P, 0, moments, W, gamma, eps, dW, d_gamma, d_beta);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- dynamic encoder
// The encoder over the dynamic voxelizer's point_voxel map (pillar_device.h "The DYNAMIC encoder"): every point of a pillar counts.
//   pillar_dyn_offsets_kernel  one workgroup: offsets = exclusive scan of occupancy (scan_device.h), the cursors set to zero.
//   pillar_dyn_list_kernel     a thread per point takes the next slot of its pillar with an integer atomic cursor: the point list.
//                              The order inside a pillar may differ between runs; the winner rule does not depend on it.
//   pillar_dyn_encode_kernel   one wave (a workgroup of its own) per pillar: the list is walked in chunks of 64 through the LDS slab,
//                              a lane owns channels lane (+ 64) with their K weights in registers.
//   pillar_dyn_moments_kernel  a thread per point, grid-stride in a capped grid: double moments and the kept count in registers, one
//                              partial per workgroup; pillar_stats_kernel adds them in workgroup order and takes N from the count.
//   pillar_dyn_bwd_kernel      a wave per pillar, a lane per channel: the winner POINT is read directly (it belongs to the pillar when
//                              point_voxel says so); partials as pillar_bwd_kernel, then pillar_bwd_final_kernel with the counted N.
// No float atomics; every float sum has one fixed order for a given (N, M): two runs agree bit for bit.
//
// GUARDS -- no input, however inconsistent, makes a kernel read or write outside its buffers:
//   * a point_voxel outside [0, M) is skipped by every kernel that reads one (list, moments);
//   * an occupancy is clamped to [0, N] and the running offset saturates at N, so 0 <= offsets[v] <= offsets[v + 1] <= N whatever
//     the counts hold, and no partial sum leaves int (a thread's 8 items saturate at N <= 2^22, 256 threads: 2^30);
//   * a point takes slot r of its pillar only when r < offsets[v + 1] - offsets[v]: a pillar with more points than its occupancy
//     says loses the surplus instead of writing into its neighbour's range; list entries [offsets[v], offsets[v] + min(cursor[v],
//     range)) are exactly the written ones -- the encode kernel reads no others, so an unfilled entry is never read;
//   * a list entry outside [0, N) reads as "no point"; a winner is followed only when 0 <= winner < N and point_voxel[winner] is
//     the pillar that names it.
#define PD_SCAN_ITEMS 8
#define PD_MAX_ENCODE_GROUPS 4096  // one-wave workgroups
#define PD_MAX_N (1 << 22)         // the dynamic voxelizer's limit

namespace {

__global__ __launch_bounds__(V3D_BLOCK) void pillar_dyn_offsets_kernel(const int32_t* __restrict__ occ, int M, int N, int32_t* __restrict__ offsets,
                                                                       int32_t* __restrict__ cursor) {
  __shared__ int lds[PL_WAVES];
  int carry = 0;
  for (int c0 = 0; c0 < M; c0 += V3D_BLOCK * PD_SCAN_ITEMS) {
    const int first = c0 + threadIdx.x * PD_SCAN_ITEMS;
    int n[PD_SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int q = 0; q < PD_SCAN_ITEMS; q++) {
      n[q] = first + q < M ? min(max(occ[first + q], 0), N) : 0;
      mine = min(mine + n[q], N);
    }
    int total;
    const int incl = v3d_block_scan_incl<PL_WAVES>(mine, total, lds);
    int at = min(carry + (incl - mine), N);
#pragma unroll
    for (int q = 0; q < PD_SCAN_ITEMS; q++) {
      if (first + q < M) {
        offsets[first + q] = at;
        cursor[first + q] = 0;
      }
      at = min(at + n[q], N);
    }
    carry = min(carry + total, N);
    __syncthreads();  // the next round's scan writes `lds` again
  }
  if (threadIdx.x == 0) offsets[M] = carry;
}

__global__ __launch_bounds__(V3D_BLOCK) void pillar_dyn_list_kernel(const int32_t* __restrict__ point_voxel, int N, int M,
                                                                    const int32_t* __restrict__ offsets, int32_t* __restrict__ cursor,
                                                                    int32_t* __restrict__ list) {
  const int i = blockIdx.x * V3D_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int v = point_voxel[i];
  if (v < 0 || v >= M) return;
  const int start = offsets[v], room = offsets[v + 1] - start;  // 0 <= start, start + room <= N (pillar_dyn_offsets_kernel)
  const int r = atomicAdd(cursor + v, 1);                       // at most N increments: no overflow
  if (r < room) list[start + r] = i;
}

template <int C, int NCH>
__global__ __launch_bounds__(64) void pillar_dyn_encode_kernel(const float* __restrict__ points, int N, const float* __restrict__ mean,
                                                               const int32_t* __restrict__ coords, int M, const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ cursor, const int32_t* __restrict__ list,
                                                               PillarGeom g, const float* __restrict__ W, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, float* __restrict__ rows,
                                                               int32_t* __restrict__ winner) {
  constexpr int K = C + 6, CH = 64 * NCH;
  __shared__ float4 slab4[64 * PL_ROW / 4];
  __shared__ int index[64];
  float* slab = reinterpret_cast<float*>(slab4);
  const int lane = threadIdx.x;
  float w[NCH][K], sc[NCH], sh[NCH];
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    const int c = lane + 64 * j;
#pragma unroll
    for (int k = 0; k < K; k++) w[j][k] = W[c * K + k];
    sc[j] = scale[c];
    sh[j] = shift[c];
  }
  for (int m = blockIdx.x; m < M; m += gridDim.x) {
    const int start = min(max(offsets[m], 0), N), room = min(max(offsets[m + 1], start), N) - start;
    const int count = min(max(cursor[m], 0), room);  // the written entries of the pillar's range
    float mu[3], centre[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      mu[k] = mean[(size_t)m * C + k];
      centre[k] = v3d::pillar_centre(coords[(size_t)m * 4 + 3 - k], g.v[k], g.o[k]);
    }
    float best[NCH];
    int win[NCH];
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      best[j] = -1.f;
      win[j] = -1;
    }
    for (int base = 0; base < count; base += 64) {  // (workgroup = wave: every trip count is workgroup-uniform)
      const int n = min(64, count - base);
      int i = -1;
      if (lane < n) {
        i = list[start + base + lane];
        if (i < 0 || i >= N) i = -1;
      }
      if (i >= 0) {
        float pt[C], f[K];
#pragma unroll
        for (int k = 0; k < C; k++) pt[k] = points[(size_t)i * C + k];
        v3d::pillar_feature_row<C>(pt, mu, centre, f);
#pragma unroll
        for (int k = 0; k < K; k++) slab[lane * PL_ROW + k] = f[k];
      }
      index[lane] = i;
      __syncthreads();
      for (int p = 0; p < n; p++) {
        const int ip = index[p];
        if (ip < 0) continue;
        float f[K];
        pl_read_row<K>(slab, p, f);
        v3d::pillar_offer_point<K, NCH>(f, ip, w, sc, sh, best, win);
      }
      __syncthreads();  // the next chunk overwrites the slab
    }
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      rows[(size_t)m * CH + lane + 64 * j] = win[j] >= 0 ? best[j] : 0.f;  // (no candidate: an empty or all-NaN pillar)
      if (winner) winner[(size_t)m * CH + lane + 64 * j] = win[j];
    }
  }
}

// partials (groups, NM + 1) double: the moments, then the number of kept points.
template <int C>
__global__ __launch_bounds__(V3D_BLOCK) void pillar_dyn_moments_kernel(const float* __restrict__ points, const int32_t* __restrict__ point_voxel,
                                                                       int N, const float* __restrict__ mean, const int32_t* __restrict__ coords,
                                                                       int M, PillarGeom g, double* __restrict__ partials) {
  constexpr int K = C + 6, NM = K + K * (K + 1) / 2;
  __shared__ double red[PL_WAVES];
  double S[NM], kept = 0.0;
#pragma unroll
  for (int i = 0; i < NM; i++) S[i] = 0.0;
  for (int i = blockIdx.x * V3D_BLOCK + threadIdx.x; i < N; i += gridDim.x * V3D_BLOCK) {
    const int v = point_voxel[i];
    if (v < 0 || v >= M) continue;
    float pt[C], mu[3], centre[3], f[K];
#pragma unroll
    for (int k = 0; k < C; k++) pt[k] = points[(size_t)i * C + k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      mu[k] = mean[(size_t)v * C + k];
      centre[k] = v3d::pillar_centre(coords[(size_t)v * 4 + 3 - k], g.v[k], g.o[k]);
    }
    v3d::pillar_feature_row<C>(pt, mu, centre, f);
    v3d::pillar_moments_add<K>(f, S);
    kept += 1.0;
  }
#pragma unroll
  for (int i = 0; i < NM; i++) {
    const double t = v3d_block_sum<PL_WAVES>(S[i], red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * (NM + 1) + i] = t;
  }
  const double t = v3d_block_sum<PL_WAVES>(kept, red);
  if (threadIdx.x == 0) partials[(size_t)blockIdx.x * (NM + 1) + NM] = t;
}

// partials (groups, CH, K + 2) double as pillar_bwd_kernel's.
template <int C, int NCH>
__global__ __launch_bounds__(V3D_BLOCK) void pillar_dyn_bwd_kernel(const float* __restrict__ points, const int32_t* __restrict__ point_voxel,
                                                                   int N, const float* __restrict__ mean, const int32_t* __restrict__ coords,
                                                                   int M, PillarGeom g, const float* __restrict__ W, const float* __restrict__ rows,
                                                                   const int32_t* __restrict__ winner, const float* __restrict__ d_rows,
                                                                   double* __restrict__ partials) {
  constexpr int K = C + 6, CH = 64 * NCH, Q = K + 2;
  __shared__ double red[PL_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float w[NCH][K];
  double G[NCH][Q];
#pragma unroll
  for (int j = 0; j < NCH; j++) {
#pragma unroll
    for (int k = 0; k < K; k++) w[j][k] = W[(lane + 64 * j) * K + k];
#pragma unroll
    for (int q = 0; q < Q; q++) G[j][q] = 0.0;
  }
  for (int m = blockIdx.x * PL_WAVES + wave; m < M; m += gridDim.x * PL_WAVES) {
    float mu[3], centre[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      mu[k] = mean[(size_t)m * C + k];
      centre[k] = v3d::pillar_centre(coords[(size_t)m * 4 + 3 - k], g.v[k], g.o[k]);
    }
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const size_t at = (size_t)m * CH + lane + 64 * j;
      const int win = winner[at];
      if (!(rows[at] > 0.f) || win < 0 || win >= N || point_voxel[win] != m) continue;  // (a winner outside the pillar: no gradient)
      float pt[C], f[K];
#pragma unroll
      for (int k = 0; k < C; k++) pt[k] = points[(size_t)win * C + k];
      v3d::pillar_feature_row<C>(pt, mu, centre, f);
      const double gd = (double)d_rows[at], y = (double)v3d::pillar_dot<K>(w[j], f);
      G[j][0] += gd;
      G[j][1] += gd * y;
#pragma unroll
      for (int k = 0; k < K; k++) G[j][2 + k] += gd * (double)f[k];
    }
  }
#pragma unroll
  for (int j = 0; j < NCH; j++) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      __syncthreads();
      red[wave][lane] = G[j][q];
      __syncthreads();
      if (wave == 0) {
        double t = red[0][lane];
#pragma unroll
        for (int v = 1; v < PL_WAVES; v++) t += red[v][lane];
        partials[((size_t)blockIdx.x * CH + lane + 64 * j) * Q + q] = t;
      }
    }
  }
}

bool pd_supported(int n_points, int M, int C, int CH) {
  return n_points <= PD_MAX_N && M <= PD_MAX_N && C >= V3D_PILLAR_MIN_C && C <= V3D_PILLAR_MAX_C && (CH == 64 || CH == 128);
}

int pd_moment_groups(int n_points) { return std::min(v3d_ceil_div(std::max(n_points, 1), V3D_BLOCK), PL_MAX_GROUPS); }

// The workspace: doubles first (the partials of the moments, later of the backward), then offsets (M + 1), cursor (M), list (N).
struct PdWorkspace {
  double* partials;
  int32_t *offsets, *cursor, *list;
  bool ok;
};

size_t pd_partials_doubles(int n_points, int M, int C, int CH) {
  const size_t fwd = (size_t)pd_moment_groups(n_points) * (v3d::pillar_moments(C + 6) + 1);
  const size_t bwd = (size_t)pl_groups(std::max(M, 1), PL_MAX_GROUPS) * CH * (C + 8);
  return std::max(fwd, bwd);
}

PdWorkspace pd_carve(void* workspace, size_t bytes, int n_points, int M, int C, int CH) {
  V3dArena a(workspace, bytes);
  PdWorkspace w;
  w.partials = a.take<double>(pd_partials_doubles(n_points, M, C, CH));
  w.offsets = a.take<int32_t>((size_t)M + 1);
  w.cursor = a.take<int32_t>((size_t)M);
  w.list = a.take<int32_t>((size_t)std::max(n_points, 1));
  w.ok = a.ok() && w.partials && w.offsets && w.cursor && w.list;
  return w;
}

// offsets -> list -> encode: the three launches of the eval forward, the last three of the training forward.
int pd_launch_encode(const float* points, const int32_t* point_voxel, int N, const float* mean, const int32_t* occ, const int32_t* coords, int M,
                     int C, const PillarGeom& g, const float* W, int CH, const float* scale, const float* shift, float* rows, int32_t* winner,
                     const PdWorkspace& ws, hipStream_t st) {
  hipLaunchKernelGGL(pillar_dyn_offsets_kernel, dim3(1), dim3(V3D_BLOCK), 0, st, occ, M, N, ws.offsets, ws.cursor);
  V3D_CHECK_LAUNCH();
  if (N > 0) {
    hipLaunchKernelGGL(pillar_dyn_list_kernel, dim3(v3d_ceil_div(N, V3D_BLOCK)), dim3(V3D_BLOCK), 0, st, point_voxel, N, M,
                       (const int32_t*)ws.offsets, ws.cursor, ws.list);
    V3D_CHECK_LAUNCH();
  }
  const dim3 grid(std::min(M, PD_MAX_ENCODE_GROUPS)), block(64);
  PL_DISPATCH_C(C, {
    if (CH == 64)
      hipLaunchKernelGGL((pillar_dyn_encode_kernel<PC, 1>), grid, block, 0, st, points, N, mean, coords, M, (const int32_t*)ws.offsets,
                         (const int32_t*)ws.cursor, (const int32_t*)ws.list, g, W, scale, shift, rows, winner);
    else
      hipLaunchKernelGGL((pillar_dyn_encode_kernel<PC, 2>), grid, block, 0, st, points, N, mean, coords, M, (const int32_t*)ws.offsets,
                         (const int32_t*)ws.cursor, (const int32_t*)ws.list, g, W, scale, shift, rows, winner);
  });
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

}  // namespace

extern "C" size_t v3d_pillar_dynamic_workspace(int n_points, int M, int C, int channels) {
  if (n_points < 0 || M <= 0 || !pd_supported(n_points, M, C, channels)) return 256;
  return v3d_align(pd_partials_doubles(n_points, M, C, channels) * sizeof(double)) + v3d_align(((size_t)M + 1) * 4) + v3d_align((size_t)M * 4) +
         v3d_align((size_t)std::max(n_points, 1) * 4);
}

extern "C" int v3d_pillar_dynamic_encode(const float* points, const int32_t* point_voxel, int n_points, const float* voxel_mean,
                                         const int32_t* occupancy, const int32_t* coordinates, int M, int C, const float* geometry_host,
                                         const float* W, int channels, const float* scale, const float* shift, float* rows, int32_t* winner,
                                         void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (M < 0 || n_points < 0 || !geometry_host) return V3D_EINVAL;
  if (!pd_supported(n_points, M, C, channels)) return V3D_EUNSUPPORTED;
  if (M == 0) return V3D_OK;
  if ((n_points > 0 && (!points || !point_voxel)) || !voxel_mean || !occupancy || !coordinates || !W || !scale || !shift || !rows || !workspace)
    return V3D_EINVAL;
  if ((uintptr_t)workspace & 7) return V3D_EWORKSPACE;
  const PdWorkspace ws = pd_carve(workspace, workspace_bytes, n_points, M, C, channels);
  if (!ws.ok) return V3D_EWORKSPACE;
  return pd_launch_encode(points, point_voxel, n_points, voxel_mean, occupancy, coordinates, M, C, pl_geom(geometry_host), W, channels, scale,
                          shift, rows, winner, ws, (hipStream_t)stream);
}

extern "C" int v3d_pillar_dynamic_train_fwd(const float* points, const int32_t* point_voxel, int n_points, const float* voxel_mean,
                                            const int32_t* occupancy, const int32_t* coordinates, int M, int C, const float* geometry_host,
                                            const float* W, int channels, const float* gamma, const float* beta, float eps, float* rows,
                                            int32_t* winner, float* bn, double* moments, void* workspace, size_t workspace_bytes,
                                            v3d_stream_t stream) {
  if (M < 0 || n_points < 0 || !geometry_host) return V3D_EINVAL;
  if (!pd_supported(n_points, M, C, channels)) return V3D_EUNSUPPORTED;
  if (M == 0) return V3D_OK;
  if ((n_points > 0 && (!points || !point_voxel)) || !voxel_mean || !occupancy || !coordinates || !W || !gamma || !beta || !rows || !winner ||
      !bn || !moments || !workspace)
    return V3D_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)moments & 7)) return V3D_EWORKSPACE;
  const PdWorkspace ws = pd_carve(workspace, workspace_bytes, n_points, M, C, channels);
  if (!ws.ok) return V3D_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const PillarGeom g = pl_geom(geometry_host);
  const int groups = pd_moment_groups(n_points);
  PL_DISPATCH_C(C, {
    hipLaunchKernelGGL((pillar_dyn_moments_kernel<PC>), dim3(groups), dim3(V3D_BLOCK), 0, st, points, point_voxel, n_points, voxel_mean, coordinates,
                       M, g, ws.partials);
  });
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(pillar_stats_kernel, dim3(1), dim3(V3D_BLOCK), 0, st, (const double*)ws.partials, groups, C + 6, channels, 0.0, 1, W, gamma,
                     beta, eps, moments, bn);
  V3D_CHECK_LAUNCH();
  return pd_launch_encode(points, point_voxel, n_points, voxel_mean, occupancy, coordinates, M, C, g, W, channels, bn + 2 * channels,
                          bn + 3 * channels, rows, winner, ws, st);
}

extern "C" int v3d_pillar_dynamic_train_bwd(const float* points, const int32_t* point_voxel, int n_points, const float* voxel_mean,
                                            const int32_t* coordinates, int M, int C, const float* geometry_host, const float* W, int channels,
                                            const float* gamma, float eps, const float* rows, const int32_t* winner, const float* d_rows,
                                            const double* moments, float* dW, float* d_gamma, float* d_beta, void* workspace,
                                            size_t workspace_bytes, v3d_stream_t stream) {
  if (M <= 0 || n_points < 0 || !geometry_host) return V3D_EINVAL;
  if (!pd_supported(n_points, M, C, channels)) return V3D_EUNSUPPORTED;
  if ((n_points > 0 && (!points || !point_voxel)) || !voxel_mean || !coordinates || !W || !gamma || !rows || !winner || !d_rows || !moments ||
      !dW || !d_gamma || !d_beta || !workspace)
    return V3D_EINVAL;
  const int groups = pl_groups(M, PL_MAX_GROUPS);
  if (workspace_bytes < (size_t)groups * channels * (C + 8) * sizeof(double) || ((uintptr_t)workspace & 7) || ((uintptr_t)moments & 7))
    return V3D_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const PillarGeom g = pl_geom(geometry_host);
  double* partials = (double*)workspace;
  PL_DISPATCH_C(C, {
    if (channels == 64)
      hipLaunchKernelGGL((pillar_dyn_bwd_kernel<PC, 1>), dim3(groups), dim3(V3D_BLOCK), 0, st, points, point_voxel, n_points, voxel_mean,
                         coordinates, M, g, W, rows, winner, d_rows, partials);
    else
      hipLaunchKernelGGL((pillar_dyn_bwd_kernel<PC, 2>), dim3(groups), dim3(V3D_BLOCK), 0, st, points, point_voxel, n_points, voxel_mean,
                         coordinates, M, g, W, rows, winner, d_rows, partials);
  });
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(pillar_bwd_final_kernel, dim3(channels), dim3(64), 0, st, (const double*)partials, groups, C + 6, channels, 0.0, 1, moments,
                     W, gamma, eps, dW, d_gamma, d_beta);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the plan's front
// cfg.PILLAR.PLAN (runtime.PillarPlan): raw points -> the dense head's input without the (M, CH) rows, the fp32 canvas and its split.
//   pillar_encode_planes_kernel  pillar_encode_kernel whose wave, instead of its output row, writes the row's hi / lo 16-bit pieces
//                                (split_prec.h split_one: what v3d_nchw_to_split_nhwc writes for the same number) at the pillar's pixel
//                                of the two NHWC planes -- a lane owns channels lane and lane + 64, so the wave stores four 128-byte
//                                runs --, clears the pixel's bit of the inverted occupancy bitmap and, f16s, raises the range flag.
//                                The row count is read on the device: the grid is sized from the capacity.
//   pillar_planes_clear_kernel   start of a frame: the bitmap back to 0xFF, the summary word to 0 and -- PERSISTENT planes -- the
//                                pixels of the list the previous frame kept zeroed with 16-byte stores (no 2 x 9 MB fill per frame).
//                                A launch of its own in front of the stores above: a pixel of both frames ends on the new values.
// Where a row lands: pillar_plane_device.h.  Several rows on one pixel (a hand-fed list): one of them wins each 2-byte store.
#define PP_CH 128
#define PP_UNITS (PP_CH * 2 / 16)  // 16-byte units per pixel and plane

namespace {

template <int C, int PREC>
__global__ __launch_bounds__(V3D_BLOCK) void pillar_encode_planes_kernel(const float* __restrict__ feat, const int32_t* __restrict__ occ,
                                                                         const int32_t* __restrict__ coords, const int32_t* __restrict__ n_ptr,
                                                                         int cap, int P, PillarGeom g, const float* __restrict__ W,
                                                                         const float* __restrict__ scale, const float* __restrict__ shift, int B,
                                                                         int H, int Wd, const float* __restrict__ entry,
                                                                         int32_t* __restrict__ range_flag, unsigned short* __restrict__ hi,
                                                                         unsigned short* __restrict__ lo, unsigned* __restrict__ occ_inv) {
  constexpr int K = C + 6, NCH = PP_CH / 64;
  __shared__ float4 slabs[PL_WAVES][64 * PL_ROW / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* slab = reinterpret_cast<float*>(slabs[wave]);
  float w[NCH][K], sc[NCH], sh[NCH];
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    const int c = lane + 64 * j;
#pragma unroll
    for (int k = 0; k < K; k++) w[j][k] = W[c * K + k];
    sc[j] = scale[c];
    sh[j] = shift[c];
  }
  const int M = v3d::pillar_live_rows(*n_ptr, cap);
  const float s_out = PREC == 1 ? entry[0] : 1.f, limit = PREC == 1 ? entry[2] : 0.f;
  float vmax = 0.f;
  for (int base = blockIdx.x * PL_WAVES; base < M; base += gridDim.x * PL_WAVES) {
    const int m = base + wave;
    float f[K];
    const int n = pl_stage<C>(feat, occ, coords, m, M, P, g, slab, f);
    if (m < M) {
      float best[NCH];
      int win[NCH];
      pl_pillar_max<K, NCH>(slab, n, P, w, sc, sh, best, win);
      const long long pix = v3d::pillar_plane_pixel(coords + (size_t)m * 4, B, H, Wd);
      if (pix >= 0) {
#pragma unroll
        for (int j = 0; j < NCH; j++) {
          unsigned short h, l;
          split_one<PREC>(best[j], s_out, h, l);
          const size_t o = (size_t)pix * PP_CH + lane + 64 * j;
          hi[o] = h;
          lo[o] = l;
          if constexpr (PREC == 1) vmax = fmaxf(vmax, fabsf(best[j]));
        }
        if (lane == 0) atomicAnd(occ_inv + v3d::pillar_occ_word(pix, Wd), ~v3d::pillar_occ_bit(pix, Wd));
      }
    }
    __syncthreads();  // the next pillar's rows overwrite the slab
  }
  if constexpr (PREC == 1) {
    if (range_flag && vmax > limit) atomicMax(range_flag, V3D_FLAG_RANGE);
  }
}

__global__ __launch_bounds__(V3D_BLOCK) void pillar_planes_clear_kernel(const int32_t* __restrict__ prev_coords, const int32_t* __restrict__ prev_n,
                                                                        int cap, int B, int H, int Wd, uint4* __restrict__ hi,
                                                                        uint4* __restrict__ lo, unsigned* __restrict__ occ_inv,
                                                                        int32_t* __restrict__ flag) {
  const long long first = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x, stride = (long long)gridDim.x * V3D_BLOCK;
  const long long words = (long long)B * H * v3d::pillar_occ_words_per_row(Wd);
  for (long long t = first; t < words; t += stride) occ_inv[t] = 0xFFFFFFFFu;
  if (flag && first == 0) *flag = 0;
  if (!prev_coords) return;
  const long long total = (long long)v3d::pillar_live_rows(*prev_n, cap) * PP_UNITS;
  for (long long t = first; t < total; t += stride) {
    const long long pix = v3d::pillar_plane_pixel(prev_coords + (size_t)(t / PP_UNITS) * 4, B, H, Wd);
    if (pix < 0) continue;
    const size_t o = (size_t)pix * PP_UNITS + (size_t)(t % PP_UNITS);
    hi[o] = make_uint4(0u, 0u, 0u, 0u);
    lo[o] = make_uint4(0u, 0u, 0u, 0u);
  }
}

}  // namespace

extern "C" int v3d_pillar_encode_planes(const float* features, const int32_t* occupancy, const int32_t* coordinates, const int32_t* n_voxels,
                                        int cap, int P, int C, const float* geometry_host, const float* W, int channels, const float* scale,
                                        const float* shift, int B, int H, int Wd, int prec, const float* act_entry, int32_t* range_flag,
                                        void* out_hi, void* out_lo, uint32_t* occ, v3d_stream_t stream) {
  if (cap < 0 || !geometry_host || B < 1 || H < 1 || Wd < 1) return V3D_EINVAL;
  if (!pl_supported(P, C, channels) || channels != PP_CH) return V3D_EUNSUPPORTED;
  if (prec == V3D_PREC_F16S ? !act_entry : prec != V3D_PREC_BF16X3) return V3D_EINVAL;
  if (cap == 0) return V3D_OK;
  if (!features || !occupancy || !coordinates || !n_voxels || !W || !scale || !shift || !out_hi || !out_lo || !occ) return V3D_EINVAL;
  const dim3 grid(pl_groups(cap, PL_MAX_ENCODE_GROUPS)), block(V3D_BLOCK);
  const PillarGeom g = pl_geom(geometry_host);
  hipStream_t st = (hipStream_t)stream;
  PL_DISPATCH_C(C, {
    if (prec == V3D_PREC_F16S)
      hipLaunchKernelGGL((pillar_encode_planes_kernel<PC, 1>), grid, block, 0, st, features, occupancy, coordinates, n_voxels, cap, P, g, W, scale,
                         shift, B, H, Wd, act_entry, range_flag, (unsigned short*)out_hi, (unsigned short*)out_lo, occ);
    else
      hipLaunchKernelGGL((pillar_encode_planes_kernel<PC, 0>), grid, block, 0, st, features, occupancy, coordinates, n_voxels, cap, P, g, W, scale,
                         shift, B, H, Wd, (const float*)nullptr, (int32_t*)nullptr, (unsigned short*)out_hi, (unsigned short*)out_lo, occ);
  });
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_pillar_planes_clear(const int32_t* prev_coordinates, const int32_t* prev_n, int cap, int B, int H, int Wd, int channels,
                                       void* out_hi, void* out_lo, uint32_t* occ, int32_t* flag, v3d_stream_t stream) {
  if (B < 1 || H < 1 || Wd < 1 || !occ || cap < 0) return V3D_EINVAL;
  if (channels != PP_CH) return V3D_EUNSUPPORTED;
  const bool list = prev_coordinates != nullptr && cap > 0;
  if (list && (!prev_n || !out_hi || !out_lo || ((uintptr_t)out_hi & 15) || ((uintptr_t)out_lo & 15))) return V3D_EINVAL;
  const long long words = (long long)B * H * v3d::pillar_occ_words_per_row(Wd);
  const long long work = std::max(words, list ? (long long)cap * PP_UNITS : 0ll);
  hipLaunchKernelGGL(pillar_planes_clear_kernel, dim3((int)std::min<long long>(v3d_ceil_div(work, (long long)V3D_BLOCK), 2048)), dim3(V3D_BLOCK), 0,
                     (hipStream_t)stream, list ? prev_coordinates : (const int32_t*)nullptr, prev_n, cap, B, H, Wd, (uint4*)out_hi, (uint4*)out_lo,
                     occ, flag);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
