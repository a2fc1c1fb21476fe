// cell_grid.hip -- the builder of cell_grid_device.h's frames: one 1 024-thread workgroup per (job, frame) does the bounds, the LDS
// histogram over the (index chunk, cell) keys, the scan and the scatter of the (x, y, z, index) records in one launch.
#include <algorithm>

#include "v3d_internal.h"
#include "dpp_device.h"
#include "cell_grid_device.h"

#define CG_BUILD_THREADS 1024

struct CgBuildJobs {
  V3dCellGridJob j[V3D_CELL_GRID_MAX_JOBS];
};

// One workgroup per (database, frame).  PPT > 0: N <= PPT * CG_BUILD_THREADS for every job and a thread keeps its points in
// registers (ONE trip to memory instead of three: a workgroup alone on its compute unit has nothing to hide a trip behind);
// PPT == 0: any N, the points are read again in every pass.
template <int PPT>
__global__ __launch_bounds__(CG_BUILD_THREADS) void bq_grid_build_kernel(const CgBuildJobs jobs) {
  extern __shared__ int bq_cnt[];  // [CG_MAX_KEYS]
  __shared__ float red[4][CG_BUILD_THREADS / V3D_WAVE];
  __shared__ int wsum[CG_BUILD_THREADS / V3D_WAVE];
  __shared__ CgHeader g;
  int* cnt = bq_cnt;
  const V3dCellGridJob job = jobs.j[blockIdx.x];
  const int N = job.N;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* p = job.xyz + (size_t)b * N * 3;
  unsigned char* w = (unsigned char*)job.ws + (size_t)b * cg_frame_bytes(N);
  int* cell_start = reinterpret_cast<int*>(w + CG_HEADER_BYTES);
  float4* sorted = reinterpret_cast<float4*>(w + cg_record_offset());
  const float inf = __builtin_huge_valf();
  [[maybe_unused]] float px[PPT ? PPT : 1], py[PPT ? PPT : 1], pz[PPT ? PPT : 1];
  if constexpr (PPT > 0) {
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      const int i = tid + k * CG_BUILD_THREADS;
      px[k] = i < N ? p[3 * (size_t)i] : inf;  // (a slot beyond N reads as a non-finite point: left out like one)
      py[k] = i < N ? p[3 * (size_t)i + 1] : inf;
      pz[k] = i < N ? p[3 * (size_t)i + 2] : inf;
    }
  }
  // body(i, x, y, z) for every point with finite x and y (a point with a non-finite x or y can be in no ball: it is left out of the grid)
  auto for_points = [&](auto body) {
    if constexpr (PPT > 0) {
#pragma unroll
      for (int k = 0; k < PPT; k++)
        if (fabsf(px[k]) < inf && fabsf(py[k]) < inf) body(tid + k * CG_BUILD_THREADS, px[k], py[k], pz[k]);
    } else {
      for (int i = tid; i < N; i += CG_BUILD_THREADS) {
        const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
        if (fabsf(x) < inf && fabsf(y) < inf) body(i, x, y, z);
      }
    }
  };
  // (a) bounds
  float xlo = inf, xhi = -inf, ylo = inf, yhi = -inf;
  for_points([&](int, float x, float y, float) {
    xlo = fminf(xlo, x), xhi = fmaxf(xhi, x);
    ylo = fminf(ylo, y), yhi = fmaxf(yhi, y);
  });
  xlo = -v3d_dpp_max_f32<true>(-xlo), xhi = v3d_dpp_max_f32<true>(xhi);
  ylo = -v3d_dpp_max_f32<true>(-ylo), yhi = v3d_dpp_max_f32<true>(yhi);
  if (lane == 0) red[0][wave] = xlo, red[1][wave] = xhi, red[2][wave] = ylo, red[3][wave] = yhi;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < CG_BUILD_THREADS / V3D_WAVE; i++) {
      xlo = fminf(xlo, red[0][i]), xhi = fmaxf(xhi, red[1][i]);
      ylo = fminf(ylo, red[2][i]), yhi = fmaxf(yhi, red[3][i]);
    }
    const CgHeader t = cg_shape(xlo, xhi, ylo, yhi, job.cell_min, N, job.max_chunks);
    g = t;
    *reinterpret_cast<CgHeader*>(w) = t;
  }
  __syncthreads();
  CgHeader gg = g;
  // (the same word in every lane: in a scalar register, so that cg_cell's test of it costs <20> no vector register -- it sits at its
  //  limit of 128)
  gg.inv_c = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gg.inv_c)));
  const int ncell = gg.nx * gg.ny, nkeys = ncell * gg.nch;
  // keys per thread of the scan below: covers nkeys + 1, odd (thread t walks the words [t * kpt, (t + 1) * kpt): an odd stride is
  // conflict-free)
  const int kpt = ((nkeys + CG_BUILD_THREADS) / CG_BUILD_THREADS) | 1;
  for (int i = tid; i < kpt * CG_BUILD_THREADS; i += CG_BUILD_THREADS)
    if (i < CG_MAX_KEYS) cnt[i] = 0;
  __syncthreads();
  auto key_of = [&](int i, float x, float y) {
    return (i / gg.chunk) * ncell + (int)cg_cell(y, gg.y0, gg.inv_c) * gg.nx + (int)cg_cell(x, gg.x0, gg.inv_c);
  };
  // (b) histogram
  for_points([&](int i, float x, float y, float) { atomicAdd(&cnt[key_of(i, x, y)], 1); });
  __syncthreads();
  // (c) exclusive scan over the keys: kpt consecutive keys per thread, in place (the counts become the keys' write cursors)
  const int k_lo = tid * kpt;
  int sum = 0;
  for (int k = 0; k < kpt; k++)
    if (k_lo + k < CG_MAX_KEYS) sum += cnt[k_lo + k];
  int binned;  // the number of binned points
  int run = v3d_block_scan_incl<CG_BUILD_THREADS / V3D_WAVE>(sum, binned, wsum) - sum;
  for (int k = 0; k < kpt; k++) {
    const int c = k_lo + k;
    if (c < CG_MAX_KEYS) {
      const int own = cnt[c];
      cnt[c] = run;
      run += own;
    }
  }
  __syncthreads();
  // the table as the queries read it: coalesced, not a thread's kpt consecutive words (the scan's layout: one 64-byte line per lane
  // and store instruction -- 30 us of a 45 us build at 26 000 keys); entry nkeys = the number of binned points
  for (int c = tid; c <= nkeys; c += CG_BUILD_THREADS) cell_start[c] = c < nkeys ? cnt[c] : binned;
  __syncthreads();
  // (d) scatter (the order inside a key's run is whatever the atomics give: the queries do not depend on it)
  for_points([&](int i, float x, float y, float z) { sorted[atomicAdd(&cnt[key_of(i, x, y)], 1)] = make_float4(x, y, z, __int_as_float(i)); });
}

int v3d_i_cell_grid_build(int n_jobs, const V3dCellGridJob* job, int B, hipStream_t st) {
  CgBuildJobs jobs;
  int n_max = 0;
  for (int i = 0; i < n_jobs; i++) {
    jobs.j[i] = job[i];
    n_max = std::max(n_max, job[i].N);
  }
  const size_t lds = (size_t)CG_MAX_KEYS * sizeof(int);
#define CG_BUILD(PPT)                                                                                                         \
  {                                                                                                                           \
    V3D_CHECK_HIP(hipFuncSetAttribute((const void*)bq_grid_build_kernel<PPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(bq_grid_build_kernel<PPT>, dim3(n_jobs, B), dim3(CG_BUILD_THREADS), lds, st, jobs);                    \
  }
  if (n_max <= 4 * CG_BUILD_THREADS) CG_BUILD(4)
  else if (n_max <= 12 * CG_BUILD_THREADS) CG_BUILD(12)
  else if (n_max <= 20 * CG_BUILD_THREADS) CG_BUILD(20)
  else CG_BUILD(0)
#undef CG_BUILD
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
