// keypoints.hip -- sectorized proposal-centric keypoint sampling (the sampler of PV-RCNN++ for PV_RCNN.sample_keypoints).
//
// No upstream counterpart: the definition is the repository's own (vision3d_amd/pointnet2/pointnet2_utils.py, module docstring).
// Per frame: keep the finite points within R_j of some stage-1 proposal (all finite points if that leaves none), split them into S
// azimuth sectors, give every sector a quota proportional to its size, and run an independent farthest-point chain per sector --
// S times shorter chains on S compute units side by side instead of ONE K-step chain on one unit (fps_kernel, pointops.hip).
//   kp_count_kernel   a workgroup per 2 048-point chunk of one frame, a wave per 512 consecutive points (8 rounds of 64): the frame's
//       proposals in LDS as (centre, R^2), per point the candidate test and the sector; ballot + popcount per (sector, wave), for BOTH
//       candidate sets (all finite points / those near a proposal: which one the frame uses is only known once every chunk is counted)
//       -> seg[frame][chunk][wave][set][sector]
//   kp_scan_kernel    a workgroup per frame: running sums over the (chunk, wave) counts written back in place, the candidate set of the
//       frame, n_k, the quotas q_k by the integer rule, every sector's first row in the lists and first slot in the output
//   kp_emit_kernel    the count kernel's grid again: the test repeated, rank inside the wave from the ballot ->
//       sector-contiguous lists of (x, y, z, original index), each in increasing original index
//   kp_sector_fps_kernel   a workgroup per (sector, frame): fps_kernel's step (points and running distances in registers, DPP arg-max,
//       one barrier) on the sector's list; register slots behind the sector's size are skipped by wave-uniform branches
//       (<= 24 576 points per sector; above that the same chain with its running distances in the workspace)
//   kp_pad_kernel     slot i >= n' repeats slot i mod n'
// No workgroup waits on another, no atomic decides a position, nothing is read back: a pure function of the inputs, capturable.
#include <algorithm>

#include "v3d_common.h"
#include "dpp_device.h"

#define KP_MAX_SECTORS 64
#define KP_MAX_PROPOSALS 1024
#define KP_ROUNDS 8
#define KP_WAVES (V3D_BLOCK / V3D_WAVE)             // 4
#define KP_WAVE_POINTS (KP_ROUNDS * V3D_WAVE)       // 512
#define KP_CHUNK (KP_WAVES * KP_WAVE_POINTS)        // 2 048
#define KP_FPS_THREADS 1024
#define KP_FPS_SLOTS 24                             // register slots (points) per thread of a chain
#define KP_FPS_CAPACITY (KP_FPS_SLOTS * KP_FPS_THREADS)  // 24 576: points of ONE sector that stay in registers
// per-frame header (int32): {candidate set (0: all finite points, 1: near a proposal), n' = filled slots, n = candidates, -},
// then n_k, q_k, first output slot, first list row -- KP_MAX_SECTORS words each
#define KP_HDR (4 + 4 * KP_MAX_SECTORS)
#define KP_HDR_N 4
#define KP_HDR_Q (4 + KP_MAX_SECTORS)
#define KP_HDR_OUT (4 + 2 * KP_MAX_SECTORS)
#define KP_HDR_ROW (4 + 3 * KP_MAX_SECTORS)

// workspace: hdr[B][KP_HDR] i32, seg[B][chunks][KP_WAVES][2][KP_MAX_SECTORS] i32, list[B][N] float4, td[B][N] f32 (running distances
// of a sector above KP_FPS_CAPACITY)
struct KpWork {
  int *hdr, *seg;
  float4* list;
  float* td;
  int chunks;
  size_t bytes;
};
static __host__ __device__ inline KpWork kp_work(void* base, int B, int N) {
  KpWork w;
  char* p = (char*)base;
  w.chunks = (N + KP_CHUNK - 1) / KP_CHUNK;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p + off;
    off += (bytes + 255) / 256 * 256;
    return r;
  };
  w.hdr = (int*)take((size_t)B * KP_HDR * 4);
  w.seg = (int*)take((size_t)B * w.chunks * KP_WAVES * 2 * KP_MAX_SECTORS * 4);
  w.list = (float4*)take((size_t)B * N * 16);
  w.td = (float*)take((size_t)B * N * 4);
  w.bytes = off;
  return w;
}

// the 8 points of a lane (row base + 64 r + lane of the frame): coordinates, sector (-1: behind the frame's end or not finite), and
// bit r of `near`: within R_j of some proposal (sp: (centre, R_j^2) in LDS)
__device__ __forceinline__ void kp_classify(const float* __restrict__ frame, int stride, int N, int base, int S, const float4* sp, int P,
                                            float (&x)[KP_ROUNDS], float (&y)[KP_ROUNDS], float (&z)[KP_ROUNDS], int (&sec)[KP_ROUNDS],
                                            unsigned& near) {
  const int lane = threadIdx.x & 63;
  const float scale = (float)S * 0.159154937f;
#pragma unroll
  for (int r = 0; r < KP_ROUNDS; r++) {
    const int i = base + r * V3D_WAVE + lane;
    x[r] = y[r] = z[r] = 0.f;
    sec[r] = -1;
    if (i < N) {
      const float* p = frame + (size_t)i * stride;
      x[r] = p[0], y[r] = p[1], z[r] = p[2];
      if (__builtin_isfinite(x[r]) && __builtin_isfinite(y[r]) && __builtin_isfinite(z[r])) {
        const float t = (atan2f(y[r], x[r]) + 3.14159274f) * scale;
        sec[r] = min(S - 1, max(0, (int)t));
      }
    }
  }
  near = 0u;
  for (int j = 0; j < P; j++) {
    const float4 q = sp[j];  // the same address in every lane: an LDS broadcast
#pragma unroll
    for (int r = 0; r < KP_ROUNDS; r++) {
      const float dx = x[r] - q.x, dy = y[r] - q.y, dz = z[r] - q.z;
      near |= ((dx * dx + dy * dy) + dz * dz < q.w ? 1u : 0u) << r;
    }
  }
}

__device__ __forceinline__ void kp_stage_proposals(const float* __restrict__ proposals, int b, int P, float radius, float4* sp) {
  for (int j = threadIdx.x; j < P; j += V3D_BLOCK) {
    const float* q = proposals + ((size_t)b * P + j) * 7;
    const float R = 0.5f * fmaxf(fmaxf(q[3], q[4]), q[5]) + radius;
    sp[j] = make_float4(q[0], q[1], q[2], R * R);
  }
  __syncthreads();
}

__global__ __launch_bounds__(V3D_BLOCK) void kp_count_kernel(const float* __restrict__ points, int stride, int B, int N, int S,
                                                             const float* __restrict__ proposals, int P, float radius, void* work) {
  __shared__ float4 sp[KP_MAX_PROPOSALS];
  const KpWork w = kp_work(work, B, N);
  const int tid = threadIdx.x, c = blockIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  kp_stage_proposals(proposals, b, P, radius, sp);
  float x[KP_ROUNDS], y[KP_ROUNDS], z[KP_ROUNDS];
  int sec[KP_ROUNDS];
  unsigned near;
  kp_classify(points + (size_t)b * N * stride, stride, N, c * KP_CHUNK + wave * KP_WAVE_POINTS, S, sp, P, x, y, z, sec, near);
  int all = 0, flt = 0;  // lane k: the wave's points of sector k, in either set
  for (int k = 0; k < S; k++) {
    int ca = 0, cf = 0;
#pragma unroll
    for (int r = 0; r < KP_ROUNDS; r++) {
      ca += __popcll(__ballot(sec[r] == k));
      cf += __popcll(__ballot(sec[r] == k && ((near >> r) & 1u)));
    }
    if (lane == k) all = ca, flt = cf;
  }
  int* row = w.seg + (((size_t)b * w.chunks + c) * KP_WAVES + wave) * 2 * KP_MAX_SECTORS;
  row[lane] = all;
  row[KP_MAX_SECTORS + lane] = flt;
}

#define KP_SCAN_THREADS (2 * KP_MAX_SECTORS)  // thread (set, sector) for the running sums; wave 0 = a thread per sector after them
__global__ __launch_bounds__(KP_SCAN_THREADS) void kp_scan_kernel(int B, int N, int K, int S, int P, int32_t* __restrict__ sector_counts,
                                                                  void* work) {
  __shared__ int tot[2][KP_MAX_SECTORS];
  __shared__ int quota[KP_MAX_SECTORS];
  __shared__ long long rem[KP_MAX_SECTORS];
  const KpWork w = kp_work(work, B, N);
  const int tid = threadIdx.x, b = blockIdx.x, k = tid & 63;
  const bool lead = tid < KP_MAX_SECTORS;  // (wave 1 only joins the barriers below)
  {  // running sum over the frame's (chunk, wave) segments, left in place
    const int set = tid >> 6;
    int* p = w.seg + (size_t)b * w.chunks * KP_WAVES * 2 * KP_MAX_SECTORS + set * KP_MAX_SECTORS + k;
    int run = 0;
    for (int s = 0; s < w.chunks * KP_WAVES; s++, p += 2 * KP_MAX_SECTORS) {
      const int v = *p;
      *p = run;
      run += v;
    }
    tot[set][k] = run;
  }
  __syncthreads();
  // every sum below has <= 64 terms: each thread of wave 0 takes them itself
  int near_total = 0;
  for (int j = 0; j < S; j++) near_total += tot[1][j];
  const int set = (P > 0 && near_total > 0) ? 1 : 0;
  long long n = 0;
  for (int j = 0; j < S; j++) n += tot[set][j];
  const int nk = k < S ? tot[set][k] : 0;
  int q = nk;
  long long r = 0;
  if (n >= K) {
    q = (int)(((long long)K * nk) / n);
    r = ((long long)K * nk) % n;
  }
  if (lead) quota[k] = q, rem[k] = r;
  __syncthreads();
  if (n >= K) {  // the K - sum(q) slots left go to the largest remainders, the lower sector first among equals
    int given = 0, rank = 0;
    for (int j = 0; j < S; j++) {
      given += quota[j];
      rank += (rem[j] > r || (rem[j] == r && j < k)) ? 1 : 0;
    }
    if (k < S && rank < K - given) q++;
  }
  __syncthreads();
  if (lead) quota[k] = q;
  __syncthreads();
  if (!lead) return;
  int out0 = 0, row0 = 0, filled = 0;
  for (int j = 0; j < S; j++) {
    if (j < k) out0 += quota[j], row0 += tot[set][j];
    filled += quota[j];
  }
  int* hdr = w.hdr + (size_t)b * KP_HDR;
  if (k == 0) hdr[0] = set, hdr[1] = filled, hdr[2] = (int)n, hdr[3] = 0;
  hdr[KP_HDR_N + k] = nk;
  hdr[KP_HDR_Q + k] = k < S ? q : 0;
  hdr[KP_HDR_OUT + k] = out0;
  hdr[KP_HDR_ROW + k] = row0;
  if (sector_counts && k < S) sector_counts[(size_t)b * S + k] = nk;
}

__global__ __launch_bounds__(V3D_BLOCK) void kp_emit_kernel(const float* __restrict__ points, int stride, int B, int N, int S,
                                                            const float* __restrict__ proposals, int P, float radius, void* work) {
  __shared__ float4 sp[KP_MAX_PROPOSALS];
  const KpWork w = kp_work(work, B, N);
  const int tid = threadIdx.x, c = blockIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  const int* hdr = w.hdr + (size_t)b * KP_HDR;
  const int set = hdr[0];
  if (set == 0) P = 0;  // every finite point is a candidate: no test to repeat
  kp_stage_proposals(proposals, b, P, radius, sp);
  float x[KP_ROUNDS], y[KP_ROUNDS], z[KP_ROUNDS];
  int sec[KP_ROUNDS];
  unsigned near;
  const int p0 = c * KP_CHUNK + wave * KP_WAVE_POINTS;
  kp_classify(points + (size_t)b * N * stride, stride, N, p0, S, sp, P, x, y, z, sec, near);
  if (set == 0) near = 0xFFu;
  // lane k: the list row of the wave's next point of sector k
  int next = hdr[KP_HDR_ROW + lane] + w.seg[(((size_t)b * w.chunks + c) * KP_WAVES + wave) * 2 * KP_MAX_SECTORS + set * KP_MAX_SECTORS + lane];
  float4* list = w.list + (size_t)b * N;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < KP_ROUNDS; r++) {
    const bool cand = sec[r] >= 0 && ((near >> r) & 1u);
    int row = -1;
    for (int k = 0; k < S; k++) {
      const bool mine = cand && sec[r] == k;
      const unsigned long long m = __ballot(mine);
      if (m == 0ull) continue;  // wave-uniform
      const int first = __builtin_amdgcn_readlane(next, k);
      if (mine) row = first + __popcll(m & below);
      if (lane == k) next += __popcll(m);
    }
    if (row >= 0 && row < N) list[row] = make_float4(x[r], y[r], z[r], __int_as_float(p0 + r * V3D_WAVE + lane));
  }
}

// ---- the farthest-point chain of one sector: rows [0, n) of `lst` in increasing original index, q picks -> out[0 .. q)
// fps_kernel's step (pointops.hip): per-thread arg-max on plain floats, (max distance, min row among its holders) by two DPP
// reductions per wave, one LDS slot per wave, ONE barrier, the same two reductions over the 16 slots.  Rows are in original-index
// order, so the lowest row among equals is the lowest original index.  Thread t owns rows t + 1 024 j; the wave's slots j with
// 1 024 j + 64 wave >= n hold nothing and are skipped by a scalar branch: a step costs what the sector's size asks for.
struct KpFpsLds {
  float wave_d[2][KP_FPS_THREADS / V3D_WAVE];
  int wave_n[2][KP_FPS_THREADS / V3D_WAVE];
};

__device__ __forceinline__ int kp_block_argmax(float bd, int bn, int s, KpFpsLds& l) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float wd = v3d_dpp_max_f32<true>(bd);
  const int wn = v3d_dpp_min_i32<true>(bd == wd ? bn : 0x7FFFFFFF);
  if (lane == 0) {
    l.wave_d[s & 1][wave] = wd;
    l.wave_n[s & 1][wave] = wn;
  }
  __syncthreads();  // double-buffered slots: one barrier per step suffices
  const float sd = l.wave_d[s & 1][lane & 15];
  const int sn = l.wave_n[s & 1][lane & 15];
  const float ad = v3d_dpp_max_f32<false>(sd);
  return v3d_dpp_min_i32<false>(sd == ad ? sn : 0x7FFFFFFF);
}

template <int PPT>
__device__ __forceinline__ void kp_fps_registers(const float4* __restrict__ lst, int n, int q, int* __restrict__ out, KpFpsLds& l) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int live = __builtin_amdgcn_readfirstlane(min(PPT, max(0, (n - wave * V3D_WAVE + KP_FPS_THREADS - 1) / KP_FPS_THREADS)));
  float px[PPT], py[PPT], pz[PPT], td[PPT];
#pragma unroll
  for (int j = 0; j < PPT; j++) {  // (selects, not branches: branches here made hipcc spill whole register tuples)
    const int row = tid + j * KP_FPS_THREADS;  // strided ownership: coalesced initial load
    const bool ok = row < n;
    const float4 v = lst[ok ? row : 0];
    px[j] = ok ? v.x : 0.f;
    py[j] = ok ? v.y : 0.f;
    pz[j] = ok ? v.z : 0.f;
    td[j] = ok ? 1e10f : -1.f;  // fminf keeps -1 forever: a slot without a point can never win (distances are >= 0)
  }
  int last = 0;
  for (int s = 0;;) {
    const float4 lp = lst[last];  // uniform -> scalar load
    if (tid == 0) out[s] = __float_as_int(lp.w);
    if (++s >= q) break;
    float bd = -1.f;
    int bn = 0x7FFFFFFF;
#pragma unroll
    for (int j = 0; j < PPT; j++) {
      if (j < live) {
        const float dx = px[j] - lp.x, dy = py[j] - lp.y, dz = pz[j] - lp.z;
        const float d2 = fminf((dx * dx + dy * dy) + dz * dz, td[j]);  // no contraction: the oracle's bits
        td[j] = d2;
        const bool better = d2 > bd;  // strict: the lowest of this thread's rows wins ties (rows grow with j)
        bd = better ? d2 : bd;
        bn = better ? tid + j * KP_FPS_THREADS : bn;
      }
    }
    last = min(kp_block_argmax(bd, bn, s, l), n - 1);  // (a live row always wins; the clamp keeps the next load inside the list whatever happens)
  }
}

// a sector above KP_FPS_CAPACITY: the same chain with the running distances in the workspace (every thread touches its own rows only)
__device__ __forceinline__ void kp_fps_streamed(const float4* __restrict__ lst, float* __restrict__ td, int n, int q, int* __restrict__ out,
                                                KpFpsLds& l) {
  const int tid = threadIdx.x;
  for (int row = tid; row < n; row += KP_FPS_THREADS) td[row] = 1e10f;
  int last = 0;
  for (int s = 0;;) {
    const float4 lp = lst[last];
    if (tid == 0) out[s] = __float_as_int(lp.w);
    if (++s >= q) break;
    float bd = -1.f;
    int bn = 0x7FFFFFFF;
    for (int row = tid; row < n; row += KP_FPS_THREADS) {
      const float4 v = lst[row];
      const float dx = v.x - lp.x, dy = v.y - lp.y, dz = v.z - lp.z;
      const float d2 = fminf((dx * dx + dy * dy) + dz * dz, td[row]);
      td[row] = d2;
      const bool better = d2 > bd;
      bd = better ? d2 : bd;
      bn = better ? row : bn;
    }
    last = min(kp_block_argmax(bd, bn, s, l), n - 1);  // (a live row always wins; the clamp keeps the next load inside the list whatever happens)
  }
}

// Register capacity: a 1 024-thread workgroup leaves a lane 128 VGPRs, a slot takes four (x, y, z, running distance) -- 24 slots
// (96 registers) compile without a spill, 32 do not.  A sector above 24 576 points takes the streamed chain.
__global__ __launch_bounds__(KP_FPS_THREADS) void kp_sector_fps_kernel(int B, int N, int K, int32_t* __restrict__ idx, void* work) {
  __shared__ KpFpsLds l;
  const KpWork w = kp_work(work, B, N);
  const int k = blockIdx.x, b = blockIdx.y;
  const int* hdr = w.hdr + (size_t)b * KP_HDR;
  const int n = hdr[KP_HDR_N + k], q = hdr[KP_HDR_Q + k], out0 = hdr[KP_HDR_OUT + k], row0 = hdr[KP_HDR_ROW + k];
  if (q <= 0 || q > n || out0 < 0 || out0 + q > K || row0 < 0 || row0 + n > N) return;  // (block-uniform; only q == 0 happens)
  const float4* lst = w.list + (size_t)b * N + row0;
  int* out = idx + (size_t)b * K + out0;
  const int slots = (n + KP_FPS_THREADS - 1) / KP_FPS_THREADS;
  if (slots <= 1) kp_fps_registers<1>(lst, n, q, out, l);
  else if (slots <= 2) kp_fps_registers<2>(lst, n, q, out, l);
  else if (slots <= 4) kp_fps_registers<4>(lst, n, q, out, l);
  else if (slots <= 8) kp_fps_registers<8>(lst, n, q, out, l);
  else if (slots <= 16) kp_fps_registers<16>(lst, n, q, out, l);
  else if (slots <= KP_FPS_SLOTS) kp_fps_registers<KP_FPS_SLOTS>(lst, n, q, out, l);
  else kp_fps_streamed(lst, w.td + (size_t)b * N + row0, n, q, out, l);
}

__global__ __launch_bounds__(V3D_BLOCK) void kp_pad_kernel(int B, int N, int K, int32_t* __restrict__ idx, void* work) {
  const KpWork w = kp_work(work, B, N);
  const int b = blockIdx.y, filled = min(K, max(0, w.hdr[(size_t)b * KP_HDR + 1]));
  int* out = idx + (size_t)b * K;
  for (int i = filled + blockIdx.x * V3D_BLOCK + threadIdx.x; i < K; i += gridDim.x * V3D_BLOCK)
    out[i] = filled > 0 ? out[i % filled] : 0;  // (reads slots < n', writes slots >= n')
}

static bool kp_sizes_ok(int B, int N, int S) { return B >= 0 && N >= 1 && S >= 1 && S <= KP_MAX_SECTORS; }

extern "C" size_t v3d_keypoints_sector_workspace(int B, int N, int S) {
  if (!kp_sizes_ok(B, N, S)) return 0;
  return kp_work(nullptr, B, N).bytes;
}

extern "C" int v3d_keypoints_sector(const float* points, int point_stride, int B, int N, int K, int S, const float* proposals, int P,
                                    float radius, int32_t* idx, int32_t* sector_counts, void* workspace, size_t workspace_bytes,
                                    v3d_stream_t stream) {
  if (!kp_sizes_ok(B, N, S) || K < 1 || point_stride < 3 || P < 0 || P > KP_MAX_PROPOSALS) return V3D_EINVAL;
  if (B == 0) return V3D_OK;
  if (B > 65535) return V3D_EUNSUPPORTED;  // frames are the grid's y dimension
  if (!proposals) P = 0;
  if (!points || !idx || !workspace || ((uintptr_t)workspace & 15)) return V3D_EINVAL;
  const KpWork w = kp_work(nullptr, B, N);
  if (workspace_bytes < w.bytes) return V3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 chunks(w.chunks, B), block(V3D_BLOCK);
  hipLaunchKernelGGL(kp_count_kernel, chunks, block, 0, st, points, point_stride, B, N, S, proposals, P, radius, workspace);
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(kp_scan_kernel, dim3(B), dim3(KP_SCAN_THREADS), 0, st, B, N, K, S, P, sector_counts, workspace);
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(kp_emit_kernel, chunks, block, 0, st, points, point_stride, B, N, S, proposals, P, radius, workspace);
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(kp_sector_fps_kernel, dim3(S, B), dim3(KP_FPS_THREADS), 0, st, B, N, K, idx, workspace);
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(kp_pad_kernel, dim3(std::min(64, v3d_ceil_div(K, V3D_BLOCK)), B), block, 0, st, B, N, K, idx, workspace);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
