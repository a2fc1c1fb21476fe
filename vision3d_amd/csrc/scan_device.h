// scan_device.h -- the workgroup prefix sums, counts and chained-scan steps the compacting / binning / ranking kernels share,
// stated once (wave64 throughout).  Every thread of the workgroup calls a block-wide helper at a workgroup-uniform point.
// The helpers keep no array of their own and return every value they compute -- a caller never reads (or stores into) the `lds`
// words it lends them, which hold per-wave sums and nothing else.
#pragma once
#include <hip/hip_runtime.h>

// Inclusive prefix sum over the lanes of a wave: lane l gets v(0) + ... + v(l).  SPAN < 64 stops the ladder early: exact for the
// lanes below SPAN (those above hold the sum of their last SPAN lanes).
template <int SPAN = 64>
__device__ __forceinline__ int v3d_wave_scan_incl(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < SPAN; off <<= 1) {
    const int t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// Inclusive prefix sum of one int per thread over a workgroup of WAVES waves, in thread order; `total` = the sum over the
// workgroup, to every thread.  `lds` >= WAVES ints.
// BARRIERS: exactly one, between the waves' stores of their sums and the reads.  It also orders the caller's earlier LDS and
// global stores before its later reads, like any barrier.  None stands behind the reads: a slow wave may still be reading `lds`
// when a fast one returns, so `lds` may be written again (by the next scan, or by the caller) only behind a later barrier of the
// workgroup.  A scan in a loop puts that barrier at the end of its body.
template <int WAVES>
__device__ __forceinline__ int v3d_block_scan_incl(int v, int& total, int* lds) {
  static_assert(WAVES >= 1 && WAVES <= 16, "a workgroup holds at most 1 024 threads");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int incl = v3d_wave_scan_incl(v);
  if (lane == 63) lds[w] = incl;
  __syncthreads();
  int woff = 0, tot = 0;  // the sums of the waves before mine, and of all
  if constexpr (WAVES <= 4) {
#pragma unroll
    for (int i = 0; i < WAVES; i++) {
      const int c = lds[i];
      if (i < w) woff += c;
      tot += c;
    }
  } else {  // scanned by the lanes: two registers where the loop keeps WAVES reads in flight (bq_grid_build_kernel<20> sits at its
            // 128-register limit and spilled 56 bytes per lane with the loop, 20 with this)
    const int c = lane < WAVES ? lds[lane] : 0;
    const int s = v3d_wave_scan_incl<WAVES>(c);
    woff = __shfl(s - c, w);
    tot = __shfl(s, WAVES - 1);
  }
  total = tot;
  return woff + incl;
}

// Sum of v over a workgroup of WAVES waves, returned to every thread.  The order is fixed -- an xor butterfly inside the wave, then
// the waves in index order through `red` (>= WAVES entries of LDS) --, which is what makes the losses bit-repeatable.  Every
// thread of the workgroup calls it, at a workgroup-uniform point; it opens with the barrier that lets `red` be reused by the
// next sum while slow waves still read the previous one.
template <int WAVES, typename T>
__device__ __forceinline__ T v3d_block_sum(T v, T* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) t += red[w];
  return t;
}

// ------------------------------------------------------------------------------------------------
// Wave64 ballot + popcount compaction.  One flag per thread, 256-thread blocks.
// Returns the exclusive rank of this thread's flag inside the block; `total` = flags set in the block.
// `lds` must hold >= 4 ints and is free for reuse on return.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int v3d_block_rank(bool flag, int& total, int* lds) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) lds[w] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int c = lds[i];
    if (i < w) off += c;
    tot += c;
  }
  __syncthreads();
  total = tot;
  return off + r;
}

// count -> scan in ONE launch without fences: counts[] is pre-set to -1 (part of the frame's 0xFF fill); every block
// PUBLISHES its count with an agent-scope atomic store, and the block with the highest index -- dispatched after all
// the others, so everything it waits for is already running or done -- reads them with agent-scope loads, spinning
// on entries that are still -1, and scans.  (A fence + arrival-counter variant cost 15 us per launch in L2
// write-backs; this one costs the same as the plain count kernel and saves the dependent scan launch.)
__device__ __forceinline__ void v3d_publish_count(int* slot, int value) {
  __hip_atomic_store(slot, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int v3d_load_coherent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int v3d_wait_count(const int* slot) {
  int v = v3d_load_coherent(slot);
  while (v < 0) {
    __builtin_amdgcn_s_sleep(1);
    v = v3d_load_coherent(slot);
  }
  return v;
}

// The chained scans' "sum of all my predecessors' published counts": counts[0] + ... + counts[n - 1], each waited for, to every
// thread of a 256-thread block -- every thread its share of the slots, an xor butterfly, the four waves' parts through `lds`
// (>= 4 ints).  The caller has published its own count before (nobody may wait on a block that waits).  BARRIERS: as
// v3d_block_scan_incl -- one, between the stores of the parts and their reads, none in front and none behind.
__device__ __forceinline__ int v3d_wait_prefix(const int* counts, int n, int* lds) {
  int part = 0;
  for (int i = threadIdx.x; i < n; i += 256) part += v3d_wait_count(counts + i);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = part;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// In-place exclusive scan of the published counts[0..n) by ONE 256-thread block (the highest-index block of a count
// kernel); returns the grand total to every thread.  `lds` >= 4 ints.
__device__ __forceinline__ int v3d_block_exclusive_scan_global(int* counts, int n, int* lds) {
  int carry = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int idx = c0 + threadIdx.x;
    const int v = idx < n ? v3d_wait_count(counts + idx) : 0;
    int tot;
    const int incl = v3d_block_scan_incl<4>(v, tot, lds);
    if (idx < n) v3d_publish_count(counts + idx, carry + incl - v);
    carry += tot;
    __syncthreads();
  }
  return carry;
}
