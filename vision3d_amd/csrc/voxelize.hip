// voxelize.hip -- device voxelizer fused with the VoxelFeatureExtractor mean (T1 + A5 + A6).
//
// Replaces spconv.utils.VoxelGenerator.generate as driven by vision3d/core/preprocess.py:17-33
// (host C++ loop over points + a 360 MB dense index grid per call) and detector/layers.py:10-17.
//
// The sequential reference semantics (voxel ids in first-touch order of the input points, the first
// max_pts points of a voxel kept in input order) are reproduced EXACTLY by a parallel formulation:
//   K1 insert : every point inserts its linear voxel key into a hash table; per slot an
//               atomicMin keeps the smallest point index (the "first toucher") and an atomicExch
//               threads the point onto the slot's linked list.
//   K2 count  : flag[i] = "point i is the first toucher of its voxel"; per-256-chunk popcounts
//               (wave64 ballots).
//   K3 scan   : exclusive scan of the chunk counts (+ per-frame voxel bases, for max_voxels).
//   K4 emit   : rank of a first toucher (chunk offset + ballot prefix) == voxel id of the
//               sequential loop.  The same thread walks its voxel's list, keeps the max_pts smallest
//               point indices (== first-come order), writes coords/occupancy/points and the mean.
//   (K2 + K3 share a launch; for ONE frame K2 + K3 + K4 are a single-pass chained scan in one launch.)
//   WIDE      : max_pts above VOX_MAX_PTS (pillars: up to VOX_MAX_PTS_WIDE slots).  K4 keeps no point list in registers: it only
//               counts its voxel's points and records the voxel's row; K5 (a thread per POINT) ranks its point among the voxel's by
//               walking the same list and writes it into its slot of the zero-filled output; K6 sums the slots in order for the mean.
// No host synchronisation: the voxel count stays in device memory.
#include "v3d_internal.h"

#define VOX_MAX_FRAMES 64
#define VOX_MAX_PTS 8
#define VOX_MAX_PTS_WIDE 64
// points per block of the count/emit kernels: ONE 256-thread round, so the per-voxel list walks of a
// whole frame run concurrently (a 2048-point chunk serialised 8 latency-bound rounds per block)
#define VOX_CHUNK 256

struct VoxParams {
  float vs[3], lo[3];
  int grid[3];
  int max_pts, max_voxels, C, B, n_points;
  int frame_off[VOX_MAX_FRAMES + 1];
};

__device__ __forceinline__ int frame_of(const VoxParams& p, int i) {
  int b = 0;
  while (b + 1 < p.B && i >= p.frame_off[b + 1]) b++;
  return b;
}

__global__ __launch_bounds__(V3D_BLOCK) void vox_insert_kernel(const float* __restrict__ pts, const VoxParams p,
                                                               const V3dHash h, unsigned* __restrict__ first,
                                                               int* __restrict__ head, int* __restrict__ pt_slot,
                                                               int* __restrict__ next) {
  for (int i = blockIdx.x * V3D_BLOCK + threadIdx.x; i < p.n_points; i += gridDim.x * V3D_BLOCK) {
    const float* q = pts + (size_t)i * p.C;
    int c[3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      // true IEEE division in fp32: bit-exact voxel indices
      const float f = floorf((q[j] - p.lo[j]) / p.vs[j]);
      ok = ok && (f >= 0.0f) && (f < (float)p.grid[j]);
      c[j] = (int)f;
    }
    if (!ok) {
      pt_slot[i] = -1;
      continue;
    }
    const int b = frame_of(p, i);
    const v3d_key_t key = (((v3d_key_t)b * p.grid[2] + c[2]) * p.grid[1] + c[1]) * p.grid[0] + c[0];
    const int s = v3d_hash_insert(h, key);
    if (s < 0) {  // unreachable: the table holds 2x n_points slots
      pt_slot[i] = -1;
      continue;
    }
    atomicMin(&first[s], (unsigned)i);
    next[i] = atomicExch(&head[s], i);
    pt_slot[i] = s;
  }
}

__device__ __forceinline__ bool vox_is_first(const int* pt_slot, const unsigned* first, int i, int n) {
  if (i >= n) return false;
  const int s = pt_slot[i];
  return s >= 0 && first[s] == (unsigned)i;
}

// count + scan in ONE launch: every block counts the first touchers of its chunk and publishes the count; the
// highest-index block turns the counts into exclusive offsets (v3d_common.h) and derives the per-frame bases.
// chunk_counts must read -1 at launch.
// frame_base[b] = number of first-touch points before frame b's first point; out_base[b] = first output
// row of frame b after clipping every earlier frame to max_voxels; n_voxels = total rows.
__global__ __launch_bounds__(V3D_BLOCK) void vox_count_scan_kernel(const int* __restrict__ pt_slot,
                                                                   const unsigned* __restrict__ first, const VoxParams p,
                                                                   int* __restrict__ chunk_counts, int n_chunks,
                                                                   int* __restrict__ frame_base, int* __restrict__ out_base,
                                                                   int* __restrict__ n_voxels) {
  __shared__ int lds[8];
  __shared__ int fb_s[VOX_MAX_FRAMES + 1];
  const int base = blockIdx.x * VOX_CHUNK;
  int cnt = 0;
  for (int r = 0; r < VOX_CHUNK / V3D_BLOCK; r++) {
    int tot;
    v3d_block_rank(vox_is_first(pt_slot, first, base + r * V3D_BLOCK + threadIdx.x, p.n_points), tot, lds);
    cnt += tot;
  }
  if (threadIdx.x == 0) v3d_publish_count(chunk_counts + blockIdx.x, cnt);
  if (blockIdx.x != gridDim.x - 1) return;

  const int total = v3d_block_exclusive_scan_global(chunk_counts, n_chunks, lds);
  __syncthreads();
  // per-frame bases: wave w handles frames w, w+4, ...
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int b = w; b <= p.B; b += V3D_BLOCK / V3D_WAVE) {
    const int pos = p.frame_off[b];
    int val;
    if (pos >= p.n_points) {
      val = total;
    } else {
      const int chunk = pos / VOX_CHUNK;
      int c = 0;
      for (int i = chunk * VOX_CHUNK + lane; i < pos; i += 64) c += vox_is_first(pt_slot, first, i, p.n_points);
      for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
      val = v3d_load_coherent(chunk_counts + chunk) + c;
    }
    if (lane == 0) {
      frame_base[b] = val;
      fb_s[b] = val;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int b = 0; b < p.B; b++) {
      out_base[b] = acc;
      acc += min(fb_s[b + 1] - fb_s[b], p.max_voxels);
    }
    out_base[p.B] = acc;
    *n_voxels = acc;
  }
}

// CHAINED (one frame, B == 1): count, scan and emit in ONE launch -- every block counts the first touchers of its chunk, PUBLISHES the
// count (chunk_offsets reads -1 at launch: part of the frame's 0xFF fill), adds up the counts of all its predecessors (spinning on
// slots that still read -1: workgroups are dispatched in index order and publish before they wait, so every wait is on a block that
// is running or done) and emits at prefix + rank; the highest-index block writes the voxel count.  The same single-pass chained
// scan as rb_scan_emit_kernel (rulebook.hip); replaces vox_count_scan_kernel + this kernel's unchained form, which stay for
// batches (B > 1: the per-frame bases need every earlier frame's total).
template <bool CHAINED, bool WIDE = false>
__global__ __launch_bounds__(V3D_BLOCK) void vox_emit_kernel(const float* __restrict__ pts, const VoxParams p,
                                                             const int* __restrict__ pt_slot,
                                                             const unsigned* __restrict__ first,
                                                             const int* __restrict__ head, const int* __restrict__ next,
                                                             int* __restrict__ chunk_offsets,
                                                             const int* __restrict__ frame_base,
                                                             const int* __restrict__ out_base,
                                                             float* __restrict__ voxels, int* __restrict__ coords,
                                                             int* __restrict__ occupancy, float* __restrict__ mean,
                                                             const V3dHash site_hash, int* __restrict__ site_vals,
                                                             int site_d, int site_h, int site_w, int* __restrict__ n_voxels,
                                                             int* __restrict__ row_of_first /*WIDE: row of the voxel point i opens, or -1*/) {
  __shared__ int lds[4];
  static_assert(VOX_CHUNK == V3D_BLOCK, "one round per block");
  const int i = blockIdx.x * VOX_CHUNK + threadIdx.x;
  const bool flag = vox_is_first(pt_slot, first, i, p.n_points);
  int tot;
  int rank = v3d_block_rank(flag, tot, lds);
  if constexpr (CHAINED) {
    if (threadIdx.x == 0) v3d_publish_count(chunk_offsets + blockIdx.x, tot);
  }
  // ---- everything about the voxel that does not depend on its NUMBER, in front of the (chained) wait for the number: the cell,
  //      the walk of the voxel's point list (the max_pts smallest point indices, ascending = first-come order) and the points
  int c[3] = {0, 0, 0};
  int best[VOX_MAX_PTS];
#pragma unroll
  for (int k = 0; k < VOX_MAX_PTS; k++) best[k] = 0x7FFFFFFF;
  int cnt = 0;
  float4 pv[VOX_MAX_PTS];
  if (flag) {
    const float* q = pts + (size_t)i * p.C;  // voxel coordinates from the first toucher itself
#pragma unroll
    for (int j = 0; j < 3; j++) c[j] = (int)floorf((q[j] - p.lo[j]) / p.vs[j]);
    for (int j = head[pt_slot[i]], guard = 0; j >= 0 && guard < p.n_points; j = next[j], guard++) {
      cnt++;
      if constexpr (!WIDE) {
        int x = j;
#pragma unroll
        for (int k = 0; k < VOX_MAX_PTS; k++) {  // sorted insert by compare-exchange
          const int lo_ = min(best[k], x);
          x = max(best[k], x);
          best[k] = lo_;
        }
      }
    }
  }
  const int occ = min(cnt, p.max_pts);
  if (!WIDE && p.C == 4) {
    // four channels (x, y, z, intensity): the points as 16-byte loads, all in flight at once (the generic loop below issues
    // max_pts x C scalar loads); same sums in the same order
#pragma unroll
    for (int k = 0; k < VOX_MAX_PTS; k++)
      pv[k] = (flag && k < p.max_pts && k < occ) ? reinterpret_cast<const float4*>(pts)[best[k]] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if constexpr (CHAINED) {
    __shared__ int s_part[V3D_BLOCK / V3D_WAVE];
    asm volatile("" ::: "memory");  // (the loads above are issued in front of the spin)
    const int prefix = v3d_wait_prefix(chunk_offsets, (int)blockIdx.x, s_part);
    rank += prefix;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_voxels = min(prefix + tot, p.max_voxels);
  } else {
    rank += chunk_offsets[blockIdx.x];
  }
  if (!flag) return;
  const int b = CHAINED ? 0 : frame_of(p, i);
  const int local = CHAINED ? rank : rank - frame_base[b];
  if (local >= p.max_voxels) {  // `continue` variant of the max_voxels rule
    if constexpr (WIDE) row_of_first[i] = -1;
    return;
  }
  const int v = CHAINED ? local : out_base[b] + local;
  reinterpret_cast<int4*>(coords)[v] = make_int4(b, c[2], c[1], c[0]);
  if (site_vals) {  // the coordinate hash the first submanifold rulebook needs (saves the rb_hash_build launch)
    // key over the RULEBOOK's grid (D, H, W), which may be larger than the voxel grid (SECOND pads z by one)
    const v3d_key_t key = (((v3d_key_t)b * site_d + c[2]) * site_h + c[1]) * site_w + c[0];
    const int hs = v3d_site_insert(site_hash, key, (unsigned)v);  // (each voxel is inserted once, with its row)
    if (hs >= 0) site_vals[hs] = v;
  }
  occupancy[v] = occ;
  if constexpr (WIDE) {  // the points and the mean: vox_fill_wide_kernel, vox_mean_wide_kernel
    row_of_first[i] = v;
    return;
  }
  if (p.C == 4) {
    float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < VOX_MAX_PTS; k++) {
      if (k < p.max_pts) {
        if (voxels) reinterpret_cast<float4*>(voxels)[(size_t)v * p.max_pts + k] = pv[k];
        sm.x += pv[k].x; sm.y += pv[k].y; sm.z += pv[k].z; sm.w += pv[k].w;
      }
    }
    const float fo = (float)occ;
    if (mean) reinterpret_cast<float4*>(mean)[v] = make_float4(sm.x / fo, sm.y / fo, sm.z / fo, sm.w / fo);
    return;
  }
  for (int ch = 0; ch < p.C; ch++) {
    float sacc = 0.f;
#pragma unroll
    for (int k = 0; k < VOX_MAX_PTS; k++) {
      if (k < p.max_pts) {
        const float val = k < occ ? pts[(size_t)best[k] * p.C + ch] : 0.f;
        if (voxels) voxels[((size_t)v * p.max_pts + k) * p.C + ch] = val;
        sacc += val;
      }
    }
    if (mean) mean[(size_t)v * p.C + ch] = sacc / (float)occ;
  }
}

// WIDE K5: point i goes to slot (number of its voxel's points with a smaller index) of its voxel's row, when that is below max_pts:
// the first max_pts points in input order, as the register list of the narrow kernel keeps them.  voxels is zero on entry.
__global__ __launch_bounds__(V3D_BLOCK) void vox_fill_wide_kernel(const float* __restrict__ pts, const VoxParams p,
                                                                  const int* __restrict__ pt_slot, const unsigned* __restrict__ first,
                                                                  const int* __restrict__ head, const int* __restrict__ next,
                                                                  const int* __restrict__ row_of_first, float* __restrict__ voxels) {
  const int i = blockIdx.x * V3D_BLOCK + threadIdx.x;
  if (i >= p.n_points) return;
  const int s = pt_slot[i];
  if (s < 0) return;
  const unsigned f = first[s];
  if (f >= (unsigned)p.n_points) return;
  const int v = row_of_first[f];
  if (v < 0) return;
  int rank = 0;
  for (int j = head[s], guard = 0; j >= 0 && guard < p.n_points; j = next[j], guard++) rank += j < i;
  if (rank >= p.max_pts) return;
  for (int ch = 0; ch < p.C; ch++) voxels[((size_t)v * p.max_pts + rank) * p.C + ch] = pts[(size_t)i * p.C + ch];
}

// WIDE K6: mean[v][ch] = (slot 0 + slot 1 + ... in order, the zero slots included) / occupancy -- the narrow kernel's sum.
__global__ __launch_bounds__(V3D_BLOCK) void vox_mean_wide_kernel(const float* __restrict__ voxels, const int* __restrict__ occupancy,
                                                                  const int* __restrict__ n_voxels, int rows_cap, int max_pts, int C,
                                                                  float* __restrict__ mean) {
  const long long total = (long long)min(*n_voxels, rows_cap) * C;
  for (long long t = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * V3D_BLOCK) {
    const int v = (int)(t / C), ch = (int)(t % C);
    float sacc = 0.f;
    for (int k = 0; k < max_pts; k++) sacc += voxels[((size_t)v * max_pts + k) * C + ch];
    mean[t] = sacc / (float)occupancy[v];
  }
}

// the kernels' parameter block from the host arguments (shared by the hard and the dynamic form)
static int vox_make_params(VoxParams& p, int n_points, int C, const int32_t* frame_offsets_host, int B, const float* voxel_size_host,
                           const float* bounds_host, int max_pts, int max_voxels) {
  for (int j = 0; j < 3; j++) {
    p.vs[j] = voxel_size_host[j];
    p.lo[j] = bounds_host[j];
    p.grid[j] = (int)lroundf((bounds_host[3 + j] - bounds_host[j]) / voxel_size_host[j]);
    if (p.grid[j] < 1) return V3D_EINVAL;
  }
  p.max_pts = max_pts;
  p.max_voxels = max_voxels;
  p.C = C;
  p.B = B;
  p.n_points = n_points;
  for (int b = 0; b <= B; b++) {
    p.frame_off[b] = frame_offsets_host[b];
    if (b > 0 && p.frame_off[b] < p.frame_off[b - 1]) return V3D_EINVAL;
  }
  return V3D_OK;
}

extern "C" size_t v3d_voxelize_workspace(int n_points) {
  const size_t n = (size_t)(n_points > 0 ? n_points : 1);
  const size_t cap = v3d_hash_capacity((long long)n);
  const size_t chunks = (n + VOX_CHUNK - 1) / VOX_CHUNK;
  return v3d_align(cap * 8) + 2 * v3d_align(cap * 4) + 2 * v3d_align(n * 4) + v3d_align(chunks * 4) +
         2 * v3d_align((VOX_MAX_FRAMES + 1) * 4) + v3d_align(n * 4) /*WIDE: row_of_first*/ + 256;
}

extern "C" int v3d_voxelize(const float* points, int n_points, int C, const int32_t* frame_offsets_host, int B,
                            const float* voxel_size_host, const float* bounds_host, int max_pts, int max_voxels,
                            float* voxels, int32_t* coords, int32_t* occupancy, float* mean, int32_t* n_voxels,
                            void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  return v3d_i_voxelize(points, n_points, C, frame_offsets_host, B, voxel_size_host, bounds_host, max_pts, max_voxels,
                        voxels, coords, occupancy, mean, n_voxels, workspace, workspace_bytes, 1, nullptr, nullptr,
                        (hipStream_t)stream);
}

// clear_tables = 0: the caller has already filled the head of the workspace (hash keys | first | head) with
// 0xFF, e.g. as part of one arena-wide memset (second_plan.hip).
int v3d_i_voxelize(const float* points, int n_points, int C, const int32_t* frame_offsets_host, int B,
                   const float* voxel_size_host, const float* bounds_host, int max_pts, int max_voxels, float* voxels,
                   int32_t* coords, int32_t* occupancy, float* mean, int32_t* n_voxels, void* workspace,
                   size_t workspace_bytes, int clear_tables, const V3dRbHash* site_hash, const int32_t* site_shape,
                   hipStream_t st) {
  if (n_points < 0 || C < 3 || B < 1 || B > VOX_MAX_FRAMES || max_pts < 1 || max_pts > VOX_MAX_PTS_WIDE || max_voxels < 1)
    return V3D_EINVAL;
  const bool wide = max_pts > VOX_MAX_PTS;
  if (wide && !voxels) return V3D_EUNSUPPORTED;  // (the mean of the wide path is summed from the point slots)
  if (!frame_offsets_host || !voxel_size_host || !bounds_host || !coords || !occupancy || !n_voxels) return V3D_EINVAL;
  if (frame_offsets_host[0] != 0 || frame_offsets_host[B] != n_points) return V3D_EINVAL;
  if (n_points == 0) {
    V3D_CHECK_HIP(v3d_fill_async(n_voxels, 0, sizeof(int32_t), st));
    return V3D_OK;
  }
  if (!points || !workspace) return V3D_EINVAL;
  if (site_hash && (long long)B * max_voxels > V3D_SITE_MAX_ROWS && n_points > V3D_SITE_MAX_ROWS) return V3D_EUNSUPPORTED;  // rows ride in 24 bits
  VoxParams p;
  {
    const int rcp = vox_make_params(p, n_points, C, frame_offsets_host, B, voxel_size_host, bounds_host, max_pts, max_voxels);
    if (rcp) return rcp;
  }
  const unsigned cap = v3d_hash_capacity(n_points);
  const int chunks = v3d_ceil_div(n_points, VOX_CHUNK);
  V3dArena ar(workspace, workspace_bytes);
  // keys | first | head are contiguous: ONE memset(0xFF) resets all three (EMPTY / UINT_MAX / -1)
  v3d_key_t* keys = ar.take<v3d_key_t>(cap);
  unsigned* first = ar.take<unsigned>(cap);
  int* head = ar.take<int>(cap);
  int* pt_slot = ar.take<int>(n_points);
  int* next = ar.take<int>(n_points);
  int* chunk_counts = ar.take<int>(chunks);
  int* frame_base = ar.take<int>(VOX_MAX_FRAMES + 1);
  int* out_base = ar.take<int>(VOX_MAX_FRAMES + 1);
  int* row_of_first = wide ? ar.take<int>(n_points) : (int*)nullptr;
  if (!ar.ok()) return V3D_EWORKSPACE;
  if (clear_tables) {
    V3D_CHECK_HIP(v3d_fill_async(keys, 0xFF, (size_t)((char*)head - (char*)keys) + (size_t)cap * 4, st));
    V3D_CHECK_HIP(v3d_fill_async(chunk_counts, 0xFF, (size_t)chunks * 4, st));  // -1 = "count not published yet"
  }
  V3dHash h = v3d_make_hash(keys, cap);
  const int ins_blocks = min(v3d_ceil_div(n_points, V3D_BLOCK), 2048);
  hipLaunchKernelGGL(vox_insert_kernel, dim3(ins_blocks), dim3(V3D_BLOCK), 0, st, points, p, h, first, head, pt_slot,
                     next);
  V3dHash sh = v3d_make_hash(site_hash ? site_hash->keys : keys, site_hash ? site_hash->hcap : cap);
  int* site_vals = (site_hash && site_shape) ? site_hash->vals : (int*)nullptr;
  const int sd = site_shape ? site_shape[0] : 0, shh = site_shape ? site_shape[1] : 0, sw = site_shape ? site_shape[2] : 0;
  if (wide) {
    const long long rows_cap = std::min<long long>(n_points, (long long)B * max_voxels);  // *n_voxels never exceeds either
    V3D_CHECK_HIP(v3d_fill_async(voxels, 0, (size_t)rows_cap * max_pts * C * sizeof(float), st));
    if (B == 1) {
      hipLaunchKernelGGL((vox_emit_kernel<true, true>), dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next,
                         chunk_counts, frame_base, out_base, voxels, coords, occupancy, mean, sh, site_vals, sd, shh, sw, n_voxels,
                         row_of_first);
    } else {
      hipLaunchKernelGGL(vox_count_scan_kernel, dim3(chunks), dim3(V3D_BLOCK), 0, st, pt_slot, first, p, chunk_counts, chunks,
                         frame_base, out_base, n_voxels);
      hipLaunchKernelGGL((vox_emit_kernel<false, true>), dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next,
                         chunk_counts, frame_base, out_base, voxels, coords, occupancy, mean, sh, site_vals, sd, shh, sw, n_voxels,
                         row_of_first);
    }
    hipLaunchKernelGGL(vox_fill_wide_kernel, dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next, row_of_first,
                       voxels);
    if (mean)
      hipLaunchKernelGGL(vox_mean_wide_kernel, dim3(std::min(v3d_ceil_div(rows_cap * C, V3D_BLOCK), 2048)), dim3(V3D_BLOCK), 0, st, voxels,
                         occupancy, n_voxels, (int)rows_cap, max_pts, C, mean);
    V3D_CHECK_LAUNCH();
    return V3D_OK;
  }
  if (B == 1) {  // one frame: count + scan + emit as a single-pass chained scan, 2 launches per voxelization instead of 3
    hipLaunchKernelGGL(vox_emit_kernel<true>, dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next,
                       chunk_counts, frame_base, out_base, voxels, coords, occupancy, mean, sh, site_vals, sd, shh, sw, n_voxels,
                       (int*)nullptr);
  } else {
    hipLaunchKernelGGL(vox_count_scan_kernel, dim3(chunks), dim3(V3D_BLOCK), 0, st, pt_slot, first, p, chunk_counts, chunks,
                       frame_base, out_base, n_voxels);
    hipLaunchKernelGGL(vox_emit_kernel<false>, dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next,
                       chunk_counts, frame_base, out_base, voxels, coords, occupancy, mean, sh, site_vals, sd, shh, sw, n_voxels,
                       (int*)nullptr);
  }
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// DYNAMIC voxelization (include/vision3d_hip.h "T1d"): every in-range point counts, no slot tensor.  K1 - K4 are the kernels above --
// K4 in its WIDE form with max_pts = INT_MAX: it counts its voxel's points (occupancy = the true count), records the voxel's row
// (row_of_first) and fills the site hash, and stores neither points nor a mean.  The mean is a sum of INTEGERS,
//   q = rint(double(v) * 2^24) (int64),  mean = float(double(sum q) / (double(k) * 2^24)),
// so neither the racy order of a voxel's list nor the order of atomics can show in it.  K5 is a thread per POINT: it finds its row
// (slot -> first toucher -> row_of_first) and writes point_voxel.  Two ways to form the sums, same bits:
//   ATOMIC  every point adds its terms into its row's accumulators with 64-bit integer atomics; K6, a thread per ROW, divides.
//           VOXDYN_G channels per pass (the accumulators are sized by n_points alone); K6 re-arms them for the next pass.
//   WALK    the first toucher walks its voxel's list with the sums in registers and divides: no accumulators, no K6.
// Measured (profiles/dynamic_voxelize.txt): the walk wins where voxels hold a few points (0.05 m voxels: a serial chase of 1 - 20
// nodes beats one atomic per point and channel), the atomics win where they hold hundreds (0.4 m pillars: one thread chases 300 nodes
// while its wave waits).  The occupancy is known by then, so the default, HYBRID, does each where it wins: voxels of at most
// VOXDYN_WALK_MAX points are walked, the points of larger ones add atomically.  v3d_voxelize_dynamic_variant picks (measurements).
#define VOXDYN_WALK_MAX 32
#define VOXDYN_G 4
#define VOXDYN_MAX_POINTS (1 << 22)
#define VOXDYN_LIMIT 65536.0f      // |v| < 2^16: a term is below 2^40, 2^22 of them stay inside int64
#define VOXDYN_SCALE 16777216.0    // 2^24

// the term of one value; false: not finite or out of range (contributes nothing, the mean becomes NaN)
__device__ __forceinline__ bool voxdyn_term(float v, long long& q) {
  if (!(fabsf(v) < VOXDYN_LIMIT)) return false;
  q = llrint((double)v * VOXDYN_SCALE);  // exact product, round half to even
  return true;
}
__device__ __forceinline__ float voxdyn_mean(long long sum, int k) { return (float)((double)sum / ((double)k * VOXDYN_SCALE)); }

// zeroes the accumulators (nvec 16-byte units, may be 0) and the status word
__global__ __launch_bounds__(V3D_BLOCK) void vox_dyn_zero_kernel(uint4* __restrict__ p, size_t nvec, int* __restrict__ status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
  for (size_t t = (size_t)blockIdx.x * V3D_BLOCK + threadIdx.x; t < nvec; t += (size_t)gridDim.x * V3D_BLOCK)
    p[t] = make_uint4(0u, 0u, 0u, 0u);
}

// row of point i (-1: out of bounds, or its voxel was cut by max_voxels); `opener`: i is its voxel's first toucher
__device__ __forceinline__ int voxdyn_row(const VoxParams& p, const int* pt_slot, const unsigned* first, const int* row_of_first, int i,
                                          int& slot, bool& opener) {
  opener = false;
  slot = pt_slot[i];
  if (slot < 0) return -1;
  const unsigned f = first[slot];
  if (f >= (unsigned)p.n_points) return -1;
  opener = f == (unsigned)i;
  return row_of_first[f];
}

// the first toucher of voxel row v (k points, hash slot `slot`) walks the voxel's list, VOXDYN_G channels per walk, and writes the mean
__device__ __forceinline__ void voxdyn_walk_voxel(const float* __restrict__ pts, const VoxParams& p, int slot, const int* __restrict__ head,
                                                  const int* __restrict__ next, int k, int v, float* __restrict__ mean,
                                                  int* __restrict__ status) {
  unsigned any = 0u;
  for (int c0 = 0; c0 < p.C; c0 += VOXDYN_G) {
    const int g = min(VOXDYN_G, p.C - c0);
    long long sum[VOXDYN_G] = {0ll, 0ll, 0ll, 0ll};
    unsigned refused = 0u;
    for (int j = head[slot], guard = 0; j >= 0 && guard < p.n_points; j = next[j], guard++) {
      float val[VOXDYN_G];
      if (p.C == 4) {
        const float4 q4 = reinterpret_cast<const float4*>(pts)[j];
        val[0] = q4.x; val[1] = q4.y; val[2] = q4.z; val[3] = q4.w;
      } else {
#pragma unroll
        for (int c = 0; c < VOXDYN_G; c++) val[c] = c < g ? pts[(size_t)j * p.C + c0 + c] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < VOXDYN_G; c++) {
        long long q;
        if (voxdyn_term(val[c], q)) sum[c] += q;
        else refused |= 1u << c;
      }
    }
    float m[VOXDYN_G];
#pragma unroll
    for (int c = 0; c < VOXDYN_G; c++) m[c] = (refused >> c & 1u) ? __builtin_nanf("") : voxdyn_mean(sum[c], k);
    if (p.C == 4) {
      reinterpret_cast<float4*>(mean)[v] = make_float4(m[0], m[1], m[2], m[3]);
    } else {
      for (int c = 0; c < g; c++) mean[(size_t)v * p.C + c0 + c] = m[c];
    }
    any |= refused & ((1u << g) - 1u);
  }
  if (any) atomicOr(status, 1);
}

// K5, a thread per POINT: its row (point_voxel, first pass only); a voxel of at most walk_max points is summed by its first toucher's
// walk (first pass, all channels); in a larger one every point adds channels [c0, c0 + VOXDYN_G) into acc[row][.], and bad[row] collects
// the channels that held a refused value.  walk_max = 0: atomics only; INT_MAX: walks only (acc and bad are not touched).
__global__ __launch_bounds__(V3D_BLOCK) void vox_dyn_point_kernel(const float* __restrict__ pts, const VoxParams p,
                                                                  const int* __restrict__ pt_slot, const unsigned* __restrict__ first,
                                                                  const int* __restrict__ head, const int* __restrict__ next,
                                                                  const int* __restrict__ row_of_first, const int* __restrict__ occupancy,
                                                                  int c0, int walk_max, unsigned long long* __restrict__ acc,
                                                                  unsigned* __restrict__ bad, float* __restrict__ mean,
                                                                  int* __restrict__ point_voxel /*nullable*/, int* __restrict__ status) {
  const int i = blockIdx.x * V3D_BLOCK + threadIdx.x;
  if (i >= p.n_points) return;
  int slot;
  bool opener;
  const int v = voxdyn_row(p, pt_slot, first, row_of_first, i, slot, opener);
  if (c0 == 0 && point_voxel) point_voxel[i] = v;
  if (v < 0) return;
  const int k = occupancy[v];
  if (k <= walk_max) {
    if (opener && c0 == 0) voxdyn_walk_voxel(pts, p, slot, head, next, k, v, mean, status);
    return;
  }
  float val[VOXDYN_G];
  const int g = min(VOXDYN_G, p.C - c0);
  if (p.C == 4) {
    const float4 q4 = reinterpret_cast<const float4*>(pts)[i];
    val[0] = q4.x; val[1] = q4.y; val[2] = q4.z; val[3] = q4.w;
  } else {
#pragma unroll
    for (int j = 0; j < VOXDYN_G; j++) val[j] = j < g ? pts[(size_t)i * p.C + c0 + j] : 0.f;
  }
  unsigned refused = 0u;
#pragma unroll
  for (int j = 0; j < VOXDYN_G; j++) {
    if (j >= g) continue;
    long long q;
    if (voxdyn_term(val[j], q)) atomicAdd(&acc[(size_t)v * VOXDYN_G + j], (unsigned long long)q);
    else refused |= 1u << j;
  }
  if (refused) atomicOr(&bad[v], refused);
}

// K6, a thread per ROW of more than walk_max points: divides its sums; rearm: leave the accumulators zero for the next pass
__global__ __launch_bounds__(V3D_BLOCK) void vox_dyn_mean_kernel(unsigned long long* __restrict__ acc, unsigned* __restrict__ bad,
                                                                 const int* __restrict__ occupancy, const int* __restrict__ n_voxels,
                                                                 int rows_cap, int C, int c0, int walk_max, int rearm,
                                                                 float* __restrict__ mean, int* __restrict__ status) {
  const int rows = min(*n_voxels, rows_cap), g = min(VOXDYN_G, C - c0);
  for (int v = blockIdx.x * V3D_BLOCK + threadIdx.x; v < rows; v += gridDim.x * V3D_BLOCK) {
    const int k = occupancy[v];
    if (k <= walk_max) continue;
    const unsigned refused = bad[v];
    float m[VOXDYN_G];
#pragma unroll
    for (int j = 0; j < VOXDYN_G; j++) {
      const long long sum = j < g ? (long long)acc[(size_t)v * VOXDYN_G + j] : 0ll;
      m[j] = (refused >> j & 1u) ? __builtin_nanf("") : voxdyn_mean(sum, k);
      if (rearm && j < g) acc[(size_t)v * VOXDYN_G + j] = 0ull;
    }
    if (C == 4) {
      reinterpret_cast<float4*>(mean)[v] = make_float4(m[0], m[1], m[2], m[3]);
    } else {
      for (int j = 0; j < g; j++) mean[(size_t)v * C + c0 + j] = m[j];
    }
    if (refused) {
      if (rearm) bad[v] = 0u;
      atomicOr(status, 1);
    }
  }
}

static int g_voxdyn_variant = V3D_VOXDYN_HYBRID;

extern "C" int v3d_voxelize_dynamic_variant(int variant) {
  const int prev = g_voxdyn_variant;
  if (variant >= V3D_VOXDYN_ATOMIC && variant <= V3D_VOXDYN_HYBRID) g_voxdyn_variant = variant;
  return prev;
}

size_t v3d_i_voxelize_dynamic_extra(int n_points) {
  const size_t n = (size_t)(n_points > 0 ? n_points : 1);
  return v3d_align(n * VOXDYN_G * 8) + v3d_align(n * 4) + 256;
}

extern "C" size_t v3d_voxelize_dynamic_workspace(int n_points) {
  return v3d_align(v3d_voxelize_workspace(n_points)) + v3d_i_voxelize_dynamic_extra(n_points);
}

extern "C" int v3d_voxelize_dynamic(const float* points, int n_points, int C, const int32_t* frame_offsets_host, int B,
                                    const float* voxel_size_host, const float* bounds_host, int max_voxels, int32_t* coords,
                                    int32_t* occupancy, float* mean, int32_t* point_voxel, int32_t* n_out, void* workspace,
                                    size_t workspace_bytes, v3d_stream_t stream) {
  if (!n_out) return V3D_EINVAL;
  const size_t base = v3d_align(v3d_voxelize_workspace(n_points));
  if (n_points > 0 && workspace && workspace_bytes < base) return V3D_EWORKSPACE;
  return v3d_i_voxelize_dynamic(points, n_points, C, frame_offsets_host, B, voxel_size_host, bounds_host, max_voxels, coords, occupancy,
                                mean, point_voxel, n_out, n_out + 1, workspace, base, workspace ? (char*)workspace + base : nullptr,
                                workspace_bytes > base ? workspace_bytes - base : 0, 1, nullptr, nullptr, -1, (hipStream_t)stream);
}

int v3d_i_voxelize_dynamic(const float* points, int n_points, int C, const int32_t* frame_offsets_host, int B,
                           const float* voxel_size_host, const float* bounds_host, int max_voxels, int32_t* coords,
                           int32_t* occupancy, float* mean, int32_t* point_voxel, int32_t* n_voxels, int32_t* status, void* workspace,
                           size_t workspace_bytes, void* extra, size_t extra_bytes, int clear_tables, const V3dRbHash* site_hash,
                           const int32_t* site_shape, int variant, hipStream_t st) {
  if (n_points < 0 || C < 3 || B < 1 || B > VOX_MAX_FRAMES || max_voxels < 1) return V3D_EINVAL;
  if (!frame_offsets_host || !voxel_size_host || !bounds_host || !coords || !occupancy || !mean || !n_voxels || !status)
    return V3D_EINVAL;
  if (frame_offsets_host[0] != 0 || frame_offsets_host[B] != n_points) return V3D_EINVAL;
  // the range the integer sums are exact in (a point inside the bounds then has in-range coordinates)
  if (n_points > VOXDYN_MAX_POINTS) return V3D_EUNSUPPORTED;
  for (int j = 0; j < 6; j++)
    if (!(fabsf(bounds_host[j]) < VOXDYN_LIMIT)) return V3D_EUNSUPPORTED;
  if (variant < 0) variant = g_voxdyn_variant;
  if (variant < V3D_VOXDYN_ATOMIC || variant > V3D_VOXDYN_HYBRID) return V3D_EINVAL;
  if (n_points == 0) {
    V3D_CHECK_HIP(v3d_fill_async(n_voxels, 0, sizeof(int32_t), st));
    V3D_CHECK_HIP(v3d_fill_async(status, 0, sizeof(int32_t), st));
    return V3D_OK;
  }
  if (!points || !workspace || !extra) return V3D_EINVAL;
  if (site_hash && (long long)B * max_voxels > V3D_SITE_MAX_ROWS && n_points > V3D_SITE_MAX_ROWS) return V3D_EUNSUPPORTED;  // rows ride in 24 bits
  VoxParams p;
  {
    const int rcp = vox_make_params(p, n_points, C, frame_offsets_host, B, voxel_size_host, bounds_host, 0x7FFFFFFF, max_voxels);
    if (rcp) return rcp;
  }
  const unsigned cap = v3d_hash_capacity(n_points);
  const int chunks = v3d_ceil_div(n_points, VOX_CHUNK);
  const long long rows_cap = std::min<long long>(n_points, (long long)B * max_voxels);  // *n_voxels never exceeds either
  V3dArena ar(workspace, workspace_bytes);  // (the layout of v3d_i_voxelize: its callers' 0xFF fill covers the same tables)
  v3d_key_t* keys = ar.take<v3d_key_t>(cap);
  unsigned* first = ar.take<unsigned>(cap);
  int* head = ar.take<int>(cap);
  int* pt_slot = ar.take<int>(n_points);
  int* next = ar.take<int>(n_points);
  int* chunk_counts = ar.take<int>(chunks);
  int* frame_base = ar.take<int>(VOX_MAX_FRAMES + 1);
  int* out_base = ar.take<int>(VOX_MAX_FRAMES + 1);
  int* row_of_first = ar.take<int>(n_points);
  V3dArena ex(extra, extra_bytes);
  unsigned long long* acc = ex.take<unsigned long long>((size_t)rows_cap * VOXDYN_G);
  unsigned* bad = ex.take<unsigned>((size_t)rows_cap);
  if (!ar.ok() || !ex.ok()) return V3D_EWORKSPACE;
  if (clear_tables) {
    V3D_CHECK_HIP(v3d_fill_async(keys, 0xFF, (size_t)((char*)head - (char*)keys) + (size_t)cap * 4, st));
    V3D_CHECK_HIP(v3d_fill_async(chunk_counts, 0xFF, (size_t)chunks * 4, st));  // -1 = "count not published yet"
  }
  {  // the status word, and for the atomic form the accumulators (acc | bad are contiguous)
    const size_t nvec = variant != V3D_VOXDYN_WALK ? (size_t)((char*)bad - (char*)acc + v3d_align((size_t)rows_cap * 4)) / 16 : 0;
    const int zb = (int)std::min<size_t>(std::max<size_t>((nvec + V3D_BLOCK - 1) / V3D_BLOCK, 1), 2048);
    hipLaunchKernelGGL(vox_dyn_zero_kernel, dim3(zb), dim3(V3D_BLOCK), 0, st, (uint4*)acc, nvec, status);
  }
  V3dHash h = v3d_make_hash(keys, cap);
  const int ins_blocks = min(v3d_ceil_div(n_points, V3D_BLOCK), 2048);
  hipLaunchKernelGGL(vox_insert_kernel, dim3(ins_blocks), dim3(V3D_BLOCK), 0, st, points, p, h, first, head, pt_slot, next);
  V3dHash sh = v3d_make_hash(site_hash ? site_hash->keys : keys, site_hash ? site_hash->hcap : cap);
  int* site_vals = (site_hash && site_shape) ? site_hash->vals : (int*)nullptr;
  const int sd = site_shape ? site_shape[0] : 0, shh = site_shape ? site_shape[1] : 0, sw = site_shape ? site_shape[2] : 0;
  if (B == 1) {
    hipLaunchKernelGGL((vox_emit_kernel<true, true>), dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next,
                       chunk_counts, frame_base, out_base, (float*)nullptr, coords, occupancy, (float*)nullptr, sh, site_vals, sd, shh, sw,
                       n_voxels, row_of_first);
  } else {
    hipLaunchKernelGGL(vox_count_scan_kernel, dim3(chunks), dim3(V3D_BLOCK), 0, st, pt_slot, first, p, chunk_counts, chunks, frame_base,
                       out_base, n_voxels);
    hipLaunchKernelGGL((vox_emit_kernel<false, true>), dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next,
                       chunk_counts, frame_base, out_base, (float*)nullptr, coords, occupancy, (float*)nullptr, sh, site_vals, sd, shh, sw,
                       n_voxels, row_of_first);
  }
  {
    const int walk_max = variant == V3D_VOXDYN_WALK ? 0x7FFFFFFF : variant == V3D_VOXDYN_HYBRID ? VOXDYN_WALK_MAX : 0;
    const int mean_blocks = (int)std::min<long long>(v3d_ceil_div(rows_cap, V3D_BLOCK), 2048);
    for (int c0 = 0; c0 < C; c0 += VOXDYN_G) {
      hipLaunchKernelGGL(vox_dyn_point_kernel, dim3(chunks), dim3(V3D_BLOCK), 0, st, points, p, pt_slot, first, head, next, row_of_first,
                         occupancy, c0, walk_max, acc, bad, mean, point_voxel, status);
      if (variant == V3D_VOXDYN_WALK) break;  // (the walks took every channel)
      hipLaunchKernelGGL(vox_dyn_mean_kernel, dim3(mean_blocks), dim3(V3D_BLOCK), 0, st, acc, bad, occupancy, n_voxels, (int)rows_cap, C,
                         c0, walk_max, c0 + VOXDYN_G < C ? 1 : 0, mean, status);
    }
  }
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
