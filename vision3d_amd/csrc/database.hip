// database.hip -- the objects of the GT-sampling database cut out of a BATCH of annotated frames in THREE launches.
//
// Replaces DatabaseBuilder._process_item / _demean (vision3d/dataset/augmentation.py:201-243) with its PointsInCuboids call
// (vision3d/core/geometry.py:27-48), which the reference runs in numpy per frame: an (N, G) mask, G boolean gathers, G
// subtractions.  Here every frame's points are tested against that frame's boxes and each kept box's points leave, in point
// order, de-meaned, in the concatenated layout SampleDatabase keeps (rows of box 0, rows of box 1, ...; boxes in annotation
// order, frames in batch order).  A box is kept iff it holds MORE than min_pts points (:232-234); a point inside two boxes
// goes to both.
//   db_count_kernel   a workgroup per 2 048-point chunk of ONE frame, a wave per 512 consecutive points (8 rounds of 64):
//       the frame's boxes in LDS, ballot + popcount per (box, wave) -> seg[chunk][wave][box]
//   db_scan_kernel    a workgroup per frame, a thread per box: running sum over the frame's (chunk, wave) counts written back
//       in place (first row of each segment inside its box), counts[box], the kept boxes' first rows inside the frame
//   db_emit_kernel    the count kernel's grid again: the test repeated, rank inside the wave from the ballot, row = rows of the
//       earlier frames + first row of the box inside the frame + first row of the segment inside the box + rank
// No workgroup waits on another and no atomic decides a position, so the result is a pure function of the inputs.  The frame
// and chunk of a workgroup follow from the device-side offsets (db_locate: a block scan over the frames' chunk counts), so the
// entry point reads nothing back; the grid is sized for the worst case (every frame ends in a partial chunk).
// The inside test is pib_inside in float64 throughout (annotation boxes are float64 upstream, kitti_dataset.py:75-79; numpy then
// promotes the float32 points).  cos / sin of the yaw and z -+ h / 2 arrive evaluated by the host in numpy (box_prep rows): the
// device's double cos / sin need not equal the host libm's, and a corner one ulp off flips a point that lies on an edge.
#include "v3d_common.h"
#include "pib_device.h"

#define DB_MAX_BOXES V3D_DATABASE_MAX_BOXES
#define DB_ROUNDS 8
#define DB_WAVE_POINTS (DB_ROUNDS * V3D_WAVE)                      // 512
#define DB_WAVES (V3D_BLOCK / V3D_WAVE)                            // 4
#define DB_CHUNK (DB_WAVES * DB_WAVE_POINTS)                       // 2 048
#define DB_FLAG_OVERFLOW 1
#define DB_FLAG_LIMIT 2

// int32 work area: flag[4] (word 0: DB_FLAG_LIMIT when a frame broke a limit), frame_rows[F], frame_kept[F], rel_start[n_boxes],
// seg[n_chunks][DB_WAVES][DB_MAX_BOXES]
struct DbWork {
  int *flag, *frame_rows, *frame_kept, *rel_start, *seg;
  int n_chunks;
  size_t bytes;
};
static __host__ __device__ inline DbWork db_work(void* base, int n_points, int n_boxes, int n_frames) {
  DbWork w;
  int* p = (int*)base;
  w.flag = p;
  w.frame_rows = p + 4;
  w.frame_kept = w.frame_rows + n_frames;
  w.rel_start = w.frame_kept + n_frames;
  w.seg = w.rel_start + n_boxes;
  w.n_chunks = (int)(((long long)n_points + DB_CHUNK - 1) / DB_CHUNK) + n_frames;  // every frame: at least one, at most one partial
  w.bytes = 4 * ((size_t)4 + 2 * (size_t)n_frames + (size_t)n_boxes + (size_t)w.n_chunks * DB_WAVES * DB_MAX_BOXES);
  return w;
}

__device__ __forceinline__ int db_chunks(int n) { return n <= 0 ? 1 : (n + DB_CHUNK - 1) / DB_CHUNK; }

// inclusive scan of one int per thread over the 256-thread block, with the barrier behind it: `lds` >= 4 ints, free on return
__device__ __forceinline__ int db_block_scan(int v, int& total, int* lds) {
  const int incl = v3d_block_scan_incl<DB_WAVES>(v, total, lds);
  __syncthreads();
  return incl;
}

// sum over i < n of value(i), to every thread
template <typename F>
__device__ __forceinline__ int db_block_sum(int n, int* lds, F value) {
  int part = 0, total;
  for (int i = threadIdx.x; i < n; i += V3D_BLOCK) part += value(i);
  db_block_scan(part, total, lds);
  return total;
}

// frame f and chunk c (inside f) of workgroup b; false for the workgroups behind the last chunk.  `lds` >= 8 ints.
__device__ __forceinline__ bool db_locate(const int* __restrict__ point_offsets, int F, int b, int* lds, int& f, int& c) {
  const int tid = threadIdx.x;
  if (tid == 0) lds[4] = -1;
  int carry = 0;
  for (int t0 = 0; t0 < F; t0 += V3D_BLOCK) {
    const int idx = t0 + tid;
    const int n = idx < F ? db_chunks(point_offsets[idx + 1] - point_offsets[idx]) : 0;
    int total;
    const int excl = carry + db_block_scan(n, total, lds) - n;  // (the scan's barriers order the store of -1 above before these)
    if (idx < F && excl <= b && b < excl + n) {
      lds[4] = idx;
      lds[5] = b - excl;
    }
    carry += total;
    if (carry > b) break;
  }
  __syncthreads();
  f = lds[4];
  c = lds[5];
  __syncthreads();
  return f >= 0;
}

struct DbFrame {
  int p_lo, p_hi, g0, G;
  bool ok;  // offsets inside the arrays, at most DB_MAX_BOXES boxes
};
__device__ __forceinline__ DbFrame db_frame(const int* __restrict__ point_offsets, const int* __restrict__ box_offsets, int f, int n_points,
                                            int n_boxes) {
  DbFrame fr;
  fr.p_lo = point_offsets[f];
  fr.p_hi = point_offsets[f + 1];
  fr.g0 = box_offsets[f];
  fr.G = box_offsets[f + 1] - fr.g0;
  fr.ok = fr.p_lo >= 0 && fr.p_hi >= fr.p_lo && fr.p_hi <= n_points && fr.g0 >= 0 && fr.G >= 0 && fr.g0 + fr.G <= n_boxes &&
          fr.G <= DB_MAX_BOXES;
  return fr;
}

// the 8 points of a lane: row base + 64 r + lane of `points`, NaN behind the frame's end (inside no box)
template <bool C4>
__device__ __forceinline__ void db_load_points(const float* __restrict__ points, int C, int base, int p_hi, float (&x)[DB_ROUNDS],
                                               float (&y)[DB_ROUNDS], float (&z)[DB_ROUNDS], float (&q)[DB_ROUNDS]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < DB_ROUNDS; r++) {
    const int i = base + r * V3D_WAVE + lane;
    x[r] = y[r] = z[r] = __builtin_nanf("");
    q[r] = 0.f;
    if (i < p_hi) {
      if (C4) {
        const float4 p = reinterpret_cast<const float4*>(points)[i];
        x[r] = p.x, y[r] = p.y, z[r] = p.z, q[r] = p.w;
      } else {
        const float* p = points + (size_t)i * C;
        x[r] = p[0], y[r] = p[1], z[r] = p[2];
      }
    }
  }
}

template <bool C4>
__global__ __launch_bounds__(V3D_BLOCK) void db_count_kernel(const float* __restrict__ points, int C, const int* __restrict__ point_offsets,
                                                             int n_points, const double* __restrict__ box_prep,
                                                             const int* __restrict__ box_offsets, int n_boxes, int F, void* work) {
  __shared__ PibBoxD sb[DB_MAX_BOXES];
  __shared__ int lds[8];
  const DbWork w = db_work(work, n_points, n_boxes, F);
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  if (b == 0 && tid == 0) w.flag[0] = 0;  // (db_scan_kernel raises it, db_emit_kernel reads it)
  int f, c;
  if (!db_locate(point_offsets, F, b, lds, f, c)) return;
  const DbFrame fr = db_frame(point_offsets, box_offsets, f, n_points, n_boxes);
  if (!fr.ok || fr.G == 0) return;
  if (tid < fr.G) sb[tid] = pib_prep_row(box_prep + 8 * (size_t)(fr.g0 + tid));
  __syncthreads();
  float x[DB_ROUNDS], y[DB_ROUNDS], z[DB_ROUNDS], q[DB_ROUNDS];
  db_load_points<C4>(points, C, fr.p_lo + c * DB_CHUNK + wave * DB_WAVE_POINTS, fr.p_hi, x, y, z, q);
  int* row = w.seg + ((size_t)b * DB_WAVES + wave) * DB_MAX_BOXES;
  for (int gb = 0; gb < fr.G; gb += V3D_WAVE) {  // lane j keeps the count of box gb + j: one coalesced store per 64 boxes
    const int ng = min(V3D_WAVE, fr.G - gb);
    int mine = 0;
    for (int j = 0; j < ng; j++) {
      const PibBoxD& pb = sb[gb + j];
      int cnt = 0;
#pragma unroll
      for (int r = 0; r < DB_ROUNDS; r++) cnt += __popcll(__ballot(pib_inside(pb, x[r], y[r], z[r], true)));
      if (lane == j) mine = cnt;
    }
    if (lane < ng) row[gb + lane] = mine;
  }
}

__global__ __launch_bounds__(V3D_BLOCK) void db_scan_kernel(const int* __restrict__ point_offsets, int n_points, const int* __restrict__ box_offsets,
                                                            int n_boxes, int F, int min_pts, int* __restrict__ counts, int* __restrict__ starts,
                                                            void* work) {
  __shared__ int lds[8];
  const DbWork w = db_work(work, n_points, n_boxes, F);
  const int tid = threadIdx.x, f = blockIdx.x;
  const int chunk_base = db_block_sum(f, lds, [&](int i) { return db_chunks(point_offsets[i + 1] - point_offsets[i]); });
  const DbFrame fr = db_frame(point_offsets, box_offsets, f, n_points, n_boxes);
  if (!fr.ok) {  // nothing of this frame is extracted; its boxes (where the offsets can be trusted) read "empty, dropped"
    if (fr.g0 >= 0 && fr.G >= 0 && fr.g0 + fr.G <= n_boxes)
      for (int g = tid; g < fr.G; g += V3D_BLOCK) counts[fr.g0 + g] = 0, starts[fr.g0 + g] = -1, w.rel_start[fr.g0 + g] = -1;
    if (tid == 0) w.flag[0] = DB_FLAG_LIMIT, w.frame_rows[f] = 0, w.frame_kept[f] = 0;
    return;
  }
  int run = 0;
  if (tid < fr.G) {
    const long long first = (long long)chunk_base * DB_WAVES, last = min(first + (long long)db_chunks(fr.p_hi - fr.p_lo) * DB_WAVES,
                                                                          (long long)w.n_chunks * DB_WAVES);
    for (long long s = max(first, 0LL); s < last; s++) {  // (the clamps only matter for offsets that do not tile the point array)
      int* p = w.seg + (size_t)s * DB_MAX_BOXES + tid;
      const int v = *p;
      *p = run;
      run += v;
    }
    counts[fr.g0 + tid] = run;
  }
  const bool keep = tid < fr.G && run > min_pts;
  int rows, kept;
  const int incl = db_block_scan(keep ? run : 0, rows, lds);
  db_block_scan(keep ? 1 : 0, kept, lds);
  if (tid < fr.G) w.rel_start[fr.g0 + tid] = keep ? incl - run : -1;
  if (tid == 0) w.frame_rows[f] = rows, w.frame_kept[f] = kept;
}

template <bool C4>
__global__ __launch_bounds__(V3D_BLOCK) void db_emit_kernel(const float* __restrict__ points, int C, const int* __restrict__ point_offsets,
                                                            int n_points, const double* __restrict__ box_prep,
                                                            const int* __restrict__ box_offsets, int n_boxes, int F, int* __restrict__ starts,
                                                            int* __restrict__ src_index, float* __restrict__ out_points, long long cap,
                                                            int* __restrict__ totals, void* work) {
  __shared__ PibBoxD sb[DB_MAX_BOXES];
  __shared__ int first_row[DB_WAVES][DB_MAX_BOXES];
  __shared__ int lds[8];
  const DbWork w = db_work(work, n_points, n_boxes, F);
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  if (b == 0) {
    const int rows = db_block_sum(F, lds, [&](int i) { return w.frame_rows[i]; });
    const int kept = db_block_sum(F, lds, [&](int i) { return w.frame_kept[i]; });
    if (tid == 0) totals[0] = kept, totals[1] = rows, totals[2] = ((long long)rows > cap ? DB_FLAG_OVERFLOW : 0) | w.flag[0];
  }
  int f, c;
  if (!db_locate(point_offsets, F, b, lds, f, c)) return;
  const DbFrame fr = db_frame(point_offsets, box_offsets, f, n_points, n_boxes);
  if (!fr.ok || fr.G == 0) return;
  const int base = db_block_sum(f, lds, [&](int i) { return w.frame_rows[i]; });
  if (tid < fr.G) {
    const int rel = w.rel_start[fr.g0 + tid];
    if (c == 0) starts[fr.g0 + tid] = rel < 0 ? -1 : base + rel;
#pragma unroll
    for (int wv = 0; wv < DB_WAVES; wv++)
      first_row[wv][tid] = rel < 0 ? -1 : base + rel + w.seg[((size_t)b * DB_WAVES + wv) * DB_MAX_BOXES + tid];
    sb[tid] = pib_prep_row(box_prep + 8 * (size_t)(fr.g0 + tid));
  }
  __syncthreads();
  float x[DB_ROUNDS], y[DB_ROUNDS], z[DB_ROUNDS], q[DB_ROUNDS];
  const int p0 = fr.p_lo + c * DB_CHUNK + wave * DB_WAVE_POINTS;
  db_load_points<C4>(points, C, p0, fr.p_hi, x, y, z, q);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int g = 0; g < fr.G; g++) {
    long long row0 = first_row[wave][g];
    if (row0 < 0) continue;  // dropped (wave-uniform)
    const PibBoxD& pb = sb[g];
    const double bx = box_prep[8 * (size_t)(fr.g0 + g) + 2], by = box_prep[8 * (size_t)(fr.g0 + g) + 3];
#pragma unroll
    for (int r = 0; r < DB_ROUNDS; r++) {
      const bool in = pib_inside(pb, x[r], y[r], z[r], true);
      const unsigned long long m = __ballot(in);
      const long long row = row0 + __popcll(m & below);
      if (in && row < cap) {  // (augmentation.py:219-227: xy - centre in float64; the database keeps float32)
        const int i = p0 + r * V3D_WAVE + lane;
        const float ox = (float)((double)x[r] - bx), oy = (float)((double)y[r] - by);
        if (C4) {
          reinterpret_cast<float4*>(out_points)[row] = make_float4(ox, oy, z[r], q[r]);
        } else {
          float* o = out_points + (size_t)row * C;
          const float* p = points + (size_t)i * C;
          o[0] = ox, o[1] = oy, o[2] = z[r];
          for (int col = 3; col < C; col++) o[col] = p[col];
        }
        src_index[row] = i;
      }
      row0 += __popcll(m);
    }
  }
}

extern "C" size_t v3d_database_work_bytes(int n_points, int n_boxes, int n_frames) {
  if (n_points < 0 || n_boxes < 0 || n_frames < 0) return 0;
  return db_work(nullptr, n_points, n_boxes, n_frames).bytes;
}

extern "C" int v3d_database_extract(const float* points, int n_points, int C, const int32_t* point_offsets, const double* box_prep,
                                    int n_boxes, const int32_t* box_offsets, int n_frames, int min_pts, int32_t* counts, int32_t* starts,
                                    int32_t* src_index, float* out_points, int64_t cap, int32_t* totals, void* work, size_t work_bytes,
                                    v3d_stream_t stream) {
  if (n_points < 0 || n_boxes < 0 || n_frames < 0 || C < 3 || cap < 0 || !totals) return V3D_EINVAL;
  if ((long long)n_points + (long long)n_frames * DB_CHUNK > 0x7fffffffLL) return V3D_EUNSUPPORTED;  // row and chunk indices are int32
  hipStream_t st = (hipStream_t)stream;
  if (n_frames == 0) {
    if (n_points || n_boxes) return V3D_EINVAL;
    V3D_CHECK_HIP(v3d_fill_async(totals, 0, 3 * sizeof(int32_t), st));
    return V3D_OK;
  }
  if ((long long)n_boxes > (long long)DB_MAX_BOXES * n_frames) return V3D_EUNSUPPORTED;  // some frame holds more than DB_MAX_BOXES
  if (!point_offsets || !box_offsets || !work || (n_points && !points) || (n_boxes && (!box_prep || !counts || !starts)) ||
      (cap && (!out_points || !src_index)))
    return V3D_EINVAL;
  const DbWork w = db_work(nullptr, n_points, n_boxes, n_frames);
  if (work_bytes < w.bytes) return V3D_EWORKSPACE;
  if (((uintptr_t)work & 3) || ((uintptr_t)box_prep & 7)) return V3D_EINVAL;
  const bool c4 = C == 4 && !((uintptr_t)points & 15) && !((uintptr_t)out_points & 15);
  const dim3 grid(w.n_chunks), block(V3D_BLOCK);
  if (c4)
    hipLaunchKernelGGL(db_count_kernel<true>, grid, block, 0, st, points, C, point_offsets, n_points, box_prep, box_offsets, n_boxes, n_frames, work);
  else
    hipLaunchKernelGGL(db_count_kernel<false>, grid, block, 0, st, points, C, point_offsets, n_points, box_prep, box_offsets, n_boxes, n_frames, work);
  V3D_CHECK_LAUNCH();
  hipLaunchKernelGGL(db_scan_kernel, dim3(n_frames), block, 0, st, point_offsets, n_points, box_offsets, n_boxes, n_frames, min_pts, counts,
                     starts, work);
  V3D_CHECK_LAUNCH();
  if (c4)
    hipLaunchKernelGGL(db_emit_kernel<true>, grid, block, 0, st, points, C, point_offsets, n_points, box_prep, box_offsets, n_boxes, n_frames,
                       starts, src_index, out_points, (long long)cap, totals, work);
  else
    hipLaunchKernelGGL(db_emit_kernel<false>, grid, block, 0, st, points, C, point_offsets, n_points, box_prep, box_offsets, n_boxes, n_frames,
                       starts, src_index, out_points, (long long)cap, totals, work);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
