// kitti_eval.hip -- KITTI 2-D bbox, BEV and 3-D average precision and AOS on the device (vision3d_amd/evaluation/kitti.py
// states the protocol).
//
// All frames go in one ragged batch (include/vision3d_hip.h "KITTI 2-D bbox, BEV and 3-D average precision"); one combo array
// covers every metric, and a combo reads the overlap plane ov + metric * ov_plane (0 BEV, 1 3-D, 2 bbox).  Whatever the frame
// count, no host reads in between:
//   1. overlaps        one workgroup per (frame, chunk of 256 detection rows): the frame's ground truths are prepped into LDS
//                      once, each lane preps its detection once and clips it against every ground truth with the rotated-IoU
//                      core (rotated_iou.h, clipper work arrays in per-wave LDS slabs); BEV and 3-D IoU come from the same
//                      intersection;
//      overlaps_image  (bbox) the same grid: 2-D IoU of (x1, y1, x2, y2) image boxes in double into the bbox plane;
//   2. pass 1          one wave per (frame, combo): ground truths in file order, lanes split the detection scan, a wave argmax
//                      (score, then earliest index) picks the match; true-positive scores are appended through an atomic cursor;
//   3. thresholds      one lane per combo walks its descending TP scores in double (the 41-point recall sampling);
//   4. pass 2          one wave per (frame, combo), one lane per threshold: each lane runs its own greedy assignment with an
//                      "assigned" bitmask in LDS and adds integer (tp, fp, fn) with global atomics (order-free, deterministic);
//                      bbox combos add the DontCare step (unassigned counted detections whose inter / area_dt with a DontCare
//                      region exceeds the minimum overlap are no false positives) and each lane's true-positive similarity sum
//                      (1 + cos(alpha_gt - alpha_dt)) / 2 in double, added as 32.32 fixed point with 64-bit integer atomics;
//      pass 2 family   (kitti_pass2_family_kernel) the combos that differ only in min_overlap (a "family": the levels of a COCO-style
//                      sweep, with the official combos of the same class, neighbour, difficulty and metric) of KE_FAMILY_MIN or
//                      more: one workgroup per (frame, family), one wave per level, one lane per threshold; the frame's scores,
//                      ignored_dt and ignored_gt are staged into LDS once, and its overlap tile too when it fits.  The same rule
//                      (ke_pass2_lane) on the same data: counts and similarity are bit-identical to the generic kernel's;
//   5. ap              one lane per combo: precision (and with the similarity, similarity / (tp + fp)), its running maximum
//                      from the right, R11 / R40 sums in definition order.
// Combos reach the kernels by value, KE_CHUNK per launch: pass 1 and the generic pass 2 launch once per chunk of 64 combos, the
// family pass 2 once per KE_FAM_CHUNK families; the thresholds and AP kernels take a grid of ceil(n / 64) waves.  Launch counts
// depend on the combos, never on the frame count.
// Limits: 1 024 detections (16 bitmask words per lane in pass 2, 16 register bits per lane in pass 1) and 256 ground truths
// (one LDS slot per thread in stage 1) per frame.
#include "v3d_common.h"
#include "rotated_iou.h"

#include <algorithm>
#include <vector>

using v3d::BoxPrep;

#define KE_NT V3D_KITTI_SAMPLE_PTS
#define KE_WORDS (V3D_KITTI_MAX_DT / 64)
#define KE_DONTCARE_BIT V3D_KITTI_DONTCARE_BIT  // gt_meta[1] (ignored_gt reads bits 0-2 only)

#define KE_CHUNK V3D_KITTI_COMBO_CHUNK  // combos per by-value table (one pass-1 / generic pass-2 launch)
#ifndef KE_FAMILY_MIN
#define KE_FAMILY_MIN 3  // families of fewer combos (the official strict / loose pairs) stay on the generic pass 2
#endif
#define KE_FAM_LEVELS 12        // combos per family (one wave each): ten sweep levels + strict + loose
#define KE_FAM_CHUNK 16         // families per by-value table (one family pass-2 launch)
#define KE_FAM_LDS (64 * 1024)  // the family kernel's LDS budget: bitmasks, staged detections, ground truths, overlap tile

struct KeCombos {
  v3d_kitti_combo c[KE_CHUNK];
};
// One family: the shared (class, neighbour, difficulty, metric) in c (its min_overlap unused), and per level the combo index
// (row of thresholds, n_thresholds, counts, similarity) and its min_overlap.
struct KeFamily {
  v3d_kitti_combo c;
  int n;
  int combo[KE_FAM_LEVELS];
  float level[KE_FAM_LEVELS];
};
struct KeFamilies {
  KeFamily f[KE_FAM_CHUNK];
};

// A rectified-camera box (x, y_bottom, z, h, w, l, ry): the BEV rectangle in the (x, z) plane -- the core's extent `w` (along
// its heading (cos a, sin a)) is the box length l, its angle a = -ry turns the heading to (cos ry, -sin ry) -- plus the
// vertical extent [y_bottom - h, y_bottom] (y points down) and the volume.
struct CamPrep {
  BoxPrep bev;
  float ytop, ybot, vol;
};
__device__ __forceinline__ CamPrep prep_cam(const float* b) {
  const float bev[5] = {b[0], b[2], b[5], b[4], -b[6] * 57.29577951308232f};
  CamPrep r;
  r.bev = v3d::prep_box(bev);
  r.ybot = b[1];
  r.ytop = b[1] - b[3];
  r.vol = b[5] * b[4] * b[3];
  return r;
}

__global__ __launch_bounds__(V3D_BLOCK) void kitti_overlaps_kernel(const float* __restrict__ gt, const int* __restrict__ gt_off,
                                                                   const float* __restrict__ dt, const int* __restrict__ dt_off,
                                                                   const int64_t* __restrict__ ov_off, float* __restrict__ ov_bev,
                                                                   float* __restrict__ ov_3d) {
  __shared__ CamPrep gts[V3D_KITTI_MAX_GT];
  __shared__ v3d::P2 clip_pts[V3D_BLOCK / V3D_WAVE][24 * 64];  // the clipper's work arrays: LDS, not scratch (rotated_iou.h)
  __shared__ float clip_dist[V3D_BLOCK / V3D_WAVE][24 * 64];
  const int f = blockIdx.x;
  const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
  const int d0 = dt_off[f], nd = dt_off[f + 1] - d0;
  if (ng <= 0 || nd <= 0 || ng > V3D_KITTI_MAX_GT || nd > V3D_KITTI_MAX_DT) return;  // (block-uniform)
  if ((int)threadIdx.x < ng) gts[threadIdx.x] = prep_cam(gt + 7 * (size_t)(g0 + threadIdx.x));
  __syncthreads();
  const int j = blockIdx.y * V3D_BLOCK + threadIdx.x;
  if (j >= nd) return;
  const CamPrep d = prep_cam(dt + 8 * (size_t)(d0 + j));
  v3d::P2* pts = clip_pts[threadIdx.x >> 6] + (threadIdx.x & 63);
  float* dist = clip_dist[threadIdx.x >> 6] + (threadIdx.x & 63);
  const size_t row = (size_t)ov_off[f] + (size_t)j * ng;
  for (int i = 0; i < ng; i++) {
    const CamPrep& g = gts[i];
    float bev = 0.f, iou3 = 0.f;
    if (v3d::iou_needs_clip(d.bev, g.bev)) {
      const float inter = v3d::inter_prepped_lds(d.bev, g.bev, pts, dist);
      bev = inter / (d.bev.area + g.bev.area - inter);
      const float oh = fmaxf(fminf(d.ybot, g.ybot) - fmaxf(d.ytop, g.ytop), 0.f);
      const float inter3 = inter * oh;
      const float den = d.vol + g.vol - inter3;
      iou3 = den > 0.f ? inter3 / den : 0.f;
    }
    ov_bev[row + i] = bev;
    ov_3d[row + i] = iou3;
  }
}

// ignored_gt: 0 counted, 1 ignored (neighbour class, or the class outside the difficulty), -1 not part of the combo
__device__ __forceinline__ int ignored_gt(const int* meta, const v3d_kitti_combo& c) {
  const int code = meta[0];
  const bool ign = (meta[1] >> c.difficulty) & 1;
  if (code == c.cls) return ign ? 1 : 0;
  return code == c.neighbour ? 1 : -1;
}
// ignored_dt: 1 too short (first, whatever the class), 0 the class, -1 another class
__device__ __forceinline__ int ignored_dt(const int* meta, const v3d_kitti_combo& c) {
  if ((meta[1] >> c.difficulty) & 1) return 1;
  return meta[0] == c.cls ? 0 : -1;
}

__global__ __launch_bounds__(V3D_BLOCK) void kitti_pass1_kernel(const int* __restrict__ gt_meta, const int* __restrict__ gt_off,
                                                                const float* __restrict__ dt, const int* __restrict__ dt_meta,
                                                                const int* __restrict__ dt_off, const int64_t* __restrict__ ov_off,
                                                                const float* __restrict__ ov, int64_t ov_plane,
                                                                KeCombos combos, int n_combos, int capacity,
                                                                int* __restrict__ tp_count, float* __restrict__ tp_scores,
                                                                int* __restrict__ n_valid) {
  const int lane = threadIdx.x & 63;
  const int combo = blockIdx.y * (V3D_BLOCK / V3D_WAVE) + (threadIdx.x >> 6);
  if (combo >= n_combos) return;  // (wave-uniform: no block barrier below)
  const v3d_kitti_combo c = combos.c[combo];
  const int f = blockIdx.x;
  const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
  const int d0 = dt_off[f], nd = dt_off[f + 1] - d0;
  if (ng <= 0 || ng > V3D_KITTI_MAX_GT || nd > V3D_KITTI_MAX_DT) return;
  const float* ovf = ov + c.metric * ov_plane + ov_off[f];  // this frame's matrix of the combo's metric
  // this lane's detections j = lane + 64 q: "in the scan" (ignored_dt != -1) and "assigned" as bits q
  const int nq = (nd + 63) >> 6;
  unsigned live = 0u, assigned = 0u;
  for (int q = 0; q < nq; q++) {
    const int j = lane + 64 * q;
    if (j < nd && ignored_dt(dt_meta + 2 * (size_t)(d0 + j), c) != -1) live |= 1u << q;
  }
  int valid = 0;
  for (int i = 0; i < ng; i++) {
    const int ig = ignored_gt(gt_meta + 2 * (size_t)(g0 + i), c);
    if (ig == -1) continue;
    valid += ig == 0;
    float best_s = -INFINITY;
    int best_j = 0x7fffffff;
    for (int q = 0; q < nq; q++) {
      if (!(((live & ~assigned) >> q) & 1u)) continue;
      const int j = lane + 64 * q;
      if (!(ovf[(size_t)j * ng + i] > c.min_overlap)) continue;
      const float s = dt[8 * (size_t)(d0 + j) + 7];
      if (best_j == 0x7fffffff || s > best_s) {  // q ascends: ties keep the earlier detection
        best_s = s;
        best_j = j;
      }
    }
    for (int m = 32; m >= 1; m >>= 1) {  // wave argmax: higher score, then lower index
      const float os = __shfl_xor(best_s, m, 64);
      const int oj = __shfl_xor(best_j, m, 64);
      if (oj != 0x7fffffff && (best_j == 0x7fffffff || os > best_s || (os == best_s && oj < best_j))) {
        best_s = os;
        best_j = oj;
      }
    }
    if (best_j == 0x7fffffff) continue;  // (a false negative when ig == 0: pass 2 counts those)
    if ((best_j & 63) == lane) assigned |= 1u << (best_j >> 6);
    if (ig == 0 && ignored_dt(dt_meta + 2 * (size_t)(d0 + best_j), c) == 0 && lane == 0) {
      const int pos = atomicAdd(tp_count + combo, 1);
      if (pos < capacity) tp_scores[(size_t)combo * capacity + pos] = best_s;
    }
  }
  if (lane == 0 && valid) atomicAdd(n_valid + combo, valid);
}

__global__ __launch_bounds__(V3D_WAVE) void kitti_thresholds_kernel(const float* __restrict__ sorted, int capacity,
                                                                    const int* __restrict__ tp_count, const int* __restrict__ n_valid,
                                                                    int n_combos, float* __restrict__ thresholds,
                                                                    int* __restrict__ n_thresholds) {
  const int combo = blockIdx.x * V3D_WAVE + threadIdx.x;
  if (combo >= n_combos) return;
  const int n = min(tp_count[combo], capacity), ngt = n_valid[combo];
  const float* s = sorted + (size_t)combo * capacity;
  int k = 0;
  if (ngt > 0) {
    double current = 0.0;
    for (int i = 0; i < n && k < KE_NT; i++) {
      const double l = (double)(i + 1) / ngt;
      const double r = i < n - 1 ? (double)(i + 2) / ngt : l;
      if ((r - current) < (current - l) && i < n - 1) continue;
      thresholds[(size_t)combo * KE_NT + k++] = s[i];
      current += 1.0 / (KE_NT - 1.0);
    }
  }
  n_thresholds[combo] = k;
}

// Image boxes are (x1, y1, x2, y2, alpha) f32 rows; overlaps are taken in double from the f32 corners, without +1.
__device__ __forceinline__ double img_inter(double x1, double y1, double x2, double y2, const float* g) {
  const double iw = fmin(x2, (double)g[2]) - fmax(x1, (double)g[0]);
  const double ih = fmin(y2, (double)g[3]) - fmax(y1, (double)g[1]);
  return (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
}

// The frame as the generic pass 2 reads it: straight from the ragged global arrays, flags derived per access.
struct KeGlobalFrame {
  const int* gt_meta;
  const int* dt_meta;
  const float* dt;  // score in column 7
  const float* ov;  // the frame's (n_dt, n_gt) matrix of the combo's metric
  int g0, d0, ng;   // the frame's first rows
  v3d_kitti_combo c;
  __device__ __forceinline__ int ig(int i) const { return ignored_gt(gt_meta + 2 * (size_t)(g0 + i), c); }
  __device__ __forceinline__ bool dontcare(int i) const { return (gt_meta[2 * (size_t)(g0 + i) + 1] >> KE_DONTCARE_BIT) & 1; }
  __device__ __forceinline__ int igd(int j) const { return ignored_dt(dt_meta + 2 * (size_t)(d0 + j), c); }
  __device__ __forceinline__ float score(int j) const { return dt[8 * (size_t)(d0 + j) + 7]; }
  __device__ __forceinline__ float overlap(int j, int i) const { return ov[(size_t)j * ng + i]; }
};

// The frame as the family pass 2 reads it: flags and scores staged in LDS once per (frame, family); `ov` is the LDS tile or,
// for a frame whose tile does not fit, the global matrix.
struct KeLdsFrame {
  const unsigned char* gtf;  // per ground truth: ignored_gt + 1 in bits 0-1, DontCare in bit 2
  const signed char* dtf;    // per detection: ignored_dt
  const float* sc;           // per detection: score
  const float* ov;
  int ng;
  __device__ __forceinline__ int ig(int i) const { return (gtf[i] & 3) - 1; }
  __device__ __forceinline__ bool dontcare(int i) const { return (gtf[i] >> 2) & 1; }
  __device__ __forceinline__ int igd(int j) const { return dtf[j]; }
  __device__ __forceinline__ float score(int j) const { return sc[j]; }
  __device__ __forceinline__ float overlap(int j, int i) const { return ov[(size_t)j * ng + i]; }
};

// Pass 2 of one lane (one threshold) on one frame, the rule written once for both pass-2 kernels: the greedy assignment with
// false positives, then (image) the DontCare step and the true-positive similarity sum in ground-truth order.  `assigned` is
// the lane's bitmask, word w at assigned[w * 64]; the frame's image rows start at g0 / d0 of gt_img / dt_img.
template <class F>
__device__ __forceinline__ void ke_pass2_lane(const F& fr, int ng, int nd, float thresh, float min_overlap, bool image,
                                              unsigned long long* assigned, const float* gt_img, const float* dt_img, int g0,
                                              int d0, int& tp, int& fp, int& fn, double& sim) {
  const int nw = (nd + 63) >> 6;
  for (int w = 0; w < nw; w++) assigned[w * 64] = 0ull;
  tp = fp = fn = 0;
  sim = 0.0;
  int dc_lo = ng, dc_hi = 0;  // (bbox) the DontCare regions lie in [dc_lo, dc_hi)
  for (int i = 0; i < ng; i++) {
    if (image && fr.dontcare(i)) {
      dc_lo = min(dc_lo, i);
      dc_hi = i + 1;
    }
    const int ig = fr.ig(i);
    if (ig == -1) continue;
    int best = -1;
    bool best_ign = false;
    float best_ov = 0.f;
    for (int j = 0; j < nd; j++) {
      const int igd = fr.igd(j);
      if (igd == -1) continue;
      if (fr.score(j) < thresh) continue;
      if ((assigned[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
      const float o = fr.overlap(j, i);
      if (!(o > min_overlap)) continue;
      if (igd == 0) {  // a counted detection: the largest overlap wins (earliest on ties), and displaces an ignored pick
        if (best < 0 || best_ign || o > best_ov) {
          best = j;
          best_ov = o;
          best_ign = false;
        }
      } else if (best < 0) {  // a short detection: only while nothing is picked
        best = j;
        best_ign = true;
      }
    }
    if (best < 0) {
      fn += ig == 0;
      continue;
    }
    assigned[(best >> 6) * 64] |= 1ull << (best & 63);
    if (ig == 0 && !best_ign) {
      tp++;
      if (image) {
        const double delta = (double)gt_img[5 * (size_t)(g0 + i) + 4] - (double)dt_img[5 * (size_t)(d0 + best) + 4];
        sim += (1.0 + cos(delta)) / 2.0;
      }
    }
  }
  // false positives; (bbox) an unassigned counted detection over a DontCare region (inter / area_dt > min overlap) is absorbed
  for (int j = 0; j < nd; j++) {
    if (fr.igd(j) != 0) continue;
    if (fr.score(j) < thresh) continue;
    if ((assigned[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
    bool absorbed = false;
    if (image && dc_lo < dc_hi) {
      const float* b = dt_img + 5 * (size_t)(d0 + j);
      const double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
      const double area = (x2 - x1) * (y2 - y1);  // (positive wherever the intersection is)
      for (int i = dc_lo; i < dc_hi && !absorbed; i++) {
        if (!fr.dontcare(i)) continue;
        const double inter = img_inter(x1, y1, x2, y2, gt_img + 5 * (size_t)(g0 + i));
        absorbed = inter > 0.0 && inter / area > (double)min_overlap;
      }
    }
    fp += !absorbed;
  }
}

// A lane's (tp, fp, fn) and (bbox) similarity into row `at` = combo * 41 + threshold
__device__ __forceinline__ void ke_pass2_add(int* counts, unsigned long long* similarity, size_t at, bool image, int tp, int fp,
                                             int fn, double sim) {
  int* out = counts + at * 3;
  if (tp) atomicAdd(out + 0, tp);
  if (fp) atomicAdd(out + 1, fp);
  if (fn) atomicAdd(out + 2, fn);
  // 32.32 fixed point: sim <= 256 per frame, so each add is < 2^40; integer adds make the total order-free and exact
  if (image && tp) atomicAdd(similarity + at, (unsigned long long)llrint(sim * 4294967296.0));
}

__global__ __launch_bounds__(V3D_BLOCK) void kitti_pass2_kernel(
    const int* __restrict__ gt_meta, const int* __restrict__ gt_off, const float* __restrict__ gt_img, const float* __restrict__ dt,
    const int* __restrict__ dt_meta, const int* __restrict__ dt_off, const float* __restrict__ dt_img,
    const int64_t* __restrict__ ov_off, const float* __restrict__ ov, int64_t ov_plane, KeCombos combos, int n_combos,
    const float* __restrict__ thresholds, const int* __restrict__ n_thresholds, int* __restrict__ counts,
    unsigned long long* __restrict__ similarity) {
  __shared__ unsigned long long assigned_lds[V3D_BLOCK / V3D_WAVE][KE_WORDS * 64];  // word w of lane L at [w * 64 + L]
  const int lane = threadIdx.x & 63;
  const int combo = blockIdx.y * (V3D_BLOCK / V3D_WAVE) + (threadIdx.x >> 6);
  if (combo >= n_combos) return;  // (wave-uniform: no block barrier below)
  const v3d_kitti_combo c = combos.c[combo];
  const bool image = c.metric == V3D_KITTI_METRIC_BBOX;  // (wave-uniform) the DontCare step and the similarity sum
  const int nt = n_thresholds[combo];
  if (lane >= nt) return;  // one lane per threshold; no cross-lane traffic below
  const int f = blockIdx.x;
  const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
  const int d0 = dt_off[f], nd = dt_off[f + 1] - d0;
  if (ng < 0 || nd < 0 || ng > V3D_KITTI_MAX_GT || nd > V3D_KITTI_MAX_DT) return;
  const float thresh = thresholds[combo * KE_NT + lane];
  const float* ovf = ov + c.metric * ov_plane + (ng ? ov_off[f] : 0);  // this frame's matrix of the combo's metric
  const KeGlobalFrame fr{gt_meta, dt_meta, dt, ovf, g0, d0, ng, c};
  int tp, fp, fn;
  double sim;
  ke_pass2_lane(fr, ng, nd, thresh, c.min_overlap, image, assigned_lds[threadIdx.x >> 6] + lane, gt_img, dt_img, g0, d0, tp, fp,
                fn, sim);
  ke_pass2_add(counts, similarity, (size_t)combo * KE_NT + lane, image, tp, fp, fn, sim);
}

// Dynamic LDS of the family kernel, in bytes from the start (8-byte aligned pieces first): `waves` bitmask slabs of words * 64
// u64, max_dt scores (f32), tile_cap overlaps (f32), max_dt ignored_dt (i8), max_gt ground-truth flags (u8).
struct KeFamLds {
  size_t scores, tile, dtf, gtf, bytes;
};
__host__ __device__ __forceinline__ KeFamLds ke_fam_lds(int waves, int words, int max_dt, int max_gt, int tile_cap) {
  KeFamLds l;
  l.scores = (size_t)waves * words * 64 * 8;
  l.tile = l.scores + 4 * (size_t)max_dt;
  l.dtf = l.tile + 4 * (size_t)tile_cap;
  l.gtf = l.dtf + (size_t)max_dt;
  l.bytes = (l.gtf + (size_t)max_gt + 15) & ~(size_t)15;
  return l;
}

// Pass 2 over level families: one workgroup per (frame, family), wave w = the family's level w, lane = threshold.  The frame's
// scores, ignored_dt, ignored_gt / DontCare flags and (when n_dt * n_gt <= tile_cap) its overlap tile go to LDS once; every
// level then runs ke_pass2_lane on them.
__global__ __launch_bounds__(KE_FAM_LEVELS * V3D_WAVE) void kitti_pass2_family_kernel(
    const int* __restrict__ gt_meta, const int* __restrict__ gt_off, const float* __restrict__ gt_img, const float* __restrict__ dt,
    const int* __restrict__ dt_meta, const int* __restrict__ dt_off, const float* __restrict__ dt_img,
    const int64_t* __restrict__ ov_off, const float* __restrict__ ov, int64_t ov_plane, KeFamilies fams, int max_dt, int max_gt,
    int words, int tile_cap, const float* __restrict__ thresholds, const int* __restrict__ n_thresholds, int* __restrict__ counts,
    unsigned long long* __restrict__ similarity) {
  extern __shared__ unsigned long long ke_fam_smem[];
  const int f = blockIdx.x;
  const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
  const int d0 = dt_off[f], nd = dt_off[f + 1] - d0;
  if (ng < 0 || nd < 0 || ng > max_gt || nd > max_dt) return;  // (block-uniform; the LDS carve holds max_dt / max_gt)
  const KeFamily& fam = fams.f[blockIdx.y];
  const v3d_kitti_combo c = fam.c;
  const KeFamLds l = ke_fam_lds(blockDim.x >> 6, words, max_dt, max_gt, tile_cap);
  unsigned char* base = (unsigned char*)ke_fam_smem;
  float* sc = (float*)(base + l.scores);
  float* tile = (float*)(base + l.tile);
  signed char* dtf = (signed char*)(base + l.dtf);
  unsigned char* gtf = base + l.gtf;
  for (int j = threadIdx.x; j < nd; j += blockDim.x) {
    sc[j] = dt[8 * (size_t)(d0 + j) + 7];
    dtf[j] = (signed char)ignored_dt(dt_meta + 2 * (size_t)(d0 + j), c);
  }
  for (int i = threadIdx.x; i < ng; i += blockDim.x) {
    const int* gm = gt_meta + 2 * (size_t)(g0 + i);
    gtf[i] = (unsigned char)((ignored_gt(gm, c) + 1) | (((gm[1] >> KE_DONTCARE_BIT) & 1) << 2));
  }
  const float* ovf = ov + c.metric * ov_plane + (ng ? ov_off[f] : 0);
  const int pairs = nd * ng;
  const bool staged = pairs <= tile_cap;  // (block-uniform)
  if (staged)
    for (int k = threadIdx.x; k < pairs; k += blockDim.x) tile[k] = ovf[k];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave >= fam.n) return;
  const int combo = fam.combo[wave];
  const bool image = c.metric == V3D_KITTI_METRIC_BBOX;
  if (lane >= n_thresholds[combo]) return;
  const float thresh = thresholds[combo * KE_NT + lane];
  const KeLdsFrame fr{gtf, dtf, sc, staged ? tile : ovf, ng};
  int tp, fp, fn;
  double sim;
  ke_pass2_lane(fr, ng, nd, thresh, fam.level[wave], image, ke_fam_smem + (size_t)wave * words * 64 + lane, gt_img, dt_img, g0,
                d0, tp, fp, fn, sim);
  ke_pass2_add(counts, similarity, (size_t)combo * KE_NT + lane, image, tp, fp, fn, sim);
}

// v (KE_NT ratios) -> its running maximum from the right, then out = (R11, R40) in percent, summed in definition order
__device__ __forceinline__ void ke_r11_r40(double* v, double* out) {
#pragma unroll
  for (int k = KE_NT - 2; k >= 0; k--) v[k] = fmax(v[k], v[k + 1]);
  double r11 = 0.0, r40 = 0.0;
#pragma unroll
  for (int k = 0; k < KE_NT; k += 4) r11 += v[k];
#pragma unroll
  for (int k = 1; k < KE_NT; k++) r40 += v[k];
  out[0] = r11 / 11.0 * 100.0;
  out[1] = r40 / 40.0 * 100.0;
}

__global__ __launch_bounds__(V3D_WAVE) void kitti_ap_kernel(const int* __restrict__ counts,
                                                            const unsigned long long* __restrict__ similarity,
                                                            const int* __restrict__ n_thresholds, int n_combos,
                                                            double* __restrict__ ap, double* __restrict__ aos) {
  const int combo = blockIdx.x * V3D_WAVE + threadIdx.x;
  if (combo >= n_combos) return;
  const int nt = n_thresholds[combo];
  double v[KE_NT];
#pragma unroll
  for (int k = 0; k < KE_NT; k++) {
    const int* cnt = counts + ((size_t)combo * KE_NT + k) * 3;
    const int tp = cnt[0], fp = cnt[1];
    v[k] = (k < nt && tp + fp > 0) ? (double)tp / (double)(tp + fp) : 0.0;
  }
  ke_r11_r40(v, ap + 2 * combo);
  if (!similarity) return;
#pragma unroll
  for (int k = 0; k < KE_NT; k++) {
    const int* cnt = counts + ((size_t)combo * KE_NT + k) * 3;
    const int den = cnt[0] + cnt[1];
    const double s = (double)(long long)similarity[(size_t)combo * KE_NT + k] * (1.0 / 4294967296.0);
    v[k] = (k < nt && den > 0) ? s / (double)den : 0.0;
  }
  ke_r11_r40(v, aos + 2 * combo);
}

// ---- 2-D bbox overlaps ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(V3D_BLOCK) void kitti_overlaps_image_kernel(const float* __restrict__ gt_img,
                                                                         const int* __restrict__ gt_off,
                                                                         const float* __restrict__ dt_img,
                                                                         const int* __restrict__ dt_off,
                                                                         const int64_t* __restrict__ ov_off,
                                                                         float* __restrict__ ov_2d) {
  __shared__ float gts[V3D_KITTI_MAX_GT][4];
  const int f = blockIdx.x;
  const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
  const int d0 = dt_off[f], nd = dt_off[f + 1] - d0;
  if (ng <= 0 || nd <= 0 || ng > V3D_KITTI_MAX_GT || nd > V3D_KITTI_MAX_DT) return;  // (block-uniform)
  if ((int)threadIdx.x < ng) {
    const float* g = gt_img + 5 * (size_t)(g0 + threadIdx.x);
    for (int k = 0; k < 4; k++) gts[threadIdx.x][k] = g[k];
  }
  __syncthreads();
  const int j = blockIdx.y * V3D_BLOCK + threadIdx.x;
  if (j >= nd) return;
  const float* b = dt_img + 5 * (size_t)(d0 + j);
  const double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
  const double area = (x2 - x1) * (y2 - y1);
  const size_t row = (size_t)ov_off[f] + (size_t)j * ng;
  for (int i = 0; i < ng; i++) {
    const float* g = gts[i];
    const double inter = img_inter(x1, y1, x2, y2, g);
    // inter > 0 needs both boxes proper in x and y: the union is positive
    ov_2d[row + i] = inter > 0.0 ? (float)(inter / (area + ((double)g[2] - g[0]) * ((double)g[3] - g[1]) - inter)) : 0.f;
  }
}

static int ke_check(int n_frames, int max_dt, int max_gt, int n_combos) {
  if (n_frames < 0 || max_dt < 0 || max_gt < 0 || n_combos < 0) return V3D_EINVAL;
  if (max_dt > V3D_KITTI_MAX_DT || max_gt > V3D_KITTI_MAX_GT || n_combos > V3D_KITTI_MAX_COMBOS) return V3D_EUNSUPPORTED;
  return V3D_OK;
}

static KeCombos ke_combos(const v3d_kitti_combo* host, int n) {
  KeCombos k = {};
  for (int i = 0; i < n && i < KE_CHUNK; i++) k.c[i] = host[i];
  return k;
}

static bool ke_same_family(const v3d_kitti_combo& a, const v3d_kitti_combo& b) {
  return a.cls == b.cls && a.neighbour == b.neighbour && a.difficulty == b.difficulty && a.metric == b.metric;
}

// The metrics the combos use as bits 1 << metric, or -1 for a metric outside 0..2 (it indexes the overlap planes)
static int ke_metrics(const v3d_kitti_combo* host, int n) {
  int bits = 0;
  for (int i = 0; i < n; i++) {
    if (host[i].metric < V3D_KITTI_METRIC_BEV || host[i].metric > V3D_KITTI_METRIC_BBOX) return -1;
    bits |= 1 << host[i].metric;
  }
  return bits;
}

extern "C" int v3d_kitti_eval_overlaps(const float* gt, const int32_t* gt_off, const float* dt, const int32_t* dt_off,
                                       const int64_t* ov_off, int n_frames, int max_dt, int max_gt, float* ov_bev, float* ov_3d,
                                       v3d_stream_t stream) {
  const int e = ke_check(n_frames, max_dt, max_gt, 0);
  if (e) return e;
  if (n_frames == 0 || max_dt == 0 || max_gt == 0) return V3D_OK;
  if (!gt || !gt_off || !dt || !dt_off || !ov_off || !ov_bev || !ov_3d) return V3D_EINVAL;
  hipLaunchKernelGGL(kitti_overlaps_kernel, dim3(n_frames, v3d_ceil_div(max_dt, V3D_BLOCK)), dim3(V3D_BLOCK), 0,
                     (hipStream_t)stream, gt, gt_off, dt, dt_off, ov_off, ov_bev, ov_3d);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_kitti_eval_pass1(const int32_t* gt_meta, const int32_t* gt_off, const float* dt, const int32_t* dt_meta,
                                    const int32_t* dt_off, const int64_t* ov_off, const float* ov, int64_t ov_plane, int n_frames,
                                    int max_dt, int max_gt, const v3d_kitti_combo* combos_host, int n_combos, int capacity,
                                    int32_t* tp_count, float* tp_scores, int32_t* n_valid, v3d_stream_t stream) {
  const int e = ke_check(n_frames, max_dt, max_gt, n_combos);
  if (e) return e;
  if (capacity < 0 || ov_plane < 0) return V3D_EINVAL;
  if (n_frames == 0 || n_combos == 0 || max_gt == 0) return V3D_OK;
  if (!gt_meta || !gt_off || !dt_off || !ov_off || !combos_host || !tp_count || !n_valid) return V3D_EINVAL;
  if (max_dt > 0 && (!dt || !dt_meta || !ov || !tp_scores)) return V3D_EINVAL;
  if (ke_metrics(combos_host, n_combos) < 0) return V3D_EINVAL;
  for (int b = 0; b < n_combos; b += KE_CHUNK) {  // one launch per by-value table of KE_CHUNK combos
    const int n = min(KE_CHUNK, n_combos - b);
    hipLaunchKernelGGL(kitti_pass1_kernel, dim3(n_frames, v3d_ceil_div(n, V3D_BLOCK / V3D_WAVE)), dim3(V3D_BLOCK), 0,
                       (hipStream_t)stream, gt_meta, gt_off, dt, dt_meta, dt_off, ov_off, ov, ov_plane, ke_combos(combos_host + b, n),
                       n, capacity, tp_count + b, tp_scores ? tp_scores + (size_t)b * capacity : nullptr, n_valid + b);
    V3D_CHECK_LAUNCH();
  }
  return V3D_OK;
}

extern "C" int v3d_kitti_eval_thresholds(const float* sorted_scores, int capacity, const int32_t* tp_count, const int32_t* n_valid,
                                         int n_combos, float* thresholds, int32_t* n_thresholds, v3d_stream_t stream) {
  const int e = ke_check(0, 0, 0, n_combos);
  if (e) return e;
  if (capacity < 0) return V3D_EINVAL;
  if (n_combos == 0) return V3D_OK;
  if (!tp_count || !n_valid || !thresholds || !n_thresholds || (capacity > 0 && !sorted_scores)) return V3D_EINVAL;
  hipLaunchKernelGGL(kitti_thresholds_kernel, dim3(v3d_ceil_div(n_combos, V3D_WAVE)), dim3(V3D_WAVE), 0, (hipStream_t)stream, sorted_scores, capacity, tp_count,
                     n_valid, n_combos, thresholds, n_thresholds);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_kitti_eval_pass2(const int32_t* gt_meta, const int32_t* gt_off, const float* gt_img, const float* dt,
                                    const int32_t* dt_meta, const int32_t* dt_off, const float* dt_img, const int64_t* ov_off,
                                    const float* ov, int64_t ov_plane, int n_frames, int max_dt, int max_gt,
                                    const v3d_kitti_combo* combos_host, int n_combos, const float* thresholds,
                                    const int32_t* n_thresholds, int32_t* counts, int64_t* similarity, v3d_stream_t stream) {
  const int e = ke_check(n_frames, max_dt, max_gt, n_combos);
  if (e) return e;
  if (ov_plane < 0) return V3D_EINVAL;
  if (n_frames == 0 || n_combos == 0) return V3D_OK;
  if (!gt_off || !dt_off || !ov_off || !combos_host || !thresholds || !n_thresholds || !counts) return V3D_EINVAL;
  if (max_gt > 0 && !gt_meta) return V3D_EINVAL;
  if (max_dt > 0 && (!dt || !dt_meta)) return V3D_EINVAL;
  if (max_dt > 0 && max_gt > 0 && !ov) return V3D_EINVAL;
  const int metrics = ke_metrics(combos_host, n_combos);
  if (metrics < 0) return V3D_EINVAL;
  const bool bbox = (metrics >> V3D_KITTI_METRIC_BBOX) & 1;  // the DontCare step and the similarity read these
  if (bbox && (!similarity || (max_gt > 0 && !gt_img) || (max_dt > 0 && !dt_img))) return V3D_EINVAL;
  unsigned long long* sim = (unsigned long long*)similarity;
  // Level families (combos equal but for min_overlap, up to KE_FAM_LEVELS each, in combo order) of KE_FAMILY_MIN or more
  // combos go to the family kernel when its LDS carve fits the budget; every other combo to the generic kernel, in runs of
  // consecutive combos, KE_CHUNK per launch.
  const int words = max(1, v3d_ceil_div(max_dt, 64));
  const KeFamLds fixed = ke_fam_lds(KE_FAM_LEVELS, words, max_dt, max_gt, 0);
  const bool family_fits = fixed.bytes <= KE_FAM_LDS;
  std::vector<KeFamily> fams;
  for (int i = 0; i < n_combos; i++) {
    int k = (int)fams.size() - 1;
    while (k >= 0 && !(ke_same_family(fams[k].c, combos_host[i]) && fams[k].n < KE_FAM_LEVELS)) k--;
    if (k < 0) {
      fams.push_back(KeFamily{});
      k = (int)fams.size() - 1;
      fams[k].c = combos_host[i];
    }
    fams[k].combo[fams[k].n] = i;
    fams[k].level[fams[k].n++] = combos_host[i].min_overlap;
  }
  std::vector<KeFamily> big;
  std::vector<char> generic(n_combos, 1);
  for (const KeFamily& fm : fams) {
    if (!family_fits || fm.n < KE_FAMILY_MIN) continue;
    big.push_back(fm);
    for (int w = 0; w < fm.n; w++) generic[fm.combo[w]] = 0;
  }
  for (int b = 0; b < n_combos;) {
    if (!generic[b]) {
      b++;
      continue;
    }
    int n = 1;
    while (n < KE_CHUNK && b + n < n_combos && generic[b + n]) n++;
    hipLaunchKernelGGL(kitti_pass2_kernel, dim3(n_frames, v3d_ceil_div(n, V3D_BLOCK / V3D_WAVE)), dim3(V3D_BLOCK), 0,
                       (hipStream_t)stream, gt_meta, gt_off, gt_img, dt, dt_meta, dt_off, dt_img, ov_off, ov, ov_plane,
                       ke_combos(combos_host + b, n), n, thresholds + (size_t)b * KE_NT, n_thresholds + b,
                       counts + (size_t)b * KE_NT * 3, sim ? sim + (size_t)b * KE_NT : nullptr);
    V3D_CHECK_LAUNCH();
    b += n;
  }
  for (size_t b = 0; b < big.size(); b += KE_FAM_CHUNK) {
    KeFamilies table = {};
    const int n = (int)std::min<size_t>(KE_FAM_CHUNK, big.size() - b);
    int waves = 0;
    for (int k = 0; k < n; k++) {
      table.f[k] = big[b + k];
      waves = max(waves, table.f[k].n);
    }
    const KeFamLds lds = ke_fam_lds(waves, words, max_dt, max_gt, 0);
    const int tile_cap = (int)((KE_FAM_LDS - lds.bytes) / 4) & ~3;  // (keeps the carve's total within the budget)
    const KeFamLds all = ke_fam_lds(waves, words, max_dt, max_gt, tile_cap);
    hipLaunchKernelGGL(kitti_pass2_family_kernel, dim3(n_frames, n), dim3(waves * V3D_WAVE), all.bytes, (hipStream_t)stream, gt_meta,
                       gt_off, gt_img, dt, dt_meta, dt_off, dt_img, ov_off, ov, ov_plane, table, max_dt, max_gt, words, tile_cap,
                       thresholds, n_thresholds, counts, sim);
    V3D_CHECK_LAUNCH();
  }
  return V3D_OK;
}

extern "C" int v3d_kitti_eval_ap(const int32_t* counts, const int64_t* similarity, const int32_t* n_thresholds, int n_combos,
                                 double* ap, double* aos, v3d_stream_t stream) {
  const int e = ke_check(0, 0, 0, n_combos);
  if (e) return e;
  if (n_combos == 0) return V3D_OK;
  if (!counts || !n_thresholds || !ap || (similarity && !aos)) return V3D_EINVAL;
  hipLaunchKernelGGL(kitti_ap_kernel, dim3(v3d_ceil_div(n_combos, V3D_WAVE)), dim3(V3D_WAVE), 0, (hipStream_t)stream, counts,
                     (const unsigned long long*)similarity, n_thresholds, n_combos, ap, aos);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_kitti_eval_overlaps_image(const float* gt_img, const int32_t* gt_off, const float* dt_img, const int32_t* dt_off,
                                             const int64_t* ov_off, int n_frames, int max_dt, int max_gt, float* ov_2d,
                                             v3d_stream_t stream) {
  const int e = ke_check(n_frames, max_dt, max_gt, 0);
  if (e) return e;
  if (n_frames == 0 || max_dt == 0 || max_gt == 0) return V3D_OK;
  if (!gt_img || !gt_off || !dt_img || !dt_off || !ov_off || !ov_2d) return V3D_EINVAL;
  hipLaunchKernelGGL(kitti_overlaps_image_kernel, dim3(n_frames, v3d_ceil_div(max_dt, V3D_BLOCK)), dim3(V3D_BLOCK), 0,
                     (hipStream_t)stream, gt_img, gt_off, dt_img, dt_off, ov_off, ov_2d);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
