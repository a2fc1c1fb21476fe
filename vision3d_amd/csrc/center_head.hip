// center_head.hip -- the anchor-free centre heatmap head (CenterPoint; stage 1 of PV-RCNN++): target assignment, loss with its
// gradient, and peak decode around the fused 1x1 head maps (B, n_cls + 8, H, W) fp32 -- channels [0, n_cls) heat logits, n_cls + j,
// j = 0..7: dx, dy, z, log w, log l, log h, sin yaw, cos yaw, raw.  Opt-in (cfg.CENTERHEAD); no upstream counterpart.
//
// The definition is the repository's own (restated in float64 by tests/center_head_ref.py):
//   geometry   (px, py) metres per cell, (x_lo, y_lo) the grid origin; the map is (H, W) = (ny, nx).
//   object     fx = (x - x_lo) / px, fy = (y - y_lo) / py in fp32 (one IEEE operation each), (ix, iy) = floor.  Live: inside the map,
//              0 <= class < n_cls, w, l, h finite and > 0.  Radius: the three CornerNet roots in DOUBLE from the fp32 box,
//              a = w / px, b = l / py, o = min_overlap, s = a + b:
//                  r1 = (s + sqrt(s^2 - 4 a b (1 - o) / (1 + o))) / 2,   r2 = (2 s + sqrt(4 s^2 - 16 (1 - o) a b)) / 2,
//                  r3 = (-2 o s + sqrt(4 o^2 s^2 + 16 o (1 - o) a b)) / 2,   r = max(min_radius, int(min(r1, r2, r3))),
//              sigma = (2 r + 1) / 6;  k = -1 / (2 sigma^2), rounded to fp32 once.
//   heat       heat[b, c, v, u] = max over the frame's live objects of class c with |u - ix| <= r, |v - iy| <= r of
//              expf(float(du^2 + dv^2) * k): exactly 1 at a centre (expf(0)), exactly 0 where no window reaches.
//   per object ind = iy * W + ix, mask, cls, reg = (fx - ix, fy - iy, z, logf w, logf l, logf h, sinf yaw, cosf yaw), padded to
//              CH_MAX_OBJ rows per frame; not live: ind = -1, mask = 0, cls = the given class, reg = 0.
//   loss       N = max(#mask, 1) over the batch, p = sigmoid(x); heat == 1: -(1 - p)^alpha log p, else -(1 - heat)^beta p^alpha
//              log(1 - p), with log p = -softplus(-x), log(1 - p) = -softplus(x) and p, 1 - p of loss_device.h v3d_sigmoid_pq;
//              hm = sum / N.  reg = sum over masked objects and
//              j of code_weights[j] |pred_j - target_j| / N, pred read at the object's cell; sign(0) = 0.
//   decode     peak: logit >= each in-map neighbour (of 8).  Per (b, c) the topk peaks by logit, ties to the lower cell; box =
//              ((ix + dx) px + x_lo, (iy + dy) py + y_lo, z, expf(w, l, h), atan2f(sin, cos)), score = sigmoid; missing: zeros.
//
// ch_targets_kernel (ONE launch): grid (tiles of 256 cells, class, frame).  Every workgroup prepares the frame's <= 128 object records
// itself (three double square roots per object: cheaper than a launch) in LDS; a lane owns one cell of one class and takes the
// maximum over the frame's records of its class whose window covers it -- no atomic, no clear: every heat cell is written once.
// The tile-0, class-0 workgroup of a frame writes the frame's per-object rows.
// ch_loss_heat_kernel: grid-stride over all channels of the maps: heat channels get their gradient, box channels exact zeros;
// per-lane double sums, the workgroup sum of loss_device.h, partials to the workspace.  ch_loss_box_kernel: a workgroup per frame,
// lane = object: the lowest-index masked object of a cell sums the gradients of the cell's objects in object order and stores them
// (plain stores behind the zeros, in stream order).  ch_loss_finalize_kernel: partials summed in index order in double.
// ch_peaks_kernel: grid (slices of 4096 cells, group = frame * n_cls + class): 64-bit keys (order-preserving logit bits << 32 |
// ~cell; 0 = not a peak) sorted in LDS (bitonic), the slice's best topk to the workspace.  ch_select_kernel: a workgroup per group
// merges the slices' sorted lists one at a time (best | next list reversed: one bitonic merge of 2048 keys, 11 steps), then decodes.
// The cell of a key is the index the kernel itself wrote into it: no index is derived from a map value; a NaN logit is never a peak.
#include "loss_device.h"
#include "v3d_internal.h"

#define CH_MAX_OBJ 128
#define CH_MAX_FRAMES 64
#define CH_MAX_CLS 8
#define CH_MAX_TOPK 1024
#define CH_MAX_CELLS (1 << 24)
#define CH_SLICE 4096
#define CH_LOSS_BLOCKS 512
#define CH_SEL_THREADS 1024
#define CH_FIN_THREADS 64  // ch_loss_finalize_kernel: one wave

struct ChFrames {  // host offsets, passed by value: first object of each frame
  int bx[CH_MAX_FRAMES + 1];
};

struct ChGeom {
  double px, py;
  float pxf, pyf, x_lo, y_lo;
  int H, W, n_cls;
};

struct ChRec {  // one live object, as the heat lanes read it
  int ix, iy, r, cls;
  float k;
};

__global__ __launch_bounds__(V3D_BLOCK) void ch_targets_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ classes,
                                                               const ChFrames fr, const ChGeom g, double min_overlap, int min_radius,
                                                               float* __restrict__ heat, int32_t* __restrict__ ind,
                                                               uint8_t* __restrict__ mask, int32_t* __restrict__ cls_out,
                                                               float* __restrict__ reg) {
  __shared__ ChRec rec[CH_MAX_OBJ];
  const int tid = threadIdx.x, b = blockIdx.z, c = blockIdx.y;
  const int b0 = fr.bx[b], n = fr.bx[b + 1] - b0;
  const bool writer = blockIdx.x == 0 && c == 0;
  if (tid < CH_MAX_OBJ) {
    bool live = false;
    int ix = 0, iy = 0, k_cls = 0;
    float row[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    ChRec r;
    r.ix = r.iy = r.r = 0, r.cls = -1, r.k = 0.f;
    if (tid < n) {
      const float* bx = boxes + 7 * (size_t)(b0 + tid);
      const float x = bx[0], y = bx[1], w = bx[3], l = bx[4], h = bx[5];
      k_cls = classes[b0 + tid];
      const float fx = (x - g.x_lo) / g.pxf, fy = (y - g.y_lo) / g.pyf;
      const bool inside = fx >= 0.f && fx < (float)g.W && fy >= 0.f && fy < (float)g.H;  // (NaN: false)
      const bool sized = w > 0.f && l > 0.f && h > 0.f && w < INFINITY && l < INFINITY && h < INFINITY;
      live = inside && sized && k_cls >= 0 && k_cls < g.n_cls;
      if (live) {
        ix = (int)floorf(fx), iy = (int)floorf(fy);
        const double a = (double)w / g.px, bb = (double)l / g.py, o = min_overlap, s = a + bb;
        const double r1 = (s + sqrt(s * s - 4.0 * a * bb * (1.0 - o) / (1.0 + o))) / 2.0;
        const double r2 = (2.0 * s + sqrt(4.0 * s * s - 16.0 * (1.0 - o) * a * bb)) / 2.0;
        const double r3 = (-2.0 * o * s + sqrt(4.0 * o * o * s * s + 16.0 * o * (1.0 - o) * a * bb)) / 2.0;
        const double rm = fmin(fmin(r1, r2), r3);
        // (a, b are finite: rm is finite or NaN.  Radii beyond 2^20 cells -- boxes of hundreds of kilometres -- are clamped: safe,
        // and outside the definition)
        int rad = rm < 1048576.0 ? (int)rm : 1048576;
        if (!(rm >= 0.0)) rad = 0;
        if (rad < min_radius) rad = min_radius;
        const double sigma = (2.0 * rad + 1.0) / 6.0;
        r.ix = ix, r.iy = iy, r.r = rad, r.cls = k_cls, r.k = (float)(-1.0 / (2.0 * sigma * sigma));
        row[0] = fx - (float)ix, row[1] = fy - (float)iy, row[2] = bx[2];
        row[3] = logf(w), row[4] = logf(l), row[5] = logf(h), row[6] = sinf(bx[6]), row[7] = cosf(bx[6]);
      }
    }
    rec[tid] = r;  // (cls = -1: not live, drawn by no class)
    if (writer) {
      const size_t o = (size_t)b * CH_MAX_OBJ + tid;
      ind[o] = live ? iy * g.W + ix : -1;
      mask[o] = live ? 1 : 0;
      cls_out[o] = tid < n ? k_cls : 0;
#pragma unroll
      for (int j = 0; j < 8; j++) reg[8 * o + j] = row[j];
    }
  }
  __syncthreads();
  const int HW = g.H * g.W;
  const int cell = blockIdx.x * V3D_BLOCK + tid;
  if (cell >= HW) return;
  const int v = cell / g.W, u = cell - v * g.W;
  float best = 0.f;
  for (int i = 0; i < n; i++) {
    const ChRec r = rec[i];
    const int du = u - r.ix, dv = v - r.iy;
    if (r.cls == c && abs(du) <= r.r && abs(dv) <= r.r)
      best = fmaxf(best, expf((float)((long long)du * du + (long long)dv * dv) * r.k));
  }
  heat[((size_t)b * g.n_cls + c) * HW + cell] = best;
}

// ---- loss

template <int THREADS>  // of the workgroup
__device__ __forceinline__ int ch_count_masked(const uint8_t* __restrict__ mask, int rows, int* red) {
  // the number of masked objects of the batch, by every workgroup for itself (<= 8 192 bytes)
  int c = 0;
  for (int i = threadIdx.x; i < rows; i += THREADS) c += mask[i] != 0;
  return v3d_block_sum<THREADS / V3D_WAVE>(c, red);
}

__global__ __launch_bounds__(V3D_BLOCK) void ch_loss_heat_kernel(const float* __restrict__ maps, const float* __restrict__ heat,
                                                                 const uint8_t* __restrict__ mask, int B, int n_cls, int HW, float alpha,
                                                                 float beta, float* __restrict__ dmaps, double* __restrict__ partial) {
  __shared__ int red_i[V3D_BLOCK / V3D_WAVE];
  __shared__ double red[V3D_BLOCK / V3D_WAVE];
  const int cnt = ch_count_masked<V3D_BLOCK>(mask, B * CH_MAX_OBJ, red_i);
  const float inv_n = 1.f / (float)(cnt > 0 ? cnt : 1);
  const int O = n_cls + 8;
  const long long total = (long long)B * O * HW;
  double sum = 0.0;
  for (long long i = (long long)blockIdx.x * V3D_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * V3D_BLOCK) {
    const int pix = (int)(i % HW);
    const int o = (int)((i / HW) % O), b = (int)(i / ((long long)HW * O));
    float gx = 0.f;
    if (o < n_cls) {
      const float x = maps[i];
      const float t = heat[((size_t)b * n_cls + o) * HW + pix];
      float e, p, q;
      v3d_sigmoid_pq(x, e, p, q);
      if (t == 1.f) {
        const float lp = -v3d_softplus(-x, e);  // log p
        const float qa = alpha == 2.f ? q * q : powf(q, alpha);
        sum += (double)(-qa * lp);
        gx = qa * (alpha * p * lp - q);
      } else {
        const float lq = -v3d_softplus(x, e);  // log(1 - p)
        const float nt = 1.f - t;
        const float w = beta == 4.f ? (nt * nt) * (nt * nt) : powf(nt, beta);
        const float pa = alpha == 2.f ? p * p : powf(p, alpha);
        sum += (double)(-w * pa * lq);
        gx = w * pa * (p - alpha * q * lq);
      }
      gx *= inv_n;
    }
    dmaps[i] = gx;  // (box channels: exact zeros; ch_loss_box_kernel stores the object cells behind this launch)
  }
  const double t = v3d_block_sum<V3D_BLOCK / V3D_WAVE>(sum, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

struct ChWeights {
  float w[8];
};

__global__ __launch_bounds__(CH_MAX_OBJ) void ch_loss_box_kernel(const float* __restrict__ maps, const int32_t* __restrict__ ind,
                                                                 const uint8_t* __restrict__ mask, const float* __restrict__ reg, int B,
                                                                 int n_cls, int HW, const ChWeights cw, float* __restrict__ dmaps,
                                                                 double* __restrict__ partial) {
  __shared__ int red_i[CH_MAX_OBJ / 64];
  __shared__ int s_ind[CH_MAX_OBJ];
  __shared__ float s_g[CH_MAX_OBJ][8];
  __shared__ double s_l[CH_MAX_OBJ];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int cnt = ch_count_masked<CH_MAX_OBJ>(mask, B * CH_MAX_OBJ, red_i);
  const float inv_n = 1.f / (float)(cnt > 0 ? cnt : 1);
  const size_t o = (size_t)b * CH_MAX_OBJ + tid;
  int cell = ind[o];
  if (!mask[o] || cell < 0 || cell >= HW) cell = -1;
  const size_t base = ((size_t)b * (n_cls + 8) + n_cls) * HW;
  double loss = 0.0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float gj = 0.f;
    if (cell >= 0) {
      const float d = maps[base + (size_t)j * HW + cell] - reg[8 * o + j];
      loss += (double)(cw.w[j] * fabsf(d));
      gj = cw.w[j] * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f) * inv_n;
    }
    s_g[tid][j] = gj;
  }
  s_ind[tid] = cell;
  s_l[tid] = loss;
  __syncthreads();
  if (cell >= 0) {
    bool first = true;
    for (int i = 0; i < tid; i++) first = first && s_ind[i] != cell;
    if (first) {  // the lowest-index object of its cell: the cell's objects in object order
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; j++) acc[j] = s_g[tid][j];
      for (int i = tid + 1; i < CH_MAX_OBJ; i++) {
        if (s_ind[i] == cell) {
#pragma unroll
          for (int j = 0; j < 8; j++) acc[j] += s_g[i][j];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; j++) dmaps[base + (size_t)j * HW + cell] = acc[j];
    }
  }
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < CH_MAX_OBJ; i++) t += s_l[i];
    partial[b] = t;
  }
}

__global__ __launch_bounds__(CH_FIN_THREADS) void ch_loss_finalize_kernel(const double* __restrict__ heat_partial, int heat_blocks,
                                                                          const double* __restrict__ box_partial, int B,
                                                                          const uint8_t* __restrict__ mask, float* __restrict__ losses) {
  __shared__ int red_i[CH_FIN_THREADS / V3D_WAVE];
  const int cnt = ch_count_masked<CH_FIN_THREADS>(mask, B * CH_MAX_OBJ, red_i);
  const double n = (double)(cnt > 0 ? cnt : 1);
  if (threadIdx.x < 2) {
    const double* p = threadIdx.x == 0 ? heat_partial : box_partial;
    const int m = threadIdx.x == 0 ? heat_blocks : B;
    double t = 0.0;
    for (int i = 0; i < m; i++) t += p[i];
    losses[threadIdx.x] = (float)(t / n);
    if (threadIdx.x == 0) losses[2] = (float)n;
  }
}

// ---- decode

// keys[0..n) (n a power of two) descending, in LDS; every thread of the workgroup calls it
__device__ __forceinline__ void ch_bitonic_desc(unsigned long long* keys, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long a = keys[i], c = keys[p];
          const bool desc = (i & k) == 0;
          if (desc ? a < c : a > c) keys[i] = c, keys[p] = a;
        }
      }
    }
  }
  __syncthreads();
}

// keys[0..n) a bitonic sequence (descending then ascending) -> descending
__device__ __forceinline__ void ch_bitonic_merge_desc(unsigned long long* keys, int n) {
  for (int j = n >> 1; j > 0; j >>= 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int p = i ^ j;
      if (p > i) {
        const unsigned long long a = keys[i], c = keys[p];
        if (a < c) keys[i] = c, keys[p] = a;
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(V3D_BLOCK) void ch_peaks_kernel(const float* __restrict__ maps, int n_cls, int H, int W, int topk,
                                                             unsigned long long* __restrict__ lists) {
  __shared__ unsigned long long keys[CH_SLICE];
  const int group = blockIdx.y, b = group / n_cls, c = group - b * n_cls;
  const int HW = H * W;
  const float* m = maps + ((size_t)b * (n_cls + 8) + c) * HW;
  const int c0 = blockIdx.x * CH_SLICE;
  for (int t = threadIdx.x; t < CH_SLICE; t += V3D_BLOCK) {
    const int cell = c0 + t;
    unsigned long long key = 0ull;
    if (cell < HW) {
      const int v = cell / W, u = cell - v * W;
      const float x = m[cell];
      bool peak = x == x;
      for (int dv = -1; dv <= 1; dv++) {
        for (int du = -1; du <= 1; du++) {
          const int vv = v + dv, uu = u + du;
          if ((dv | du) != 0 && vv >= 0 && vv < H && uu >= 0 && uu < W) peak = peak && x >= m[vv * W + uu];
        }
      }
      if (peak) {
        unsigned int bits = __float_as_uint(x + 0.f);  // (-0 -> +0: equal logits, equal keys)
        bits = (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
        key = ((unsigned long long)bits << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)cell);
      }
    }
    keys[t] = key;
  }
  ch_bitonic_desc(keys, CH_SLICE);
  unsigned long long* out = lists + ((size_t)group * gridDim.x + blockIdx.x) * CH_MAX_TOPK;
  for (int t = threadIdx.x; t < CH_MAX_TOPK; t += V3D_BLOCK) out[t] = t < topk ? keys[t] : 0ull;
}

__global__ __launch_bounds__(CH_SEL_THREADS) void ch_select_kernel(const float* __restrict__ maps, const ChGeom g, int topk, int slices,
                                                                   const unsigned long long* __restrict__ lists,
                                                                   float* __restrict__ boxes, float* __restrict__ scores) {
  __shared__ unsigned long long keys[2 * CH_MAX_TOPK];
  const int group = blockIdx.x, b = group / g.n_cls, c = group - b * g.n_cls, tid = threadIdx.x;
  const int HW = g.H * g.W;
  const unsigned long long* in = lists + (size_t)group * slices * CH_MAX_TOPK;
  keys[tid] = in[tid];  // (a slice's list is sorted already)
  for (int s = 1; s < slices; s++) {
    keys[2 * CH_MAX_TOPK - 1 - tid] = in[(size_t)s * CH_MAX_TOPK + tid];  // reversed: best | next list is a bitonic sequence
    ch_bitonic_merge_desc(keys, 2 * CH_MAX_TOPK);
  }
  __syncthreads();
  if (tid >= topk) return;
  const unsigned long long key = keys[tid];
  float out[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float score = 0.f;
  const unsigned int cell = 0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull);
  if (key != 0ull && cell < (unsigned int)HW) {
    const int iy = (int)cell / g.W, ix = (int)cell - iy * g.W;
    const float* m = maps + (size_t)b * (g.n_cls + 8) * HW + cell;
    const float* r = m + (size_t)g.n_cls * HW;
    const float x = m[(size_t)c * HW];
    out[0] = ((float)ix + r[0]) * g.pxf + g.x_lo;
    out[1] = ((float)iy + r[(size_t)HW]) * g.pyf + g.y_lo;
    out[2] = r[2 * (size_t)HW];
    out[3] = expf(r[3 * (size_t)HW]), out[4] = expf(r[4 * (size_t)HW]), out[5] = expf(r[5 * (size_t)HW]);
    out[6] = atan2f(r[6 * (size_t)HW], r[7 * (size_t)HW]);
    const float e = expf(-fabsf(x));
    score = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  }
  const size_t slot = (size_t)group * topk + tid;  // (B, n_cls * topk): group-major
#pragma unroll
  for (int j = 0; j < 7; j++) boxes[7 * slot + j] = out[j];
  scores[slot] = score;
}

// ---- host

static int ch_geom(ChGeom& g, const double* geom_host, int n_cls, int H, int W) {
  g.px = geom_host[0], g.py = geom_host[1];
  g.pxf = (float)geom_host[0], g.pyf = (float)geom_host[1], g.x_lo = (float)geom_host[2], g.y_lo = (float)geom_host[3];
  g.H = H, g.W = W, g.n_cls = n_cls;
  return g.px > 0.0 && g.py > 0.0 && g.pxf > 0.f && g.pyf > 0.f;
}

extern "C" int v3d_center_targets(const float* boxes, const int32_t* classes, const int32_t* box_offsets_host, int B, int n_cls, int H,
                                  int W, const double* geom_host, double min_overlap, int min_radius, float* heat, int32_t* ind,
                                  uint8_t* mask, int32_t* cls, float* reg, v3d_stream_t stream) {
  if (B < 0 || n_cls < 1 || H < 1 || W < 1 || min_radius < 0) return V3D_EINVAL;
  if (B > CH_MAX_FRAMES || n_cls > CH_MAX_CLS || (long long)H * W > CH_MAX_CELLS) return V3D_EUNSUPPORTED;
  if (!box_offsets_host || !geom_host) return V3D_EINVAL;
  if (B == 0) return V3D_OK;
  ChFrames fr;
  if (box_offsets_host[0] < 0) return V3D_EINVAL;
  for (int b = 0; b <= B; b++) fr.bx[b] = box_offsets_host[b];
  for (int b = 0; b < B; b++) {
    const long long nb = (long long)fr.bx[b + 1] - fr.bx[b];
    if (nb < 0) return V3D_EINVAL;
    if (nb > CH_MAX_OBJ) return V3D_EUNSUPPORTED;
  }
  for (int b = B + 1; b <= CH_MAX_FRAMES; b++) fr.bx[b] = fr.bx[B];
  ChGeom g;
  if (!ch_geom(g, geom_host, n_cls, H, W) || !(min_overlap > 0.0 && min_overlap < 1.0)) return V3D_EINVAL;
  if (!heat || !ind || !mask || !cls || !reg || (fr.bx[B] > 0 && (!boxes || !classes))) return V3D_EINVAL;
  const int tiles = (H * W + V3D_BLOCK - 1) / V3D_BLOCK;
  hipLaunchKernelGGL(ch_targets_kernel, dim3(tiles, n_cls, B), dim3(V3D_BLOCK), 0, (hipStream_t)stream, boxes, classes, fr, g,
                     min_overlap, min_radius, heat, ind, mask, cls, reg);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" size_t v3d_center_loss_workspace(void) { return v3d_align((size_t)(CH_LOSS_BLOCKS + CH_MAX_FRAMES) * sizeof(double)); }

extern "C" int v3d_center_loss_fwd_bwd(const float* maps, const float* heat, const int32_t* ind, const uint8_t* mask, const float* reg,
                                       int B, int n_cls, int H, int W, float alpha, float beta, const float* code_weights_host,
                                       float* losses, float* dmaps, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (B < 1 || n_cls < 1 || H < 1 || W < 1) return V3D_EINVAL;
  if (B > CH_MAX_FRAMES || n_cls > CH_MAX_CLS || (long long)H * W > CH_MAX_CELLS) return V3D_EUNSUPPORTED;
  if (!maps || !heat || !ind || !mask || !reg || !code_weights_host || !losses || !dmaps || !workspace) return V3D_EINVAL;
  if (workspace_bytes < v3d_center_loss_workspace() || ((uintptr_t)workspace & 7)) return V3D_EWORKSPACE;
  const int HW = H * W;
  const long long total = (long long)B * (n_cls + 8) * HW;
  const int blocks = (int)std::min<long long>(CH_LOSS_BLOCKS, (total + V3D_BLOCK - 1) / V3D_BLOCK);
  double* heat_partial = (double*)workspace;
  double* box_partial = heat_partial + CH_LOSS_BLOCKS;
  ChWeights cw;
  for (int j = 0; j < 8; j++) cw.w[j] = code_weights_host[j];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ch_loss_heat_kernel, dim3(blocks), dim3(V3D_BLOCK), 0, st, maps, heat, mask, B, n_cls, HW, alpha, beta, dmaps,
                     heat_partial);
  hipLaunchKernelGGL(ch_loss_box_kernel, dim3(B), dim3(CH_MAX_OBJ), 0, st, maps, ind, mask, reg, B, n_cls, HW, cw, dmaps, box_partial);
  hipLaunchKernelGGL(ch_loss_finalize_kernel, dim3(1), dim3(CH_FIN_THREADS), 0, st, (const double*)heat_partial, blocks,
                     (const double*)box_partial, B, mask, losses);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_center_loss_scale(float* dmaps, int B, int n_cls, int H, int W, const float* g_hm, const float* g_reg,
                                     v3d_stream_t stream) {
  if (B < 1 || n_cls < 1 || H < 1 || W < 1) return V3D_EINVAL;
  if (B > CH_MAX_FRAMES || n_cls > CH_MAX_CLS || (long long)H * W > CH_MAX_CELLS) return V3D_EUNSUPPORTED;
  if (!dmaps || !g_hm || !g_reg) return V3D_EINVAL;
  // heat channels *= *g_hm, box channels *= *g_reg
  const long long HW = (long long)H * W, period = (n_cls + 8) * HW;
  return v3d_i_loss_scale(dmaps, B, period, n_cls * HW, g_hm, g_reg, 2048, (hipStream_t)stream);
}

extern "C" size_t v3d_center_decode_workspace(int B, int n_cls, int H, int W) {
  if (B < 1 || n_cls < 1 || H < 1 || W < 1 || (long long)H * W > CH_MAX_CELLS) return 0;
  const size_t slices = ((size_t)H * W + CH_SLICE - 1) / CH_SLICE;
  return v3d_align((size_t)B * n_cls * slices * CH_MAX_TOPK * sizeof(unsigned long long));
}

extern "C" int v3d_center_decode(const float* maps, int B, int n_cls, int H, int W, const double* geom_host, int topk, float* boxes,
                                 float* scores, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (B < 1 || n_cls < 1 || H < 1 || W < 1 || topk < 1) return V3D_EINVAL;
  if (B > CH_MAX_FRAMES || n_cls > CH_MAX_CLS || topk > CH_MAX_TOPK || (long long)H * W > CH_MAX_CELLS) return V3D_EUNSUPPORTED;
  ChGeom g;
  if (!maps || !geom_host || !boxes || !scores || !workspace || !ch_geom(g, geom_host, n_cls, H, W)) return V3D_EINVAL;
  if (workspace_bytes < v3d_center_decode_workspace(B, n_cls, H, W) || ((uintptr_t)workspace & 7)) return V3D_EWORKSPACE;
  const int slices = (H * W + CH_SLICE - 1) / CH_SLICE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* lists = (unsigned long long*)workspace;
  hipLaunchKernelGGL(ch_peaks_kernel, dim3(slices, B * n_cls), dim3(V3D_BLOCK), 0, st, maps, n_cls, H, W, topk, lists);
  hipLaunchKernelGGL(ch_select_kernel, dim3(B * n_cls), dim3(CH_SEL_THREADS), 0, st, maps, g, topk, slices,
                     (const unsigned long long*)lists, boxes, scores);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}
