// dense_train.hip -- the dense half of a SECOND TRAIN step on the matrix cores (BASELINE configs[2]; VERDICT r2 "J1").
//
// Reference: RPN = 7 x [Conv2d(128 -> 128, 3x3 pad 1 | 1x1, no bias) + BatchNorm2d(batch statistics) + ReLU]
// (vision3d/detector/second.py:58-94) + the two 1x1 heads (detector/proposal.py:19-22), forward and backward, which
// train.py:58-66 runs under autograd through cuDNN.  Rounds 1-2 left this half to MIOpen (bf16 autocast, channels_last);
// here it is hand-written, bf16 storage / fp32 accumulation -- the arithmetic of that autocast path (bf16 pack / unpack and the
// hi / lo split of the fp32-class planes: split_prec.h):
//
//   dt_conv3_kernel,      implicit-GEMM convolution (3x3 | 1x1), NHWC bf16 -> NHWC bf16 (the raw, pre-BatchNorm output) + per-workgroup
//   dt_conv_kernel        channel sums for the batch statistics.  The SAME kernel on a transposed / tap-flipped weight image is the
//                         data gradient.
//   dt_bn_*               batch statistics (fixed-order reduction of the per-tile sums, running statistics), normalise + ReLU,
//                         and the backward pair (channel sums of dy and dy * x_hat, then the input gradient).
//   dt_wgrad_kernel       weight gradient dW[tap][ci][co] = sum_pixels X[p + tap][ci] * dY[p][co] straight from the NHWC tensors:
//                         both MFMA operands need the REDUCTION index (pixels) contiguous per lane, which NHWC does not give --
//                         the fragments come out of LDS through the gfx950 transpose read (ds_read_b64_tr_b16).
//   dt_head_*             the fused [cls | reg] 1x1 head (<= 64 output channels, with bias): VALU kernels, it is a stream.
//
// Every reduction (batch statistics, dgamma / dbeta, dW, head gradients) is two-level in a fixed order: results are
// bit-repeatable, no atomics.
//
// The step runs in two arithmetics -- bf16 storage, and the fp32-class split storage ("bf16x3": every tensor a hi + lo pair of bf16
// planes, DtT) -- through ONE pair of drivers at the end of this file (dt_forward / dt_backward, "one call per direction"): the
// element-wise and reduction kernels serve both (a nullable lo plane), the few steps that differ are the dt_step_* helpers.
#include "v3d_internal.h"
#include "split_prec.h"

// the inference head's convolution (dense_conv.hip v3d_conv2d_nhwc_split) on bf16x3 images, every tile convolved
static inline int dt_conv2d_plain(const void* x_hi, const void* x_lo, const void* weight_image, const float* bias, int relu, int B, int H, int W,
                                  int Cin, int Cout, int ksize, void* y_hi, void* y_lo, float* y_nchw, v3d_stream_t stream) {
  return v3d_conv2d_nhwc_split(x_hi, x_lo, weight_image, bias, relu, B, H, W, Cin, Cout, ksize, y_hi, y_lo, y_nchw, nullptr, 0, nullptr, nullptr,
                               nullptr, nullptr, nullptr, 0, nullptr, stream);
}

typedef unsigned short dt_bf16;  // storage type at the C ABI

// Split storage (the fp32-class training path, "bf16x3"): a tensor is TWO bf16 planes, value = hi + lo (hi = RNE(v), lo = RNE(v - hi):
// 16 significant bits, the operand format of the 3-term products of csrc/dense_conv.hip; the split itself: split_prec.h PREC 0).  The elementwise / reduction kernels below
// take a nullable `lo` plane beside every bf16 tensor: null = the bf16-storage path, unchanged.
__device__ __forceinline__ void dt_load8(const dt_bf16* __restrict__ hi, const dt_bf16* __restrict__ lo, long long off, float (&v)[8]) {
  bf16_unpack8(*reinterpret_cast<const u32x4*>(hi + off), v);
  if (lo) {
    float w[8];
    bf16_unpack8(*reinterpret_cast<const u32x4*>(lo + off), w);
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] += w[e];
  }
}
__device__ __forceinline__ void dt_store8(dt_bf16* __restrict__ hi, dt_bf16* __restrict__ lo, long long off, const float (&v)[8]) {
  u32x4 h, l;
  split_act<0>(v, 1.f, h, l);
  *reinterpret_cast<u32x4*>(hi + off) = h;
  if (lo) *reinterpret_cast<u32x4*>(lo + off) = l;
}
// the host side's handle of such a tensor (NHWC bf16 planes); lo == nullptr: bf16 storage
struct DtT {
  unsigned char* hi;
  unsigned char* lo;
};
static inline DtT dt_t(const void* hi, const void* lo = nullptr) { return DtT{(unsigned char*)hi, (unsigned char*)lo}; }
#define DT_TRY(call) do { const int rc_ = (call); if (rc_ != V3D_OK) return rc_; } while (0)

#define DT_C 128          // channels of every RPN convolution (Cin = Cout)
#define DT_BM 128         // pixels per tile
#define DT_THREADS 512    // 4 matrix waves + 4 loader waves
#define DT_TS (DT_C + 4)  // fp32 epilogue tile row stride
#define DT_A_BYTES (DT_BM * DT_C * 2)        // one stage of A: 128 pixels x 128 channels bf16
#define DT_B_BYTES (4 * 8 * 1024)            // one stage of B: 4 k-substeps x 8 cout tiles x 1 KB fragments
#define DT_STAGE (DT_A_BYTES + DT_B_BYTES)
#define DT_SMEM (2 * DT_STAGE)               // 128 KB: two stages (>= the fp32 epilogue tile + the statistics scratch)

__device__ __attribute__((aligned(16))) const unsigned dt_zero16[4] = {0u, 0u, 0u, 0u};  // halo source of the LDS-DMA gather
// LDS byte address of a __shared__ object: the low half of its generic address (flat aperture base in the high half)
__device__ __forceinline__ unsigned lds_addr_dt(const void* p) { return (unsigned)(unsigned long long)p; }

// ------------------------------------------------------------------------------------------------ weights
// (Cout, Cin, k, k) fp32 -> bf16 fragment image img[tap][ss = ci/32][nt = co/16][lane][8]: lane (j = lane & 15, kg = lane >> 4)
// holds B[k = ss*32 + kg*8 + e][n = nt*16 + j].  transpose = 0: B[ci][co] = W[co][ci][tap] (forward).  transpose = 1: the data
// gradient as a convolution of dY: B[k = co][n = ci] = W[co][ci][taps - 1 - tap] (taps flipped, channels swapped).
__device__ __forceinline__ float dt_pack_value(const float* __restrict__ w, int taps, int transpose, int t) {  // element t of the image
  int r = t;
  const int e = r % 8; r /= 8;
  const int lane = r % 64; r /= 64;
  const int nt = r % 8; r /= 8;
  const int ss = r % 4; r /= 4;
  const int tap = r;
  const int k = ss * 32 + (lane >> 4) * 8 + e, n = nt * 16 + (lane & 15);
  return transpose ? w[((size_t)k * DT_C + n) * taps + (taps - 1 - tap)] : w[((size_t)n * DT_C + k) * taps + tap];
}
__global__ void dt_pack_weights_kernel(const float* __restrict__ w, int taps, int transpose, dt_bf16* __restrict__ img) {
  const int total = taps * 4 * 8 * 64 * 8;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x)
    img[t] = bf16_from_f32(dt_pack_value(w, taps, transpose, t));
}

extern "C" size_t v3d_dense_train_weight_image_bytes(int ksize) { return (size_t)ksize * ksize * DT_B_BYTES; }

// every layer's two images (forward, data gradient) in ONE launch: blockIdx.y = 2 layer + transpose (a pack is ~5 us of launch
// and ~1 us of work; 14 of them per step were 1 % of it)
struct DtPackJobs {
  const float* w[16];
  int taps[16];
};
__global__ void dt_pack_all_kernel(DtPackJobs jobs, unsigned char* __restrict__ images, size_t stride) {
  const int l = blockIdx.y >> 1, transpose = blockIdx.y & 1, taps = jobs.taps[l];
  const float* __restrict__ w = jobs.w[l];
  dt_bf16* __restrict__ img = reinterpret_cast<dt_bf16*>(images + (size_t)blockIdx.y * stride);
  const int total = taps * 4 * 8 * 64 * 8;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x)
    img[t] = bf16_from_f32(dt_pack_value(w, taps, transpose, t));
}

extern "C" int v3d_dense_train_pack_weights(const float* weight, int ksize, int transpose, void* image, v3d_stream_t stream) {
  if (!weight || !image || (ksize != 1 && ksize != 3)) return V3D_EINVAL;
  hipLaunchKernelGGL(dt_pack_weights_kernel, dim3(128), dim3(256), 0, (hipStream_t)stream, weight, ksize * ksize, transpose ? 1 : 0,
                     (dt_bf16*)image);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ------------------------------------------------------------------------------------------------ convolution
// The general form, templated on the kernel size.  Only KS = 1 is instantiated -- the RPN's 1x1 layer and its data gradient; the 3x3
// layers are the 2-D tile kernel's, below.  (The parameter stays: written out for one tap, the loaders compile to other code --
// the compiler does not fold the tap index of a stage, (G % 2) >> 1, to zero -- and a rewrite of this kernel wants a measurement.)
// Tile = 128 pixels x 128 couts; stage = 64 input channels of one tap (A: 128 pixel rows x 128 B = 16 KB, B: 2 k-substeps x 8 cout
// tiles x 1 KB = 16 KB); the stages of ALL tiles of a (persistent) workgroup stream through a ring of 4 LDS slots.
// Waves 4-7 LOAD, three stages ahead (LDS-DMA, hand-counted vmcnt, raw barriers): 8 consecutive lanes fetch the 128 bytes of one
// pixel row (row-contiguous requests, see tools/mb_gather.hip; zero halo), the weight fragments come linearly from the packed
// image.  With two 64 KB stages and one stage of look-ahead the kernel ran at one memory round trip per stage (137 us per
// 3x3 layer at bs = 8 against 33 us of MFMA): a stage is ~1 000 clocks of matrix work, a round trip several thousand, and the
// CU needs ~100 KB in flight to keep its L2 fill rate.
// Waves 0-3 MULTIPLY: wave (ph = w & 1, ch = w >> 1) owns pixel tiles 4 ph .. 4 ph + 3 x cout tiles 4 ch .. 4 ch + 3 (16
// accumulators); per 32-channel substep 4 A + 4 B fragment reads for 16 MFMAs.  One barrier per stage.
// Epilogue (per tile, while the loaders keep prefetching the next tile): the accumulators go through a 17 KB LDS scratch in four
// quarters of 32 pixels -> bf16 NHWC, 16-byte stores.  With `stats`: channel sums and sums of squares OF THE ROUNDED VALUES (what
// the backward pass reads back), accumulated over all tiles of the workgroup in tile order -> stats[workgroup][2][128].
#define DT_NSLOT 4
#define DT_SLOT 32768
#define DT_SCRATCH (32 * DT_TS * 4)
#define DT_CONV_SMEM (DT_NSLOT * DT_SLOT + DT_SCRATCH)  // 128 KB + 16.5 KB
#define DT_CONV_GRID 256
template <int KS>
__global__ __launch_bounds__(DT_THREADS) void dt_conv_kernel(const dt_bf16* __restrict__ x, const dt_bf16* __restrict__ w_img,
                                                             int B, int H, int W, dt_bf16* __restrict__ y,
                                                             float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dt_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = B * H * W;
  const int ntiles = (M + DT_BM - 1) / DT_BM;
  constexpr int SPT = 2 * KS * KS;  // stages per tile
  const int my_tiles = blockIdx.x < ntiles ? (ntiles - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  const int nstage = my_tiles * SPT;
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;

  if (wave >= 4) {
    // ------------------------------------------------------------------ loaders
    const int lw = wave - 4;
    const int sub = lane >> 3, slot8 = lane & 7;  // pixel of the request (8 per instruction), 16-byte part of its 128 bytes
    auto issue = [&](int G) {
      const int tile = blockIdx.x + (G / SPT) * gridDim.x, s = G % SPT;
      const int tap = s >> 1, hf = s & 1;
      const int dy = KS == 3 ? tap / 3 - 1 : 0, dx = KS == 3 ? tap % 3 - 1 : 0;
      unsigned char* A = dt_smem + (G % DT_NSLOT) * DT_SLOT;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int px = (j * 4 + lw) * 8 + sub;  // pixel row of the tile
        const int m = tile * DT_BM + px;
        const int b = m / (H * W), rem = m - b * H * W;
        const int h = rem / W, wq = rem - h * W;
        const int hh = h + dy, ww = wq + dx;
        const bool ok = m < M && hh >= 0 && hh < H && ww >= 0 && ww < W;
        const int part = slot8 ^ ((px >> 1) & 7);  // LDS slot `slot8` of pixel px holds channel part slot8 ^ swizzle(px)
        const dt_bf16* src = ok ? x + (size_t)(m + dy * W + dx) * DT_C + hf * 64 + part * 8 : reinterpret_cast<const dt_bf16*>(dt_zero16);
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(A + (j * 4 + lw) * 1024), 16, 0, 0);
      }
      const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(w_img) + (size_t)tap * DT_B_BYTES + hf * 16384 + lw * 4096 + lane * 16;
      unsigned char* Bd = A + 16384 + lw * 4096;
#pragma unroll
      for (int j = 0; j < 4; j++) __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + j * 1024), (lptr_t)(Bd + j * 1024), 16, 0, 0);
    };
    for (int a = 0; a < DT_NSLOT - 1; a++)
      if (a < nstage) issue(a);
    for (int G = 0; G < nstage; G++) {
      const int younger = min(DT_NSLOT - 2, nstage - 1 - G);  // stages in flight behind G (8 requests each from this wave)
      if (younger >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_barrier" ::: "memory");  // stage G readable; stage G - 1 is finished everywhere: its slot is free
      if (G + DT_NSLOT - 1 < nstage) issue(G + DT_NSLOT - 1);
      if (G % SPT == SPT - 1) {  // the multipliers' epilogue: 8 barriers the loaders take part in (their requests stay in flight)
#pragma unroll
        for (int q = 0; q < 8; q++) asm volatile("s_barrier" ::: "memory");
      }
    }
    asm volatile("s_barrier\n\ts_barrier" ::: "memory");  // the statistics exchange at the end of the multipliers
  } else {
    // ------------------------------------------------------------------ multipliers
    const int ph = wave & 1, ch = wave >> 1;
    const int c8 = tid & 15, rg = tid >> 4;  // epilogue role: 8 consecutive couts, scratch rows rg and rg + 16
    float s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; e++) s1[e] = s2[e] = 0.f;
    float* tl = reinterpret_cast<float*>(dt_smem + DT_NSLOT * DT_SLOT);
    f32x4 acc[4][4];
    for (int G = 0; G < nstage; G++) {
      const int s = G % SPT;
      if (s == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      asm volatile("s_barrier" ::: "memory");  // (pairs with the loaders' barrier of stage G)
      const unsigned char* A = dt_smem + (G % DT_NSLOT) * DT_SLOT;
      const unsigned char* Bs = A + 16384;
      // two fragment sets: the 8 reads of substep 1 are in flight while the 16 MFMAs of substep 0 issue
      bf16x8 fa[2][4], fb[2][4];
      auto frags = [&](int ss, bf16x8 (&a)[4], bf16x8 (&b)[4]) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int px = (ph * 4 + i) * 16 + (lane & 15);
          a[i] = *reinterpret_cast<const bf16x8*>(A + px * 128 + (((ss * 4 + (lane >> 4)) ^ ((px >> 1) & 7)) << 4));
        }
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = *reinterpret_cast<const bf16x8*>(Bs + (ss * 8 + ch * 4 + j) * 1024 + lane * 16);
      };
      frags(0, fa[0], fb[0]);
      frags(1, fa[1], fb[1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ss = 0; ss < 2; ss++) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ss][i], fb[ss][j], acc[i][j], 0, 0, 0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage's fragments are in registers before its slot is handed back
      if (s == SPT - 1) {
        // ---- epilogue of the tile, four quarters of 32 pixels through the scratch (the ring stays untouched)
        const int tile = blockIdx.x + (G / SPT) * gridDim.x, m0 = tile * DT_BM;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (ph == (q >> 1)) {
#pragma unroll
            for (int i2 = 0; i2 < 2; i2++)
#pragma unroll
              for (int j = 0; j < 4; j++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                  tl[(i2 * 16 + (lane >> 4) * 4 + r) * DT_TS + (ch * 4 + j) * 16 + (lane & 15)] = acc[(q & 1) * 2 + i2][j][r];
          }
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
          for (int k = 0; k < 2; k++) {
            const int row = rg + 16 * k, m = m0 + q * 32 + row;
            if (m < M) {
              const f32x4 t0 = *reinterpret_cast<const f32x4*>(tl + row * DT_TS + c8 * 8);
              const f32x4 t1 = *reinterpret_cast<const f32x4*>(tl + row * DT_TS + c8 * 8 + 4);
              const u32x4 v = {bf16_pack2(t0[0], t0[1]), bf16_pack2(t0[2], t0[3]), bf16_pack2(t1[0], t1[1]), bf16_pack2(t1[2], t1[3])};
              *reinterpret_cast<u32x4*>(y + (size_t)m * DT_C + c8 * 8) = v;
              if (stats) {
                float xr[8];
                bf16_unpack8(v, xr);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                  s1[e] += xr[e];
                  s2[e] = fmaf(xr[e], xr[e], s2[e]);
                }
              }
            }
          }
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // everyone has read the quarter
        }
      }
    }
    // ---- the workgroup's statistics: 16 row groups -> one partial per channel, in row-group order
    if (stats) {
#pragma unroll
      for (int e = 0; e < 8; e++) {
        tl[(rg * 2 + 0) * DT_C + c8 * 8 + e] = s1[e];
        tl[(rg * 2 + 1) * DT_C + c8 * 8 + e] = s2[e];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (stats) {
      const int which = tid / DT_C, c = tid % DT_C;  // 256 multiplier threads = 2 x 128
      float a = 0.f;
      for (int g = 0; g < 16; g++) a += tl[(g * 2 + which) * DT_C + c];
      stats[((size_t)blockIdx.x * 2 + which) * DT_C + c] = a;
    }
    asm volatile("s_barrier" ::: "memory");
  }
}

// ------------------------------------------------------------------------------------------------ 3x3 convolution, 2-D tiles
// The kernel above reads every input pixel row once PER TAP: nine times the activation tensor (650 MB per layer at bs = 8) through
// L2 slices that cannot hold a tile's three-row neighbourhood for every CU -- measured 135-172 us per layer, HBM / Infinity-Cache
// bound, against 33 us of MFMA.  Here a tile is a 16 x 16 block of output pixels x all 128 couts; its (16 + 2) x (16 + 2) input
// neighbourhood is brought into LDS ONCE, as two 64-channel slices (324 pixel rows x 128 B = 41 KB each, zero halo, chunk p of
// pixel row hp stored at chunk p ^ (hp & 7): every ds_read_b128 lane group then covers the 16 slots of the 256-byte bank row once,
// for every tap alignment), each slice loaded while the other multiplies.  The reduction runs slice-outer, tap-inner: stage =
// (slice, tap) = 64 channels x 128 couts = 16 KB of weight fragments through a ring of 4 slots.
//
// What bounds this kernel is the ISSUE cost of LDS-DMA requests while the LDS is busy serving fragment reads (100-185 clocks per
// 1 KB request, MI355X_MICROARCH.md): the first version (8 x 16 tiles, 256-byte pixel rows) issued 333 requests per 128 pixels
// -- 12 k clocks per loading wave against 9.2 k clocks of MFMA, measured 107 us per layer; with 256-pixel tiles the weight stages
// are amortised over twice the MFMAs (185 requests per 128 pixels).
//
// Waves 8-11 load.  Waves 0-7 multiply, two per SIMD: wave (pq, ch) owns block rows 4 pq .. 4 pq + 3 (four 16-pixel tiles) x couts
// 64 ch .. 64 ch + 63 (four tiles): 16 accumulators, 16 fragment reads per 32 MFMAs.  The WEIGHTS are the MFMA's row operand, so a
// lane ends up with four consecutive couts of one pixel: the epilogue is one 8-byte store per accumulator straight from registers
// (no LDS round trip, no barrier), and the batch statistics accumulate in registers over all tiles of the workgroup.
// One barrier per stage, in the MIDDLE of its MFMAs: the second half's fragments are requested before the first half multiplies,
// the next stage's first half (its weights landed a stage early) before the second half does.
#ifndef DT_TIMELINE
#define DT_TIMELINE 0  // 1: cycle-counter stamps of workgroup 8 (tools/mb_dense_train.py prints them)
#endif
#if DT_TIMELINE
__device__ unsigned long long dt_tl[2][128];
extern "C" int v3d_debug_dense_train_timeline(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(dt_tl), sizeof(dt_tl));
}
#define DT_STAMP(role, idx) do { if (blockIdx.x == 8 && lane == 0 && (wave == 0 || wave == 8) && (idx) < 128) dt_tl[role][idx] = __builtin_readcyclecounter(); } while (0)
#else
#define DT_STAMP(role, idx)
#endif
#define DT3_TH 8                                  // (tile of the weight-gradient kernel)
#define DT3_TW 16
#define DT3_HALO ((DT3_TH + 2) * (DT3_TW + 2))
#define DC3_T 16                                  // 16 x 16 output pixels
#define DC3_HW (DC3_T + 2)
#define DC3_HALO (DC3_HW * DC3_HW)                // 324 pixel rows
#define DC3_APIECES ((DC3_HALO + 7) / 8)          // 41 LDS-DMA requests of 8 pixel rows x 128 B
#define DC3_ABUF (DC3_APIECES * 1024)             // 41 984 B per slice
#define DC3_BSLOT 16384
#define DC3_NB 4
#define DC3_SMEM (2 * DC3_ABUF + DC3_NB * DC3_BSLOT)  // 83 968 + 65 536 = 149 504 B
#define DC3_THREADS 768                           // 8 multiplying waves (two per SIMD) + 4 loading waves
#define DC3_SPT 18                                // stages per tile: 2 slices x 9 taps
// Reduce-scatter over the 16 lanes that share lane >> 4: returns, to lane l (= lane & 15), the sum over those lanes of v[l].
// Four halving steps (lane bit 3 picks the upper or lower eight values and sends the others to its partner, ...): a fixed tree.
// The exchanges are DPP row rotations / quad permutes and one ds_swizzle: no address arithmetic, no LDS traffic.
__device__ __forceinline__ float dt_x8(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128 /* row_ror:8 */, 0xf, 0xf, false)); }
__device__ __forceinline__ float dt_x4(float x) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x101f /* xor 4 */)); }
__device__ __forceinline__ float dt_x2(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4e /* quad_perm 2,3,0,1 */, 0xf, 0xf, false)); }
__device__ __forceinline__ float dt_x1(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xb1 /* quad_perm 1,0,3,2 */, 0xf, 0xf, false)); }
__device__ __forceinline__ float dt_rs16(const float (&v)[16], int l) {
  float k8[8], k4[4], k2[2];
  const bool h3 = l & 8, h2 = l & 4, h1 = l & 2, h0 = l & 1;
#pragma unroll
  for (int i = 0; i < 8; i++) k8[i] = (h3 ? v[8 + i] : v[i]) + dt_x8(h3 ? v[i] : v[8 + i]);
#pragma unroll
  for (int i = 0; i < 4; i++) k4[i] = (h2 ? k8[4 + i] : k8[i]) + dt_x4(h2 ? k8[i] : k8[4 + i]);
#pragma unroll
  for (int i = 0; i < 2; i++) k2[i] = (h1 ? k4[2 + i] : k4[i]) + dt_x2(h1 ? k4[i] : k4[2 + i]);
  return (h0 ? k2[1] : k2[0]) + dt_x1(h0 ? k2[0] : k2[1]);
}
template <int N> __device__ __forceinline__ void dt_vmwait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__global__ __launch_bounds__(DC3_THREADS) void dt_conv3_kernel(const dt_bf16* __restrict__ x, const dt_bf16* __restrict__ w_img,
                                                               int B, int H, int W, dt_bf16* __restrict__ y,
                                                               float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dt_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tx_n = (W + DC3_T - 1) / DC3_T, ty_n = (H + DC3_T - 1) / DC3_T;
  const int ntiles = B * ty_n * tx_n;
  const int my_tiles = blockIdx.x < ntiles ? (ntiles - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  const int nstage = my_tiles * DC3_SPT;
  unsigned char* const abuf = dt_smem;                      // [2 slices][41 x 1 KB]
  unsigned char* const bring = dt_smem + 2 * DC3_ABUF;      // [4][16 KB]
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto tile_origin = [&](int t, int& b, int& y0, int& x0) {  // wave-uniform: scalar registers
    const int tile = __builtin_amdgcn_readfirstlane(blockIdx.x + t * gridDim.x);
    b = tile / (ty_n * tx_n);
    const int r = tile - b * ty_n * tx_n;
    y0 = (r / tx_n) * DC3_T;
    x0 = (r % tx_n) * DC3_T;
  };

  if (wave >= 8) {
    // ------------------------------------------------------------------ loaders
    // (they share their SIMDs with two multiplying waves each: at equal priority every address instruction of a request waits
    // for a gap between MFMAs -- measured ~160 clocks per weight request, ~900 per slice request)
    __builtin_amdgcn_s_setprio(3);
    const int lw = wave - 8;
    const int sub = lane >> 3, slot = lane & 7;
    int nb = 0, ny0 = 0, nx0 = 0;  // origin of the tile whose slice is being requested
    // request k of this loader = piece 4 k + lw: the lane's pixel row (hy, hx) of the neighbourhood and its byte offset from the
    // tile's first pixel are fixed -- tabulated once (computed per request, this address arithmetic was most of a request's cost)
    int tab_yx[11], tab_rel[11];
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const int hp = (4 * k + lw) * 8 + sub;
      const int hy = hp / DC3_HW, hx = hp - hy * DC3_HW;
      tab_yx[k] = hp < DC3_HALO ? (hy | (hx << 16)) : 0x7fff;  // (row 32767 is outside every image)
      tab_rel[k] = ((hy - 1) * W + (hx - 1)) * (DT_C * 2) + ((slot ^ (hp & 7)) << 4);
    }
    const unsigned char* tile_base = nullptr;  // first pixel of the tile being requested (wave-uniform)
    auto issue_a = [&](int h, int k) {  // 8 pixel rows x 64 channels of slice h of the tile at (nb, ny0, nx0)
      const int yy = ny0 - 1 + (tab_yx[k] & 0xffff), xx = nx0 - 1 + (tab_yx[k] >> 16);
      const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
      const unsigned char* src = ok ? tile_base + (long long)(tab_rel[k] + h * 128) : reinterpret_cast<const unsigned char*>(dt_zero16);
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(abuf + h * DC3_ABUF + (4 * k + lw) * 1024), 16, 0, 0);
    };
    auto new_tile = [&](int t) {
      tile_origin(t, nb, ny0, nx0);
      tile_base = reinterpret_cast<const unsigned char*>(x + (((size_t)nb * H + ny0) * W + nx0) * DT_C);
    };
    auto issue_b = [&](int G) {  // stage G = (tile, slice h, tap): 16 KB of weight fragments
      const int s = G % DC3_SPT, h = s / 9, tap = s - 9 * h;
      const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(w_img) + (size_t)tap * DT_B_BYTES + h * 16384 + lw * 4096 + lane * 16;
      unsigned char* Bd = bring + (G % DC3_NB) * DC3_BSLOT + lw * 4096;
#pragma unroll
      for (int j = 0; j < 4; j++) __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + j * 1024), (lptr_t)(Bd + j * 1024), 16, 0, 0);
    };
    // Slice sl (= 2 tile + h, multiplied in stages 9 sl .. 9 sl + 8) is requested in iterations 9 sl - 9 .. 9 sl - 2 -- its buffer is
    // released by barrier 9 sl - 9, and a request issued in iteration i is older than weight stage i + 3, whose landing barrier
    // i + 2 waits for.  11 requests per loader in 8 iterations: k = i' and, for i' < 3, k = 8 + i'; piece = 4 k + lw (< 41).
    auto issue_slice_part = [&](int G) -> int {  // returns the number of requests issued
      const int sl = G / 9 + 1, ip = G - 9 * (sl - 1);
      if (sl >= 2 * my_tiles || ip >= 8) return 0;
      if (ip == 0 && (sl & 1) == 0) new_tile(sl >> 1);
      // (k as a compile-time index of the tables: a switch over the iteration within the slice)
      int n = 1;
      switch (ip) {
        case 0: issue_a(sl & 1, 0); if (32 + lw < DC3_APIECES) { issue_a(sl & 1, 8); n = 2; } break;
        case 1: issue_a(sl & 1, 1); if (36 + lw < DC3_APIECES) { issue_a(sl & 1, 9); n = 2; } break;
        case 2: issue_a(sl & 1, 2); if (40 + lw < DC3_APIECES) { issue_a(sl & 1, 10); n = 2; } break;
        case 3: issue_a(sl & 1, 3); break;
        case 4: issue_a(sl & 1, 4); break;
        case 5: issue_a(sl & 1, 5); break;
        case 6: issue_a(sl & 1, 6); break;
        default: issue_a(sl & 1, 7); break;
      }
      return n;
    };
    int na_prev = 0;
    if (nstage > 0) {
      new_tile(0);
#pragma unroll
      for (int k = 0; k < 11; k++)
        if (4 * k + lw < DC3_APIECES) issue_a(0, k);
      issue_b(0);
      issue_b(1);
      issue_b(2);
      dt_vmwait<4>();  // slice 0, stages 0 and 1
      asm volatile("s_barrier" ::: "memory");
      na_prev = issue_slice_part(0);
      if (3 < nstage) issue_b(3);
    }
    for (int G = 1; G < nstage; G++) {
      // barrier G promises: weight stage G + 1 and every request older than it have landed.  Younger than it: the slice requests of
      // iteration G - 1 and weight stage G + 2.
      const int younger = __builtin_amdgcn_readfirstlane((G + 1 < nstage ? na_prev : 0) + (G + 2 < nstage ? 4 : 0));
      DT_STAMP(1, 4 * G);
      if (younger >= 6) dt_vmwait<6>();
      else if (younger == 5) dt_vmwait<5>();
      else if (younger == 4) dt_vmwait<4>();
      else dt_vmwait<0>();
      DT_STAMP(1, 4 * G + 1);
      asm volatile("s_barrier" ::: "memory");  // stage G - 1 is finished everywhere: its weight slot is free
      DT_STAMP(1, 4 * G + 2);
      na_prev = issue_slice_part(G);
      if (G + 3 < nstage) issue_b(G + 3);
      DT_STAMP(1, 4 * G + 3);
    }
    if (nstage > 0) asm volatile("s_barrier" ::: "memory");  // the multipliers' last one
    asm volatile("s_barrier\n\ts_barrier" ::: "memory");     // the statistics exchange
  } else {
    // ------------------------------------------------------------------ multipliers
    const int pq = wave & 3, ch = wave >> 2;
    const int kg = lane >> 4, pxl = lane & 15;
    f32x4 acc[4][4];   // [cout tile][pixel tile]
    // batch statistics: after every tile the 16 pixel-column lanes of a cout group reduce-scatter their 16 (cout tile, r) sums in a
    // fixed tree (dt_rs16), so that lane (pxl, kg) carries ONE channel -- 64 ch + 16 (pxl >> 2) + 4 kg + (pxl & 3) -- over all tiles
    float st1 = 0.f, st2 = 0.f;
    bf16x8 wf[2][4], xf[2][4];  // [32-channel substep][tile]
    // Fragment addresses.  Pixel fragment of (tap (ty, tx), pixel tile pt, substep ss), lane (pxl, kg): pixel row hp = q + c with
    // q = 72 pq + pxl (the lane's part) and c = 18 (ty + pt) + tx (a constant of the unrolled stage); byte address
    // 128 hp + 16 ((4 ss + kg) ^ (hp & 7)).  (hp & 7) only depends on c through c & 7: eight per-lane bases pw[c & 7], everything
    // else is the instruction's immediate offset; substep 1 is the same address with bit 6 flipped.  (Computed per read, these
    // addresses were ~40 VALU instructions per half stage in the shadow of 16 MFMAs.)
    typedef const __attribute__((address_space(3))) unsigned char* lds_t;
    const lds_t lds = (lds_t)dt_smem;
    unsigned pw[8];
    {
      const int q = pq * 4 * DC3_HW + pxl;
#pragma unroll
      for (int jj = 0; jj < 8; jj++) pw[jj] = (unsigned)(q * 128 + ((kg ^ ((q + jj) & 7)) << 4));
    }
    const unsigned wlane = (unsigned)(2 * DC3_ABUF + ch * 4096 + lane * 16);
    auto read_w = [&](unsigned wb, int ss, bf16x8 (&w)[4]) {  // wb: wlane + 16 KB x ring slot
#pragma unroll
      for (int ct = 0; ct < 4; ct++) w[ct] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(lds + wb + (ss * 8 + ct) * 1024);
    };
    auto read_x = [&](int s, int ss, bf16x8 (&xv)[4]) {  // s = stage within the tile: a constant of the unrolled body
      const int h = s >= 9 ? 1 : 0, tap = s - 9 * h;
      const int ty = tap / 3, tx = tap - 3 * ty;
#pragma unroll
      for (int pt = 0; pt < 4; pt++) {
        const int c = (ty + pt) * DC3_HW + tx;
        xv[pt] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(lds + (pw[c & 7] ^ (unsigned)(ss << 6)) + (h * DC3_ABUF + c * 128));
      }
    };
    if (nstage > 0) {
      asm volatile("s_barrier" ::: "memory");  // slice 0 and weight stages 0, 1 are readable
      read_w(wlane, 0, wf[0]);
      read_x(0, 0, xf[0]);
    }
#pragma unroll 1
    for (int t = 0; t < my_tiles; t++) {
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int p = 0; p < 4; p++) acc[a][p] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int slot0 = __builtin_amdgcn_readfirstlane((2 * t) & 3);  // 18 stages per tile: the ring position advances by 2 per tile
#pragma unroll
      for (int s = 0; s < DC3_SPT; s++) {
        const unsigned wb = wlane + (unsigned)(((slot0 + s) & 3) << 14), wbn = wlane + (unsigned)(((slot0 + s + 1) & 3) << 14);
        if (t == 0 && s < 14) DT_STAMP(0, 4 * s);
        read_w(wb, 1, wf[1]);
        read_x(s, 1, xf[1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int p = 0; p < 4; p++) acc[a][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][a], xf[0][p], acc[a][p], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // every fragment read of this stage has returned: its weight slot may be overwritten behind this barrier
        if (t == 0 && s < 14) DT_STAMP(0, 4 * s + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t == 0 && s < 14) DT_STAMP(0, 4 * s + 2);
        asm volatile("s_barrier" ::: "memory");
        if (t == 0 && s < 14) DT_STAMP(0, 4 * s + 3);
        read_w(wbn, 0, wf[0]);  // (behind the last stage: a read of valid LDS nobody uses -- unconditional, so that no branch join
        read_x(s == DC3_SPT - 1 ? 0 : s + 1, 0, xf[0]);  //  makes the compiler wait for these before the MFMAs below)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int p = 0; p < 4; p++) acc[a][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][a], xf[1][p], acc[a][p], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      {
        // ---- epilogue straight from the accumulators: lane = (pixel column pxl, couts 64 ch + 16 ct + 4 kg .. + 3) of rows 4 pq + pt
        int b, y0, x0;
        DT_STAMP(0, 112 + 2 * t);
        tile_origin(t, b, y0, x0);
        const int xx = x0 + pxl;
        f32x2 u1[8], u2[8];  // this tile, this lane's pixels: [2 cout tile + r / 2][r & 1]
#pragma unroll
        for (int e = 0; e < 8; e++) u1[e] = u2[e] = f32x2{0.f, 0.f};
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const int yy = y0 + pq * 4 + p;
          const bool valid = yy < H && xx < W;
          // 16-byte stores (the tail is bound by the NUMBER of store instructions -- ~75 clocks each per CU whatever their width:
          // 16 x 8 B per lane took 9.6 k clocks per tile, into an L2-resident target just the same): v_permlane16_swap trades cout
          // tile a of the odd-kg lanes against tile a + 2 of the even-kg lanes, after which an even lane holds couts
          // 16 a + 4 kg .. + 7 and an odd lane couts 16 (a + 2) + 4 (kg - 1) .. + 7 of its pixel
          dt_bf16* dst = y + (((size_t)b * H + yy) * W + xx) * DT_C + ch * 64 + ((kg & 1) ? 32 + (kg - 1) * 4 : kg * 4);
          unsigned lo[4], hi[4];
#pragma unroll
          for (int a = 0; a < 4; a++) {
            lo[a] = valid ? bf16_pack2(acc[a][p][0], acc[a][p][1]) : 0u;
            hi[a] = valid ? bf16_pack2(acc[a][p][2], acc[a][p][3]) : 0u;
            // statistics of the ROUNDED values: what the next kernel reads
            const f32x2 va = {__uint_as_float(lo[a] << 16), __uint_as_float(lo[a] & 0xFFFF0000u)};
            const f32x2 vb = {__uint_as_float(hi[a] << 16), __uint_as_float(hi[a] & 0xFFFF0000u)};
            u1[a * 2] += va; u2[a * 2] = __builtin_elementwise_fma(va, va, u2[a * 2]);          // (packed fp32 instructions)
            u1[a * 2 + 1] += vb; u2[a * 2 + 1] = __builtin_elementwise_fma(vb, vb, u2[a * 2 + 1]);
          }
#pragma unroll
          for (int a = 0; a < 2; a++) {
            const auto s0 = __builtin_amdgcn_permlane16_swap(lo[a], lo[a + 2], false, false);
            const auto s1 = __builtin_amdgcn_permlane16_swap(hi[a], hi[a + 2], false, false);
            if (valid) *reinterpret_cast<u32x4*>(dst + a * 16) = u32x4{s0[0], s1[0], s0[1], s1[1]};
          }
        }
        if (stats) {
          float f1[16], f2[16];
#pragma unroll
          for (int e = 0; e < 8; e++) {
            f1[2 * e] = u1[e][0]; f1[2 * e + 1] = u1[e][1];
            f2[2 * e] = u2[e][0]; f2[2 * e + 1] = u2[e][1];
          }
          st1 += dt_rs16(f1, pxl);
          st2 += dt_rs16(f2, pxl);
        }
        DT_STAMP(0, 113 + 2 * t);
      }
    }
    // ---- the workgroup's statistics: the four row groups of a channel, in order
    float* const red = reinterpret_cast<float*>(abuf);  // (every request has landed and every fragment read has returned)
    if (stats) {
      const int c = ch * 64 + (pxl >> 2) * 16 + kg * 4 + (pxl & 3);
      red[(pq * 2 + 0) * DT_C + c] = st1;
      red[(pq * 2 + 1) * DT_C + c] = st2;
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (stats && tid < 2 * DT_C) {
      const int which = tid / DT_C, c = tid % DT_C;
      float a = 0.f;
#pragma unroll
      for (int g = 0; g < 4; g++) a += red[(g * 2 + which) * DT_C + c];
      stats[((size_t)blockIdx.x * 2 + which) * DT_C + c] = a;
    }
    asm volatile("s_barrier" ::: "memory");
  }
}

// rows of the `stats` output of v3d_dense_train_conv = workgroups of its persistent grid
extern "C" int v3d_dense_train_conv_tiles(int B, int H, int W) {
  const long long t1 = ((long long)B * H * W + DT_BM - 1) / DT_BM;                                          // 1x1: runs of 128 pixels
  const long long t3 = (long long)B * ((H + DC3_T - 1) / DC3_T) * ((W + DC3_T - 1) / DC3_T);                    // 3x3: 16 x 16 blocks
  const long long tiles = t1 < t3 ? t1 : t3;  // both kernels get a workgroup per row of `stats`, none without a tile
  return (int)(tiles < DT_CONV_GRID ? tiles : DT_CONV_GRID);
}

// x, y: bf16 NHWC (B, H, W, 128).  image: v3d_dense_train_pack_weights.  stats (nullable): (v3d_dense_train_conv_tiles, 2, 128) fp32.
extern "C" int v3d_dense_train_conv(const void* x, const void* image, int B, int H, int W, int ksize, void* y, float* stats,
                                    v3d_stream_t stream) {
  if (!x || !image || !y || B < 1 || H < 1 || W < 1 || H >= 32768 || W >= 65536 || (ksize != 1 && ksize != 3)) return V3D_EINVAL;
  if ((long long)B * H * W > 0x7FFFFFF0ll) return V3D_EINVAL;
  const int grid = v3d_dense_train_conv_tiles(B, H, W);
  hipStream_t st = (hipStream_t)stream;
  if (ksize == 3) {
    static V3dPerDeviceFlag attr3;
    V3D_CHECK_HIP(v3d_set_max_lds(attr3, (const void*)dt_conv3_kernel, DC3_SMEM));
    hipLaunchKernelGGL(dt_conv3_kernel, dim3(grid), dim3(DC3_THREADS), DC3_SMEM, st, (const dt_bf16*)x, (const dt_bf16*)image, B, H, W,
                       (dt_bf16*)y, stats);
  } else {
    static V3dPerDeviceFlag attr1;
    V3D_CHECK_HIP(v3d_set_max_lds(attr1, (const void*)dt_conv_kernel<1>, DT_CONV_SMEM));
    hipLaunchKernelGGL(dt_conv_kernel<1>, dim3(grid), dim3(DT_THREADS), DT_CONV_SMEM, st, (const dt_bf16*)x, (const dt_bf16*)image, B, H, W,
                       (dt_bf16*)y, stats);
  }
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// ------------------------------------------------------------------------------------------------ BatchNorm (batch statistics)
// Column sums of a (rows, cols) fp32 matrix of partials, in double, in a FIXED order: a workgroup of 1024 threads owns 32 columns,
// thread (column j = tid & 31, part = tid >> 5) adds rows part, part + 32, ...; the 32 parts are then added in part order.
// Returns the sum of column `col0 + j` to the threads with part == 0 (others: 0); `red` = 32 x 32 doubles of LDS.
// (These kernels are latency chains, not streams: with 8 parts a thread walked 128 rows one dependent load after the other -- 38 us.)
#define DT_COLSUM_THREADS 1024
__device__ __forceinline__ double dt_colsum32(const float* __restrict__ partial, int rows, int cols, int col0, double (*red)[32]) {
  const int j = threadIdx.x & 31, part = threadIdx.x >> 5;
  double a = 0.0;
  if (col0 + j < cols)
    for (int r = part; r < rows; r += 32) a += (double)partial[(size_t)r * cols + col0 + j];
  red[part][j] = a;
  __syncthreads();
  double t = 0.0;
  if (part == 0)
    for (int q = 0; q < 32; q++) t += red[q][j];
  return t;
}

// partial (tiles, 2, 128) -> mean, invstd (biased variance, as torch normalises), running statistics with the unbiased variance
// (momentum update, num_batches_tracked += 1).  8 workgroups x 16 channels: columns {c, 128 + c} of the same channels share a block.
__global__ __launch_bounds__(DT_COLSUM_THREADS) void dt_bn_finalize_kernel(const float* __restrict__ partial, int tiles, long long count, float eps,
                                                             float momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                             float* __restrict__ running_mean, float* __restrict__ running_var,
                                                             long long* __restrict__ nbt) {
  __shared__ double red[32][32];
  __shared__ double tot[32];
  const int j = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int which = j >> 4, c = blockIdx.x * 16 + (j & 15);
  // (a 32-column window of the (tiles, 256) matrix is not contiguous here: gather the two 16-column halves by hand)
  double a = 0.0;
  for (int r = part; r < tiles; r += 32) a += (double)partial[((size_t)r * 2 + which) * DT_C + c];
  red[part][j] = a;
  __syncthreads();
  if (part == 0) {
    double t = 0.0;
    for (int q = 0; q < 32; q++) t += red[q][j];
    tot[j] = t;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int cc = blockIdx.x * 16 + threadIdx.x;
    const double mu = tot[threadIdx.x] / (double)count;
    double var = tot[16 + threadIdx.x] / (double)count - mu * mu;
    var = var > 0.0 ? var : 0.0;
    mean[cc] = (float)mu;
    invstd[cc] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
      const double unb = count > 1 ? var * (double)count / (double)(count - 1) : var;
      running_mean[cc] = (float)((1.0 - momentum) * (double)running_mean[cc] + momentum * mu);
      running_var[cc] = (float)((1.0 - momentum) * (double)running_var[cc] + momentum * unb);
      if (cc == 0 && nbt) *nbt += 1;
    }
  }
}

extern "C" int v3d_dense_train_bn_finalize(const float* partial, int tiles, long long count, float eps, float momentum, float* mean,
                                           float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                           v3d_stream_t stream) {
  if (!partial || tiles < 1 || count < 1 || !mean || !invstd || ((running_mean == nullptr) != (running_var == nullptr))) return V3D_EINVAL;
  hipLaunchKernelGGL(dt_bn_finalize_kernel, dim3(DT_C / 16), dim3(DT_COLSUM_THREADS), 0, (hipStream_t)stream, partial, tiles, count, eps, momentum, mean,
                     invstd, running_mean, running_var, (long long*)num_batches_tracked);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// The folded affine of a channel: y = relu(fmaf(x, sc, sh)).  The forward stores THIS expression, and both backward kernels decide
// the ReLU mask with it (not with fmaf(x_hat, gamma, beta), which rounds differently where y is within an ulp of 0: the gradient
// would pass where the stored output is 0, or stop where it is positive -- tests/test_gpu_bn_edges.py, the tie kind).
__device__ __forceinline__ void dt_bn_fold(float mean, float invstd, float gamma, float beta, float& sc, float& sh) {
  sc = invstd * gamma;
  sh = beta - mean * sc;
}

// y = relu((x - mean) * invstd * gamma + beta), bf16 NHWC -> bf16 NHWC.  thread = 8 channels of one pixel (16-byte load / store).
__global__ __launch_bounds__(256) void dt_bn_relu_apply_kernel(const dt_bf16* __restrict__ x, const dt_bf16* __restrict__ x_lo, long long M,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                               dt_bf16* __restrict__ y, dt_bf16* __restrict__ y_lo) {
  const int c8 = threadIdx.x & 15;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int c = c8 * 8 + e;
    dt_bn_fold(mean[c], invstd[c], gamma[c], beta[c], sc[e], sh[e]);
  }
  for (long long m = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); m < M; m += (long long)gridDim.x * 16) {
    float v[8];
    dt_load8(x, x_lo, m * DT_C + c8 * 8, v);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      v[e] = fmaf(v[e], sc[e], sh[e]);
      if (relu) v[e] = fmaxf(v[e], 0.f);
    }
    dt_store8(y, y_lo, m * DT_C + c8 * 8, v);
  }
}

static int dt_bn_relu_apply(DtT x, long long M, const float* mean, const float* invstd, const float* gamma, const float* beta, int relu, DtT y,
                            v3d_stream_t stream) {
  if (!x.hi || !y.hi || M < 1 || !mean || !invstd || !gamma || !beta) return V3D_EINVAL;
  const long long blocks = (M + 15) / 16;
  hipLaunchKernelGGL(dt_bn_relu_apply_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     (const dt_bf16*)x.hi, (const dt_bf16*)x.lo, M, mean, invstd, gamma, beta, relu, (dt_bf16*)y.hi, (dt_bf16*)y.lo);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_dense_train_bn_relu_apply(const void* x, long long M, const float* mean, const float* invstd, const float* gamma,
                                             const float* beta, int relu, void* y, v3d_stream_t stream) {
  return dt_bn_relu_apply(dt_t(x), M, mean, invstd, gamma, beta, relu, dt_t(y), stream);
}

// Backward of y = relu(x_hat * gamma + beta), x_hat = (x - mean) * invstd, batch statistics:
//   g = dy * [y > 0];  dbeta = sum g;  dgamma = sum g * x_hat;  dx = gamma * invstd * (g - dbeta / M - x_hat * dgamma / M).
// Pass 1 (this kernel): per-block partial (sum g, sum g * x_hat) per channel, blocks in a fixed grid, thread = 8 channels of a pixel,
// the 16 pixel rows of a block reduced through LDS in row order.
#define DT_RED_BLOCKS 512
// tail of a 256-thread block whose thread (c8, rg) holds two sums for channels 8 c8 .. 8 c8 + 7 over the pixel rows of row group rg:
// the 16 row groups are added through LDS in row-group order -> partial[block][2][128]
__device__ __forceinline__ void dt_rowgroup_sums(const float (&s1)[8], const float (&s2)[8], float* __restrict__ partial) {
  __shared__ float red[16][2][DT_C];
  const int c8 = threadIdx.x & 15, rg = threadIdx.x >> 4;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    red[rg][0][c8 * 8 + e] = s1[e];
    red[rg][1][c8 * 8 + e] = s2[e];
  }
  __syncthreads();
  const int which = threadIdx.x / DT_C, c = threadIdx.x % DT_C;
  float a = 0.f;
  for (int g = 0; g < 16; g++) a += red[g][which][c];
  partial[((size_t)blockIdx.x * 2 + which) * DT_C + c] = a;
}

__global__ __launch_bounds__(256) void dt_bn_bwd_reduce_kernel(const dt_bf16* __restrict__ x, const dt_bf16* __restrict__ x_lo,
                                                               const dt_bf16* __restrict__ dy, const dt_bf16* __restrict__ dy_lo, long long M,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               int relu, float* __restrict__ partial /*[blocks][2][128]*/) {
  const int c8 = threadIdx.x & 15, rg = threadIdx.x >> 4;
  float mu[8], is[8], sc[8], sh[8], s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int c = c8 * 8 + e;
    mu[e] = mean[c]; is[e] = invstd[c];
    dt_bn_fold(mu[e], is[e], gamma[c], beta[c], sc[e], sh[e]);
    s1[e] = s2[e] = 0.f;
  }
  for (long long m = (long long)blockIdx.x * 16 + rg; m < M; m += (long long)gridDim.x * 16) {
    float xv[8], gv[8];
    dt_load8(x, x_lo, m * DT_C + c8 * 8, xv);
    dt_load8(dy, dy_lo, m * DT_C + c8 * 8, gv);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const float xh = (xv[e] - mu[e]) * is[e];
      const float g = (!relu || fmaf(xv[e], sc[e], sh[e]) > 0.f) ? gv[e] : 0.f;  // the forward's y > 0
      s1[e] += g;
      s2[e] = fmaf(g, xh, s2[e]);
    }
  }
  dt_rowgroup_sums(s1, s2, partial);
}

// blocks partials (blocks, 2, 128) -> dbeta, dgamma: 8 workgroups x 32 columns of the (blocks, 256) matrix
__global__ __launch_bounds__(DT_COLSUM_THREADS) void dt_bn_bwd_finalize_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ dbeta,
                                                                 float* __restrict__ dgamma) {
  __shared__ double red[32][32];
  const double t = dt_colsum32(partial, blocks, 2 * DT_C, blockIdx.x * 32, red);
  if ((threadIdx.x >> 5) == 0) {
    const int col = blockIdx.x * 32 + (threadIdx.x & 31);
    (col >= DT_C ? dgamma : dbeta)[col & (DT_C - 1)] = (float)t;
  }
}

__global__ __launch_bounds__(256) void dt_bn_bwd_apply_kernel(const dt_bf16* __restrict__ x, const dt_bf16* __restrict__ x_lo,
                                                              const dt_bf16* dy, const dt_bf16* dy_lo, long long M,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ dbeta, const float* __restrict__ dgamma, int relu,
                                                              dt_bf16* dx, dt_bf16* dx_lo) {
  const int c8 = threadIdx.x & 15;
  float mu[8], is[8], ga[8], sc[8], sh[8], k0[8], k1[8];
  const float inv_m = 1.f / (float)M;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int c = c8 * 8 + e;
    mu[e] = mean[c]; is[e] = invstd[c]; ga[e] = gamma[c];
    dt_bn_fold(mu[e], is[e], ga[e], beta[c], sc[e], sh[e]);
    k0[e] = dbeta[c] * inv_m;
    k1[e] = dgamma[c] * inv_m;
  }
  for (long long m = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); m < M; m += (long long)gridDim.x * 16) {
    float xv[8], gv[8], o[8];
    dt_load8(x, x_lo, m * DT_C + c8 * 8, xv);
    dt_load8(dy, dy_lo, m * DT_C + c8 * 8, gv);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const float xh = (xv[e] - mu[e]) * is[e];
      const float g = (!relu || fmaf(xv[e], sc[e], sh[e]) > 0.f) ? gv[e] : 0.f;  // the forward's y > 0
      o[e] = ga[e] * is[e] * (g - k0[e] - xh * k1[e]);
    }
    dt_store8(dx, dx_lo, m * DT_C + c8 * 8, o);
  }
}

extern "C" size_t v3d_dense_train_bn_bwd_workspace(void) { return (size_t)DT_RED_BLOCKS * 2 * DT_C * sizeof(float); }

// x: the layer's raw convolution output (bf16 NHWC), dy: gradient w.r.t. the post-ReLU output -> dx (gradient w.r.t. x, bf16 NHWC;
// may alias dy), dgamma, dbeta (fp32).  The ReLU mask is the forward's: fmaf(x, sc, sh) > 0 with dt_bn_fold's sc / sh, the value
// v3d_dense_train_bn_relu_apply rounded and stored -- so it equals (y > 0) of that output on every element.
// (x_lo / dy_lo / dx_lo: the lo planes of split storage, all three or none)
static int dt_bn_relu_bwd(const void* x, const void* x_lo, const void* dy, const void* dy_lo, long long M, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, int relu, void* dx, void* dx_lo, float* dgamma,
                          float* dbeta, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (!x || !dy || !dx || M < 1 || !mean || !invstd || !gamma || !beta || !dgamma || !dbeta || !workspace) return V3D_EINVAL;
  if (workspace_bytes < v3d_dense_train_bn_bwd_workspace()) return V3D_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long long want = (M + 15) / 16;
  const int blocks = (int)(want < DT_RED_BLOCKS ? want : DT_RED_BLOCKS);
  float* partial = (float*)workspace;
  hipLaunchKernelGGL(dt_bn_bwd_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const dt_bf16*)x, (const dt_bf16*)x_lo, (const dt_bf16*)dy,
                     (const dt_bf16*)dy_lo, M, mean, invstd, gamma, beta, relu, partial);
  hipLaunchKernelGGL(dt_bn_bwd_finalize_kernel, dim3(2 * DT_C / 32), dim3(DT_COLSUM_THREADS), 0, st, partial, blocks, dbeta, dgamma);
  hipLaunchKernelGGL(dt_bn_bwd_apply_kernel, dim3(blocks > 4096 ? 4096 : blocks), dim3(256), 0, st, (const dt_bf16*)x, (const dt_bf16*)x_lo,
                     (const dt_bf16*)dy, (const dt_bf16*)dy_lo, M, mean, invstd, gamma, beta, dbeta, dgamma, relu, (dt_bf16*)dx, (dt_bf16*)dx_lo);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_dense_train_bn_relu_bwd(const void* x, const void* dy, long long M, const float* mean, const float* invstd,
                                           const float* gamma, const float* beta, int relu, void* dx, float* dgamma, float* dbeta,
                                           void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  return dt_bn_relu_bwd(x, nullptr, dy, nullptr, M, mean, invstd, gamma, beta, relu, dx, nullptr, dgamma, dbeta, workspace, workspace_bytes,
                        stream);
}

// Batch statistics of a split tensor: per-block partial (sum x, sum x^2) per channel in the layout dt_bn_finalize_kernel reduces
// (the bf16-storage path gets them from the convolution's epilogue; the split path's convolutions are csrc/dense_conv.hip's).
__global__ __launch_bounds__(256) void dt_bn_stats_kernel(const dt_bf16* __restrict__ x, const dt_bf16* __restrict__ x_lo, long long M,
                                                          float* __restrict__ partial /*[blocks][2][128]*/) {
  const int c8 = threadIdx.x & 15, rg = threadIdx.x >> 4;
  float s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; e++) s1[e] = s2[e] = 0.f;
  for (long long m = (long long)blockIdx.x * 16 + rg; m < M; m += (long long)gridDim.x * 16) {
    float xv[8];
    dt_load8(x, x_lo, m * DT_C + c8 * 8, xv);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      s1[e] += xv[e];
      s2[e] = fmaf(xv[e], xv[e], s2[e]);
    }
  }
  dt_rowgroup_sums(s1, s2, partial);
}

#define DT_WG_SLABS 64
// ------------------------------------------------------------------------------------------------ weight gradient
// dW[tap][ci][co] = sum_pixels X[p + tap][ci] * dY[p][co] straight from the NHWC tensors.  (The first version re-laid both
// operands out as zero-bordered channel planes with three shifted copies of X: 0.8 ms of layout kernels per step and ~1 GB of
// operand traffic per layer at bs = 8; 210 + 123 us per layer against 80 here.)  The reduction index (pixels) must be the
// contiguous one of both MFMA operands, which NHWC rows are not: the fragments are read from LDS with ds_read_b64_tr_b16, the
// gfx950 transpose read -- within a 16-lane group, lane s supplies the address of 4 consecutive channels of pixel s >> 2
// (chunk s & 3) and lane i receives channel i of those 4 pixels (probed: tools/mb_tr16.hip).
// Work split: workgroup = (block of 32 input channels, slab of 8 x 16 pixel tiles).  Per tile the loaders bring the tile's
// (8 + 2) x (16 + 2) neighbourhood of X -- only this block's 32 channels: 64 B per pixel -- and the 8 x 16 block of dY (all 128
// channels) into LDS, double buffered, ONE barrier per tile; the 8 multiplying waves (wave = input-channel tile x pair of cout
// tiles, TAPS x 2 accumulators) walk the tile in four 32-pixel steps: 2 + 2 transpose reads for dY, 2 per tap for X (a tap is a
// pixel-row offset into the same LDS image), TAPS x 2 MFMAs.  LDS images are chunk-swizzled so that the 8 pixels x 4 chunks a
// half-wave reads together fall on distinct banks.  Accumulators stay in registers over the whole slab; slabs are summed by
// dt_wgrad_reduce_kernel in slab order.
#define DT_W2_XBUF (192 * 64)        // neighbourhood image: 180 pixel rows x 64 B (12 requests of 16 rows)
#define DT_W2_YBUF (128 * 256)
#define DT_W2_BUF (DT_W2_XBUF + DT_W2_YBUF)   // 45 056 B per tile
#define DT_W2_SMEM (2 * DT_W2_BUF)
template <int TAPS>
__global__ __launch_bounds__(768) void dt_wgrad_kernel(const dt_bf16* __restrict__ x, const dt_bf16* __restrict__ dy, int B, int H, int W,
                                                        int slabs, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dt_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cib = blockIdx.x / slabs, slab = blockIdx.x - cib * slabs;  // the 4 channel blocks of a slab are `slabs` apart: same XCD
  const int tx_n = (W + DT3_TW - 1) / DT3_TW, ty_n = (H + DT3_TH - 1) / DT3_TH;
  const int ntiles = B * ty_n * tx_n;
  const int my_tiles = slab < ntiles ? (ntiles - 1 - slab) / slabs + 1 : 0;
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  if (wave >= 8) {
    // ------------------------------------------------------------------ loaders
    const int lw = wave - 8;
    auto issue = [&](int i) {
      const int tile = __builtin_amdgcn_readfirstlane(slab + i * slabs);
      const int b = tile / (ty_n * tx_n), r = tile - b * ty_n * tx_n;
      const int y0 = (r / tx_n) * DT3_TH, x0 = (r % tx_n) * DT3_TW;
      unsigned char* buf = dt_smem + (i & 1) * DT_W2_BUF;
      // X neighbourhood: request q covers 16 pixel rows x 64 B (4 lanes per row); rows q = lw, lw + 4, lw + 8
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int q = j * 4 + lw;
        const int hp = q * 16 + (lane >> 2), slot = lane & 3;
        const int hy = hp / (DT3_TW + 2), hx = hp - hy * (DT3_TW + 2);
        const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
        const bool ok = hp < DT3_HALO && yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int part = slot ^ (((hp >> 3) & 1) << 1);
        const dt_bf16* src = ok ? x + (((size_t)b * H + yy) * W + xx) * DT_C + cib * 32 + part * 8 : reinterpret_cast<const dt_bf16*>(dt_zero16);
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(buf + q * 1024), 16, 0, 0);
      }
      // dY block: request q covers 4 pixel rows x 256 B; q = lw, lw + 4, ... (8 per loader)
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int q = j * 4 + lw;
        const int px = q * 4 + (lane >> 4), slot = lane & 15;
        const int yy = y0 + (px >> 4), xx = x0 + (px & 15);
        const bool ok = yy < H && xx < W;
        const int part = slot ^ (((px & 3) << 1) | (((px >> 3) & 1) << 3));
        const dt_bf16* src = ok ? dy + (((size_t)b * H + yy) * W + xx) * DT_C + part * 8 : reinterpret_cast<const dt_bf16*>(dt_zero16);
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(buf + DT_W2_XBUF + q * 1024), 16, 0, 0);
      }
    };
    if (my_tiles > 0) issue(0);
    for (int i = 0; i < my_tiles; i++) {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");  // tile i readable; tile i - 1 finished: its buffer is free
      if (i + 1 < my_tiles) issue(i + 1);
    }
    asm volatile("s_barrier" ::: "memory");
    return;
  }
  // -------------------------------------------------------------------- multipliers
  const int t = wave & 1, cp = wave >> 1;  // input-channel tile (16 of the block's 32), cout tiles 2 cp and 2 cp + 1
  f32x4 acc[TAPS][2];
#pragma unroll
  for (int a = 0; a < TAPS; a++) acc[a][0] = acc[a][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kg = lane >> 4, s16 = lane & 15, c = s16 & 3, e4 = s16 >> 2;
  const unsigned lds0 = lds_addr_dt(dt_smem);
  for (int i = 0; i < my_tiles; i++) {
    asm volatile("s_barrier" ::: "memory");
    const unsigned xb = lds0 + (i & 1) * DT_W2_BUF, yb = xb + DT_W2_XBUF;
#pragma unroll 1
    for (int st = 0; st < 4; st++) {  // 32 pixels = block rows 2 st, 2 st + 1; k = kg * 8 + e: row 2 st + (kg >> 1), column (kg & 1) * 8 + e
      const int row = 2 * st + (kg >> 1), col0 = (kg & 1) * 8 + e4;  // (+ 4 for the second read of a fragment)
      unsigned long long fb[2][2];
#pragma unroll
      for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r2 = 0; r2 < 2; r2++) {
          const int px = row * 16 + col0 + r2 * 4;
          const int part = (2 * (2 * cp + n) + (c >> 1)) ^ (((px & 3) << 1) | (((px >> 3) & 1) << 3));
          asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fb[n][r2]) : "v"(yb + px * 256 + (part << 4) + (c & 1) * 8) : "memory");
        }
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      constexpr int TG = TAPS == 9 ? 3 : 1;  // taps per batch of transpose reads (a batch = one kernel row)
      bf16x8 bfrag[2];
#pragma unroll
      for (int a0 = 0; a0 < TAPS; a0 += TG) {
        unsigned long long fa[TG][2];
#pragma unroll
        for (int a = 0; a < TG; a++) {
          const int dyy = TAPS == 9 ? (a0 + a) / 3 - 1 : 0, dxx = TAPS == 9 ? (a0 + a) % 3 - 1 : 0;
#pragma unroll
          for (int r2 = 0; r2 < 2; r2++) {
            const int hp = (row + 1 + dyy) * (DT3_TW + 2) + col0 + r2 * 4 + 1 + dxx;
            const int part = (2 * t + (c >> 1)) ^ (((hp >> 3) & 1) << 1);
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fa[a][r2]) : "v"(xb + hp * 64 + (part << 4) + (c & 1) * 8) : "memory");
          }
        }
        // the batch has landed (the reads are invisible to the compiler: tie their registers to the wait)
        if (a0 == 0) {
          if constexpr (TG == 3)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[0][0]), "+v"(fb[0][1]), "+v"(fb[1][0]), "+v"(fb[1][1]), "+v"(fa[0][0]), "+v"(fa[0][1]),
                         "+v"(fa[1][0]), "+v"(fa[1][1]), "+v"(fa[2][0]), "+v"(fa[2][1]) :: "memory");
          else
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[0][0]), "+v"(fb[0][1]), "+v"(fb[1][0]), "+v"(fb[1][1]), "+v"(fa[0][0]), "+v"(fa[0][1]) :: "memory");
#pragma unroll
          for (int n = 0; n < 2; n++) bfrag[n] = __builtin_bit_cast(bf16x8, u64x2{fb[n][0], fb[n][1]});
        } else {
          if constexpr (TG == 3)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[1][0]), "+v"(fa[1][1]), "+v"(fa[2][0]), "+v"(fa[2][1]) :: "memory");
        }
#pragma unroll
        for (int a = 0; a < TG; a++) {
          const bf16x8 af = __builtin_bit_cast(bf16x8, u64x2{fa[a][0], fa[a][1]});
#pragma unroll
          for (int n = 0; n < 2; n++) acc[a0 + a][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfrag[n], acc[a0 + a][n], 0, 0, 0);
        }
      }
    }
  }
  asm volatile("s_barrier" ::: "memory");
  // D[row = ci within the tile = (lane >> 4) * 4 + r][col = cout within the tile = lane & 15]
#pragma unroll
  for (int a = 0; a < TAPS; a++)
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int ci = cib * 32 + t * 16 + kg * 4 + r, co = (2 * cp + n) * 16 + s16;
        partial[(((size_t)slab * TAPS + a) * DT_C + ci) * DT_C + co] = acc[a][n][r];
      }
}

// partial (slabs, taps, ci, co) -> dW (co, ci, taps) fp32.  One workgroup per (input channel, group of <= 3 taps): thread (co, g) sums
// its slabs in slab order (coalesced 512-byte rows), the eight group sums are combined in a fixed tree.  Bit-repeatable.
// Which slabs are group g's is the only difference between the two arithmetics, and it decides the result's bits:
//   INTERLEAVED = false  8 g .. 8 g + 7       (bf16 storage: at most DT_WG_SLABS = 64 partials)
//   INTERLEAVED = true   g, g + 8, g + 16 ... (split storage: the partials of three terms, any number)
template <bool INTERLEAVED>
__global__ __launch_bounds__(1024) void dt_wgrad_reduce_kernel(const float* __restrict__ partial, int slabs, int taps, float* __restrict__ dw) {
  __shared__ float grp[8][3][DT_C];
  const int ci = blockIdx.x, a0 = blockIdx.y * 3, na = taps - a0 < 3 ? taps - a0 : 3;
  const int co = threadIdx.x & (DT_C - 1), g = threadIdx.x >> 7;
  const size_t total = (size_t)taps * DT_C * DT_C;
  for (int a = 0; a < na; a++) {
    const size_t at = ((size_t)(a0 + a) * DT_C + ci) * DT_C + co;
    float v = 0.f;
    if constexpr (INTERLEAVED) {
      for (int s = g; s < slabs; s += 8) v += partial[(size_t)s * total + at];
    } else {
#pragma unroll
      for (int s = 0; s < 8; s++)
        if (8 * g + s < slabs) v += partial[(size_t)(8 * g + s) * total + at];
    }
    grp[g][a][co] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < DT_C * na; idx += 1024) {
    const int c = idx / na, a = idx - c * na;
    const float v = ((grp[0][a][c] + grp[1][a][c]) + (grp[2][a][c] + grp[3][a][c])) + ((grp[4][a][c] + grp[5][a][c]) + (grp[6][a][c] + grp[7][a][c]));
    dw[((size_t)c * DT_C + ci) * taps + a0 + a] = v;
  }
}

extern "C" size_t v3d_dense_train_wgrad_workspace(int ksize) { return (size_t)DT_WG_SLABS * ksize * ksize * DT_C * DT_C * sizeof(float); }

// one product term: the slab partials of x (*) dy
static int dt_wgrad_launch(int ksize, const void* x, const void* dy, int B, int H, int W, int slabs, float* partial, hipStream_t st) {
  static V3dPerDeviceFlag attr9, attr1;
  V3D_CHECK_HIP(v3d_set_max_lds(attr9, (const void*)dt_wgrad_kernel<9>, DT_W2_SMEM));
  V3D_CHECK_HIP(v3d_set_max_lds(attr1, (const void*)dt_wgrad_kernel<1>, DT_W2_SMEM));
  if (ksize == 3)
    hipLaunchKernelGGL(dt_wgrad_kernel<9>, dim3(4 * slabs), dim3(768), DT_W2_SMEM, st, (const dt_bf16*)x, (const dt_bf16*)dy, B, H, W, slabs, partial);
  else
    hipLaunchKernelGGL(dt_wgrad_kernel<1>, dim3(4 * slabs), dim3(768), DT_W2_SMEM, st, (const dt_bf16*)x, (const dt_bf16*)dy, B, H, W, slabs, partial);
  return V3D_OK;
}

// bf16 storage: one term.  Split storage: (x_hi, dy_hi), (x_hi, dy_lo), (x_lo, dy_hi) into three sets of slab partials, summed by one
// fixed-order reduction.  workspace: v3d_dense_train_wgrad_workspace per term.
static int dt_wgrad(DtT x, DtT dy, int B, int H, int W, int ksize, float* dw, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  const bool split = x.lo != nullptr;
  if (workspace_bytes < (split ? 3 : 1) * v3d_dense_train_wgrad_workspace(ksize)) return V3D_EWORKSPACE;
  const long long tiles = (long long)B * ((H + DT3_TH - 1) / DT3_TH) * ((W + DT3_TW - 1) / DT3_TW);
  const int slabs = (int)(tiles < DT_WG_SLABS ? tiles : DT_WG_SLABS), taps = ksize * ksize;
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  const size_t term = (size_t)slabs * taps * DT_C * DT_C;
  const dim3 grid(DT_C, (taps + 2) / 3);
  DT_TRY(dt_wgrad_launch(ksize, x.hi, dy.hi, B, H, W, slabs, partial, st));
  if (split) {
    DT_TRY(dt_wgrad_launch(ksize, x.hi, dy.lo, B, H, W, slabs, partial + term, st));
    DT_TRY(dt_wgrad_launch(ksize, x.lo, dy.hi, B, H, W, slabs, partial + 2 * term, st));
    hipLaunchKernelGGL(dt_wgrad_reduce_kernel<true>, grid, dim3(1024), 0, st, partial, 3 * slabs, taps, dw);
  } else {
    hipLaunchKernelGGL(dt_wgrad_reduce_kernel<false>, grid, dim3(1024), 0, st, partial, slabs, taps, dw);
  }
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// x: bf16 NHWC input of the layer, dy: bf16 NHWC gradient of its raw output -> dw (128, 128, k, k) fp32.  No planar operands.
extern "C" int v3d_dense_train_wgrad(const void* x, const void* dy, int B, int H, int W, int ksize, float* dw, void* workspace,
                                          size_t workspace_bytes, v3d_stream_t stream) {
  if (!x || !dy || !dw || !workspace || B < 1 || H < 1 || W < 1 || (ksize != 1 && ksize != 3)) return V3D_EINVAL;
  return dt_wgrad(dt_t(x), dt_t(dy), B, H, W, ksize, dw, workspace, workspace_bytes, stream);
}

// the same on split planes (value = hi + lo): dw = x_hi (*) dy_hi + x_hi (*) dy_lo + x_lo (*) dy_hi, the weight gradient of the split step
// on its own.  workspace: THREE v3d_dense_train_wgrad_workspace (one set of slab partials per term).
extern "C" int v3d_dense_train_wgrad_split(const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, int B, int H, int W,
                                           int ksize, float* dw, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (!x_hi || !x_lo || !dy_hi || !dy_lo || !dw || !workspace || B < 1 || H < 1 || W < 1 || (ksize != 1 && ksize != 3)) return V3D_EINVAL;
  return dt_wgrad(dt_t(x_hi, x_lo), dt_t(dy_hi, dy_lo), B, H, W, ksize, dw, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ 1x1 head (<= 64 outputs, bias)
// maps[b][o][pix] = sum_c feat[m][c] * W[o][c] + bias[o]   (fp32 NCHW out: what ProposalLayer.reshape_* and the loss take)
#define DT_HEAD_MAX 64
template <int O>  // compile-time: the per-pixel output vector stays in registers
__global__ __launch_bounds__(256) void dt_head_fwd_kernel(const dt_bf16* __restrict__ feat, long long M, int HW, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ maps) {
  __shared__ float ws[O * DT_C];
  __shared__ float bs[O];
  for (int i = threadIdx.x; i < O * DT_C; i += 256) ws[i] = w[i];
  for (int i = threadIdx.x; i < O; i += 256) bs[i] = bias ? bias[i] : 0.f;
  __syncthreads();
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
    float a[O];
#pragma unroll
    for (int o = 0; o < O; o++) a[o] = bs[o];
#pragma unroll 1
    for (int p = 0; p < 16; p++) {
      float v[8];
      bf16_unpack8(*reinterpret_cast<const u32x4*>(feat + m * DT_C + p * 8), v);
#pragma unroll
      for (int o = 0; o < O; o++)
#pragma unroll
        for (int e = 0; e < 8; e++) a[o] = fmaf(v[e], ws[o * DT_C + p * 8 + e], a[o]);
    }
    const long long b = m / HW, pix = m - b * HW;
#pragma unroll
    for (int o = 0; o < O; o++) maps[(b * O + o) * HW + pix] = a[o];
  }
}

// dFeat[m][c] = sum_o dP[b][o][pix] * W[o][c]  (bf16 NHWC out)
template <int O>  // compile-time: the per-pixel gradient vector stays in registers
__global__ __launch_bounds__(256) void dt_head_bwd_data_kernel(const float* __restrict__ dmaps, long long M, int HW, const float* __restrict__ w,
                                                               dt_bf16* __restrict__ dfeat, dt_bf16* __restrict__ dfeat_lo) {
  __shared__ float ws[O * DT_C];
  for (int i = threadIdx.x; i < O * DT_C; i += 256) ws[i] = w[i];
  __syncthreads();
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
    const long long b = m / HW, pix = m - b * HW;
    float g[O];
#pragma unroll
    for (int o = 0; o < O; o++) g[o] = dmaps[(b * O + o) * HW + pix];
#pragma unroll 1
    for (int p = 0; p < 16; p++) {
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < O; o++)
#pragma unroll
        for (int e = 0; e < 8; e++) a[e] = fmaf(g[o], ws[o * DT_C + p * 8 + e], a[e]);
      dt_store8(dfeat, dfeat_lo, m * DT_C + p * 8, a);
    }
  }
}

// partial dW[o][c] and db[o] per block of DT_HEAD_PX pixels: thread = channel c (two halves of the outputs), dP staged in LDS
#define DT_HEAD_PX 512
#define DT_HEAD_BLOCKS 1024
template <int O>  // even
__global__ __launch_bounds__(256) void dt_head_bwd_weight_kernel(const dt_bf16* __restrict__ feat, const dt_bf16* __restrict__ feat_lo,
                                                                 const float* __restrict__ dmaps, long long M, int HW,
                                                                 float* __restrict__ partial /*[blocks][O + 1][128]*/) {
  __shared__ float gs[64][O + 1];
  const int c = threadIdx.x & 127, oh = threadIdx.x >> 7;
  const int o_lo = oh * (O / 2);
  float acc[O / 2];
#pragma unroll
  for (int i = 0; i < O / 2; i++) acc[i] = 0.f;
  float db = 0.f;  // thread (c = o, oh = 0) also carries db[o]
  for (long long m0 = (long long)blockIdx.x * 64; m0 < M; m0 += (long long)gridDim.x * 64) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * O; idx += 256) {
      const int px = idx & 63, o = idx >> 6;
      const long long m = m0 + px;
      float v = 0.f;
      if (m < M) {
        const long long b = m / HW, pix = m - b * HW;
        v = dmaps[(b * O + o) * HW + pix];
      }
      gs[px][o] = v;
    }
    __syncthreads();
    const int npx = (int)min((long long)64, M - m0);
    for (int px = 0; px < npx; px++) {
      const float fv = bf16_to_f32(feat[(m0 + px) * DT_C + c]) + (feat_lo ? bf16_to_f32(feat_lo[(m0 + px) * DT_C + c]) : 0.f);
#pragma unroll
      for (int i = 0; i < O / 2; i++) acc[i] = fmaf(gs[px][o_lo + i], fv, acc[i]);
      if (oh == 0 && c < O) db += gs[px][c];
    }
  }
  float* outp = partial + (size_t)blockIdx.x * (O + 1) * DT_C;
#pragma unroll
  for (int i = 0; i < O / 2; i++) outp[(o_lo + i) * DT_C + c] = acc[i];
  if (oh == 0) outp[O * DT_C + c] = c < O ? db : 0.f;
}

__global__ __launch_bounds__(DT_COLSUM_THREADS) void dt_head_bwd_reduce_kernel(const float* __restrict__ partial, int blocks, int O,
                                                                               float* __restrict__ dw, float* __restrict__ db) {
  __shared__ double red[32][32];
  const int total = (O + 1) * DT_C;
  const double t = dt_colsum32(partial, blocks, total, blockIdx.x * 32, red);
  if ((threadIdx.x >> 5) == 0) {
    const int idx = blockIdx.x * 32 + (threadIdx.x & 31);
    if (idx < O * DT_C) dw[idx] = (float)t;
    else if (idx - O * DT_C < O) db[idx - O * DT_C] = (float)t;
  }
}

extern "C" size_t v3d_dense_train_head_workspace(int O) { return (size_t)DT_HEAD_BLOCKS * (O + 1) * DT_C * sizeof(float); }

extern "C" int v3d_dense_train_head_fwd(const void* feat, int B, int H, int W, const float* weight, const float* bias, int O, float* maps,
                                        v3d_stream_t stream) {
  if (!feat || !weight || !maps || B < 1 || H < 1 || W < 1 || O < 1 || O > DT_HEAD_MAX) return V3D_EINVAL;
  const long long M = (long long)B * H * W;
  const long long blocks = (M + 255) / 256;
  const unsigned gb = (unsigned)(blocks < 2048 ? blocks : 2048);
#define DT_HEAD_CASE(OV)                                                                                                                   \
  if (O == OV)                                                                                                                             \
    hipLaunchKernelGGL(dt_head_fwd_kernel<OV>, dim3(gb), dim3(256), 0, (hipStream_t)stream, (const dt_bf16*)feat, M, H * W, weight, bias, maps); \
  else
  DT_HEAD_CASE(8) DT_HEAD_CASE(16) DT_HEAD_CASE(24) DT_HEAD_CASE(32) DT_HEAD_CASE(48) DT_HEAD_CASE(64) return V3D_EUNSUPPORTED;
#undef DT_HEAD_CASE
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

// dmaps fp32 (B, O, H, W) -> dfeat bf16 NHWC, dweight (O, 128), dbias (O)
static int dt_head_bwd(const void* feat, const void* feat_lo, const float* dmaps, int B, int H, int W, const float* weight, int O, void* dfeat,
                       void* dfeat_lo, float* dweight, float* dbias, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  if (!feat || !dmaps || !weight || !dfeat || !dweight || !dbias || !workspace || B < 1 || H < 1 || W < 1 || O < 1 || O > DT_HEAD_MAX)
    return V3D_EINVAL;
  if (workspace_bytes < v3d_dense_train_head_workspace(O)) return V3D_EWORKSPACE;
  const long long M = (long long)B * H * W;
  hipStream_t st = (hipStream_t)stream;
  const long long blocks = (M + 255) / 256;
  const long long want = (M + 63) / 64;
  const int wb = (int)(want < DT_HEAD_BLOCKS ? want : DT_HEAD_BLOCKS);
  const unsigned db_ = (unsigned)(blocks < 2048 ? blocks : 2048);
#define DT_HEAD_CASE(OV)                                                                                                              \
  if (O == OV) {                                                                                                                      \
    hipLaunchKernelGGL(dt_head_bwd_data_kernel<OV>, dim3(db_), dim3(256), 0, st, dmaps, M, H * W, weight, (dt_bf16*)dfeat, (dt_bf16*)dfeat_lo); \
    hipLaunchKernelGGL(dt_head_bwd_weight_kernel<OV>, dim3(wb), dim3(256), 0, st, (const dt_bf16*)feat, (const dt_bf16*)feat_lo, dmaps, M, H * W, (float*)workspace); \
  } else
  DT_HEAD_CASE(8) DT_HEAD_CASE(16) DT_HEAD_CASE(24) DT_HEAD_CASE(32) DT_HEAD_CASE(48) DT_HEAD_CASE(64) return V3D_EUNSUPPORTED;
#undef DT_HEAD_CASE
  hipLaunchKernelGGL(dt_head_bwd_reduce_kernel, dim3(((O + 1) * DT_C + 31) / 32), dim3(DT_COLSUM_THREADS), 0, st, (const float*)workspace, wb, O, dweight, dbias);
  V3D_CHECK_LAUNCH();
  return V3D_OK;
}

extern "C" int v3d_dense_train_head_bwd(const void* feat, const float* dmaps, int B, int H, int W, const float* weight, int O, void* dfeat,
                                        float* dweight, float* dbias, void* workspace, size_t workspace_bytes, v3d_stream_t stream) {
  return dt_head_bwd(feat, nullptr, dmaps, B, H, W, weight, O, dfeat, nullptr, dweight, dbias, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ one call per direction
// The whole dense half of a train step enqueued by ONE native call each way (the host side of ~120 kernel launches: as for the
// sparse training plan, a Python-level operator chain would leave the step host-bound).  The caller owns the arena (a plain
// device buffer of v3d_dense_train_arena_bytes[_split]; nothing in it is read before it is written) -- it carries what the backward
// needs from the forward: every layer's raw convolution output and post-ReLU activation, the batch statistics, the weight images.
//
// ONE driver (dt_forward, dt_backward) runs the step in both arithmetics; `split` picks the primitive of a step (dt_step_*, dt_wgrad):
//   bf16 storage                              the kernels of this file; one plane per tensor
//   split ("bf16x3", the fp32-class step of   every tensor a pair of planes (16 significant bits), every product three MFMA terms
//   the reference's train.py:58-66)           (hi*hi + hi*lo + lo*hi, fp32 accumulation: 2^-17 per product, scale-free):
//     convolutions, forward and data gradient   csrc/dense_conv.hip's bf16x3 kernels (the inference RPN's), raw output, no epilogue;
//                                               the data gradient is the same convolution on the channel-swapped, tap-flipped weights
//     weight gradient                           dt_wgrad_kernel three times into three sets of slab partials, one reduction
//     batch statistics, BN + ReLU, their        the kernels above on hi + lo (fp32 arithmetic; statistics from the stored values:
//     backward, the head's gradients            dt_bn_stats_kernel; fixed-order two-level reductions as before)
//     head forward                              dense_conv.hip's 1x1 stream kernel (bias, fp32 NCHW maps)
//   About 2.4x the traffic and 3x the matrix work of the bf16-storage step; no tensor of it ever exists in reduced precision.
struct DtArena {
  bool split;
  int B, H, W, stat_rows;  // stat_rows: rows of the statistics partials (bf16: workgroups of the convolution; split: of dt_bn_stats_kernel)
  long long M;
  size_t plane, slot, img;  // bytes of one bf16 plane of a tensor, of a tensor (1 or 2 planes), of a weight image
  size_t off_raw, off_act, off_stat, off_partial, off_img, off_himg, off_wt, off_g0, off_g1, off_ws, total;  // himg, wt: split only
  unsigned char* base;
  DtT at(size_t off, int l = 0) const {
    unsigned char* p = base + off + (size_t)l * slot;
    return DtT{p, split ? p + plane : nullptr};
  }
  void* image(int i) const { return base + off_img + (size_t)i * img; }  // 2 l: layer l forward, 2 l + 1: its data gradient
};
static DtArena dt_arena_layout(int B, int H, int W, int n_layers, int O, bool split, void* arena = nullptr) {
  DtArena a;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  a.split = split; a.B = B; a.H = H; a.W = W; a.base = (unsigned char*)arena;
  a.M = (long long)B * H * W;
  const long long want = (a.M + 15) / 16;
  a.stat_rows = split ? (int)(want < DT_RED_BLOCKS ? want : DT_RED_BLOCKS) : v3d_dense_train_conv_tiles(B, H, W);
  a.plane = up((size_t)B * H * W * DT_C * 2);
  a.slot = (split ? 2 : 1) * a.plane;
  a.img = up(split ? v3d_conv2d_weight_image_bytes(DT_C, DT_C, 3) : (size_t)9 * DT_B_BYTES);
  size_t o = 0;
  a.off_raw = o; o += (size_t)n_layers * a.slot;
  a.off_act = o; o += (size_t)n_layers * a.slot;
  a.off_stat = o; o += up((size_t)n_layers * 2 * DT_C * 4);
  a.off_partial = o; o += up((size_t)(split ? DT_RED_BLOCKS : a.stat_rows) * 2 * DT_C * 4);
  a.off_img = o; o += (size_t)n_layers * 2 * a.img;
  a.off_himg = o; o += split ? up(v3d_conv2d_weight_image_bytes(DT_C, O, 1)) : 0;  // the head's image
  a.off_wt = o; o += split ? up((size_t)9 * DT_C * DT_C * 4) : 0;                  // a layer's flipped fp32 weights
  a.off_g0 = o; o += a.slot;
  a.off_g1 = o; o += a.slot;
  size_t ws = (split ? 3 : 1) * v3d_dense_train_wgrad_workspace(3);
  if (v3d_dense_train_head_workspace(O) > ws) ws = v3d_dense_train_head_workspace(O);
  if (v3d_dense_train_bn_bwd_workspace() > ws) ws = v3d_dense_train_bn_bwd_workspace();
  a.off_ws = o; o += up(ws);
  a.total = o;
  return a;
}

extern "C" size_t v3d_dense_train_arena_bytes(int B, int H, int W, int n_layers, int O) {
  return B < 1 || H < 1 || W < 1 || n_layers < 1 || O < 1 ? 0 : dt_arena_layout(B, H, W, n_layers, O, false).total;
}
extern "C" size_t v3d_dense_train_arena_bytes_split(int B, int H, int W, int n_layers, int O) {
  return B < 1 || H < 1 || W < 1 || n_layers < 1 || O < 1 ? 0 : dt_arena_layout(B, H, W, n_layers, O, true).total;
}

// (kept for the C ABI: nothing in the arena is read before it is written)
extern "C" int v3d_dense_train_arena_init(void* arena, int, int, int, int, int, v3d_stream_t) { return arena ? V3D_OK : V3D_EINVAL; }

// wt[ci][co][t] = w[co][ci][taps - 1 - t]: the data gradient's weights of the split path, before dense_conv.hip packs them
__global__ __launch_bounds__(256) void dt_wt_flip_kernel(const float* __restrict__ w, int taps, float* __restrict__ wt) {
  const int total = DT_C * DT_C * taps;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int t = i % taps, co = (i / taps) % DT_C, ci = i / (taps * DT_C);
    wt[i] = w[((size_t)co * DT_C + ci) * taps + (taps - 1 - t)];
  }
}

// the step's weight images (read again by the backward call: the weights do not change between the two calls of a step)
static int dt_step_pack(const DtArena& a, const v3d_dense_train_layer* layers, int n_layers, const float* head_weight, int O, v3d_stream_t stream) {
  if (!a.split) {
    DtPackJobs jobs;
    for (int l = 0; l < n_layers; l++) {
      jobs.w[l] = layers[l].weight;
      jobs.taps[l] = layers[l].ksize * layers[l].ksize;
    }
    hipLaunchKernelGGL(dt_pack_all_kernel, dim3(32, 2 * n_layers), dim3(256), 0, (hipStream_t)stream, jobs, a.base + a.off_img, a.img);
    return V3D_OK;
  }
  float* wt = (float*)(a.base + a.off_wt);
  for (int l = 0; l < n_layers; l++) {
    const v3d_dense_train_layer& L = layers[l];
    DT_TRY(v3d_conv2d_pack_weights(L.weight, nullptr, DT_C, DT_C, L.ksize, V3D_PREC_BF16X3, a.image(2 * l), stream));
    hipLaunchKernelGGL(dt_wt_flip_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, L.weight, L.ksize * L.ksize, wt);
    DT_TRY(v3d_conv2d_pack_weights(wt, nullptr, DT_C, DT_C, L.ksize, V3D_PREC_BF16X3, a.image(2 * l + 1), stream));
  }
  return v3d_conv2d_pack_weights(head_weight, nullptr, O, DT_C, 1, V3D_PREC_BF16X3, a.base + a.off_himg, stream);
}

// y = the raw convolution of x (no bias, no activation) -- a forward layer, or the data gradient on image 2 l + 1.
// partial (forward only): the batch-statistics partials of y, a.stat_rows rows.
static int dt_step_conv(const DtArena& a, DtT x, const void* image, int ksize, DtT y, float* partial, v3d_stream_t stream) {
  if (!a.split) return v3d_dense_train_conv(x.hi, image, a.B, a.H, a.W, ksize, y.hi, partial, stream);
  DT_TRY(dt_conv2d_plain(x.hi, x.lo, image, nullptr, 0, a.B, a.H, a.W, DT_C, DT_C, ksize, y.hi, y.lo, nullptr, stream));
  if (partial)
    hipLaunchKernelGGL(dt_bn_stats_kernel, dim3(a.stat_rows), dim3(256), 0, (hipStream_t)stream, (const dt_bf16*)y.hi, (const dt_bf16*)y.lo, a.M,
                       partial);
  return V3D_OK;
}

static int dt_step_head_fwd(const DtArena& a, DtT x, const float* weight, const float* bias, int O, float* maps, v3d_stream_t stream) {
  if (!a.split) return v3d_dense_train_head_fwd(x.hi, a.B, a.H, a.W, weight, bias, O, maps, stream);
  V3D_CHECK_LAUNCH();
  return dt_conv2d_plain(x.hi, x.lo, a.base + a.off_himg, bias, 0, a.B, a.H, a.W, DT_C, O, 1, nullptr, nullptr, maps, stream);
}

static int dt_forward(DtT bev, int B, int H, int W, const v3d_dense_train_layer* layers, int n_layers, const float* head_weight,
                      const float* head_bias, int O, void* arena, float* maps, bool split, v3d_stream_t stream) {
  const DtArena a = dt_arena_layout(B, H, W, n_layers, O, split, arena);
  for (int l = 0; l < n_layers; l++)
    if (!layers[l].weight || !layers[l].gamma || !layers[l].beta || (layers[l].ksize != 1 && layers[l].ksize != 3)) return V3D_EINVAL;
  DT_TRY(dt_step_pack(a, layers, n_layers, head_weight, O, stream));
  float* partial = (float*)(a.base + a.off_partial);
  DtT x = bev;
  for (int l = 0; l < n_layers; l++) {
    const v3d_dense_train_layer& L = layers[l];
    const DtT raw = a.at(a.off_raw, l), act = a.at(a.off_act, l);
    float* mean = (float*)(a.base + a.off_stat) + (size_t)l * 2 * DT_C;
    DT_TRY(dt_step_conv(a, x, a.image(2 * l), L.ksize, raw, partial, stream));
    DT_TRY(v3d_dense_train_bn_finalize(partial, a.stat_rows, a.M, L.eps, L.momentum, mean, mean + DT_C, L.running_mean, L.running_var,
                                       L.num_batches_tracked, stream));
    DT_TRY(dt_bn_relu_apply(raw, a.M, mean, mean + DT_C, L.gamma, L.beta, 1, act, stream));
    x = act;
  }
  return dt_step_head_fwd(a, x, head_weight, head_bias, O, maps, stream);
}

static int dt_backward(DtT bev, const float* dmaps, int B, int H, int W, const v3d_dense_train_layer* layers, int n_layers,
                       const float* head_weight, int O, void* arena, float* dhead_weight, float* dhead_bias, DtT dbev, bool split,
                       v3d_stream_t stream) {
  const DtArena a = dt_arena_layout(B, H, W, n_layers, O, split, arena);
  void* ws = a.base + a.off_ws;
  const size_t ws_bytes = a.total - a.off_ws;
  const DtT g[2] = {a.at(a.off_g0), a.at(a.off_g1)};
  const DtT feat = a.at(a.off_act, n_layers - 1);
  DT_TRY(dt_head_bwd(feat.hi, feat.lo, dmaps, B, H, W, head_weight, O, g[0].hi, g[0].lo, dhead_weight, dhead_bias, ws, ws_bytes, stream));
  int cur = 0;  // g[cur] = gradient w.r.t. the post-ReLU output of layer l
  for (int l = n_layers - 1; l >= 0; l--) {
    const v3d_dense_train_layer& L = layers[l];
    if (!L.grad_weight || !L.grad_gamma || !L.grad_beta || (L.ksize != 1 && L.ksize != 3)) return V3D_EINVAL;
    const DtT raw = a.at(a.off_raw, l), xin = l == 0 ? bev : a.at(a.off_act, l - 1);
    const float* mean = (const float*)(a.base + a.off_stat) + (size_t)l * 2 * DT_C;
    // gradient w.r.t. the raw convolution output, in place
    DT_TRY(dt_bn_relu_bwd(raw.hi, raw.lo, g[cur].hi, g[cur].lo, a.M, mean, mean + DT_C, L.gamma, L.beta, 1, g[cur].hi, g[cur].lo, L.grad_gamma,
                          L.grad_beta, ws, ws_bytes, stream));
    DT_TRY(dt_wgrad(xin, g[cur], B, H, W, L.ksize, L.grad_weight, ws, ws_bytes, stream));
    DT_TRY(dt_step_conv(a, g[cur], a.image(2 * l + 1), L.ksize, l == 0 ? dbev : g[cur ^ 1], nullptr, stream));
    cur ^= 1;
  }
  return V3D_OK;
}

// bev: bf16 NHWC (B, H, W, 128) -> maps fp32 (B, O, H, W).  layers[l]: weight (128, 128, k, k), gamma, beta, running statistics.
extern "C" int v3d_dense_train_forward(const void* bev, int B, int H, int W, const v3d_dense_train_layer* layers, int n_layers,
                                       const float* head_weight, const float* head_bias, int O, void* arena, float* maps,
                                       v3d_stream_t stream) {
  if (!bev || !layers || !arena || !maps || !head_weight || n_layers < 1 || n_layers > 16) return V3D_EINVAL;
  return dt_forward(dt_t(bev), B, H, W, layers, n_layers, head_weight, head_bias, O, arena, maps, false, stream);
}

// dmaps fp32 (B, O, H, W) -> gradients of every layer (layers[l].grad_*), of the head, and of the input (dbev, bf16 NHWC).
extern "C" int v3d_dense_train_backward(const void* bev, const float* dmaps, int B, int H, int W, const v3d_dense_train_layer* layers,
                                        int n_layers, const float* head_weight, int O, void* arena, float* dhead_weight,
                                        float* dhead_bias, void* dbev, v3d_stream_t stream) {
  if (!bev || !dmaps || !layers || !arena || !head_weight || !dhead_weight || !dhead_bias || !dbev || n_layers < 1 || n_layers > 16)
    return V3D_EINVAL;
  return dt_backward(dt_t(bev), dmaps, B, H, W, layers, n_layers, head_weight, O, arena, dhead_weight, dhead_bias, dt_t(dbev), false, stream);
}

// the same step on split NHWC planes (B, H, W, 128): bev_hi + bev_lo -> maps fp32 (B, O, H, W)
extern "C" int v3d_dense_train_forward_split(const void* bev_hi, const void* bev_lo, int B, int H, int W, const v3d_dense_train_layer* layers,
                                             int n_layers, const float* head_weight, const float* head_bias, int O, void* arena, float* maps,
                                             v3d_stream_t stream) {
  if (!bev_hi || !bev_lo || !layers || !arena || !maps || !head_weight || n_layers < 1 || n_layers > 16 || O < 1 || O > 16) return V3D_EINVAL;
  if ((long long)B * H * W > 0x7FFFFFF0ll / DT_C) return V3D_EINVAL;
  return dt_forward(dt_t(bev_hi, bev_lo), B, H, W, layers, n_layers, head_weight, head_bias, O, arena, maps, true, stream);
}

// dmaps fp32 (B, O, H, W) -> gradients of every layer, of the head, and of the input (dbev: split NHWC planes)
extern "C" int v3d_dense_train_backward_split(const void* bev_hi, const void* bev_lo, const float* dmaps, int B, int H, int W,
                                              const v3d_dense_train_layer* layers, int n_layers, const float* head_weight, int O, void* arena,
                                              float* dhead_weight, float* dhead_bias, void* dbev_hi, void* dbev_lo, v3d_stream_t stream) {
  if (!bev_hi || !bev_lo || !dmaps || !layers || !arena || !head_weight || !dhead_weight || !dhead_bias || !dbev_hi || !dbev_lo || n_layers < 1 ||
      n_layers > 16 || O < 1 || O > 16)
    return V3D_EINVAL;
  return dt_backward(dt_t(bev_hi, bev_lo), dmaps, B, H, W, layers, n_layers, head_weight, O, arena, dhead_weight, dhead_bias,
                     dt_t(dbev_hi, dbev_lo), true, stream);
}
