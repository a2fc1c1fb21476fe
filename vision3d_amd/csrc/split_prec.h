// split_prec.h -- the split-precision arithmetic of every convolution in the library, stated ONCE: the sparse kernels (sp_device.h:
// spconv.hip, brick.hip), the dense head (dense_conv.hip) and the dense train step (dense_train.hip) all split, scale, pack and
// multiply through the helpers below, so a producer and a consumer of split data cannot disagree on a rounding rule, a target
// exponent or a trailer word.  Needs <hip/hip_runtime.h> only (tools/mb_f16split.hip includes it on its own).
//
// ---- the split-precision product, two arithmetics (template parameter PREC of every packed kernel) ----
// Both evaluate  a * w = al*Wh + ah*Wl + ah*Wh  (three MFMA terms, fp32 accumulation, smallest terms first) on operands split into
// hi = rne(x), lo = rne(x - hi); they differ in the 16-bit format of the pieces:
//   PREC 0 "bf16x3"  bf16 pieces: 8 + 8 significant bits, 2^-17 per product, any fp32 magnitude (no scale to choose): the arithmetic
//                    of rounds 1-4, kept for the training plan (gradients span too many binades for a per-tensor scale) and as
//                    the library's `fast` inference mode.  Strict elementwise error of a SECOND layer against float64 on entries
//                    above 1e-3 of the layer maximum: 1.1e-3 ... 2.1e-3 (torch's fp32 conv3d: 2e-5 ... 1.1e-4).
//   PREC 1 "f16s"    f16 pieces of x * s with a power-of-two scale s per tensor: 11 + 11 significant bits, 2^-22 per product --
//                    the error of a 1 728-term dot product is then fp32's own accumulation noise (tools/mb_f16split.hip on MI355X:
//                    strict relative error max 1.0e-4 / rms 2.2e-6 against 1.7e-4 / 2.5e-6 for the exact-fp32 MFMA and
//                    2.1e-3 / 5.5e-5 for bf16x3), at the SAME three MFMAs.  v_mfma_f32_16x16x32_f16 keeps subnormal f16 inputs
//                    (probed), so a piece below 2^-14 degrades to the 2^-24 quantum instead of vanishing: with the tensor's
//                    maximum scaled to 2^8 ... 2^14 everything down to 2^-17 of the maximum keeps full precision.
//                    The scales: activations -- V3dActScale: {s, 1/s, limit} in device memory, chosen by the caller from the
//                    observed maximum of the tensor with headroom (runtime.py: calibration); an output beyond the CONSUMER's
//                    limit raises a device flag (the frame is then re-run after recalibration, like a capacity overflow) --;
//                    weights -- per layer from max|W| at pack time, its inverse in the image's trailer.  Scaling by powers of
//                    two is exact, so the result does not depend on the scales as long as nothing leaves the f16 range.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

// 16-byte fragment registers and the 2-wide converter types.  u32x4 is a native vector type on purpose: HIP's uint4 is a struct with
// a union inside and an array of them is NOT promoted to registers (it round-tripped through scratch every k-step: 142 us/conv).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// ---- scales and the weight-image trailer ------------------------------------------------------------------------------------------
// power-of-two scale that puts a tensor whose largest magnitude has the fp32 bits `amax_bits` into [2^target, 2^(target + 1)):
// only the exponent is used.  Zero / subnormal maxima give 1; the exponent is clamped so that the scale AND its inverse are normal.
// (runtime.scale_entry_from_max restates this in Python.)
__host__ __device__ static inline float v3d_pow2_scale(unsigned amax_bits, int target) {
  const int eb = (int)((amax_bits >> 23) & 0xFFu);
  if (eb == 0 || eb == 255) return 1.f;
  int sb = 127 + target - (eb - 127);
  sb = sb < 2 ? 2 : (sb > 252 ? 252 : sb);
  const unsigned bits = (unsigned)sb << 23;
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(bits);
#else
  float f;
  memcpy(&f, &bits, 4);
  return f;
#endif
}
#define V3D_F16S_WEIGHT_TARGET 13  // max|W| * s_w in [2^13, 2^14)
#define V3D_F16S_ACT_TARGET 13     // max|x| * s in [2^(13 - headroom), 2^(14 - headroom))

// trailer of a packed weight image, sparse and dense alike (every precision allocates it; PREC 1 fills it), 32-bit words:
#define V3D_WIMG_TRAILER 256  // bytes
enum { V3D_WIMG_MAX_BITS = 0 /*fp32 bits of max|W|*/, V3D_WIMG_INV_SCALE = 1 /*1 / s_w*/, V3D_WIMG_SCALE = 2 /*s_w*/, V3D_WIMG_PREC = 3 /*1: f16s*/ };

// max |w * factor[t / per_cout]| of a weight tensor of `n` values into word 0 of the image's trailer (zeroed by the caller; `factor`
// nullable): non-negative floats order like their bits.  A static template: an object that launches it carries its own copy.
template <int = 0>
static __global__ void v3d_wmax_kernel(const float* __restrict__ w, const float* __restrict__ factor, long long per_cout, long long n,
                                       unsigned* __restrict__ trailer) {
  unsigned m = 0u;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    float v = w[t];
    if (factor) v *= factor[t / per_cout];
    m = max(m, __float_as_uint(v) & 0x7FFFFFFFu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(trailer + V3D_WIMG_MAX_BITS, m);
}
// f16s pack kernels, every thread: s_w from the maximum in word 0; the grid's first thread completes the trailer
__device__ __forceinline__ float v3d_wimg_weight_scale(unsigned* __restrict__ trailer) {
  const float sw = v3d_pow2_scale(trailer[V3D_WIMG_MAX_BITS], V3D_F16S_WEIGHT_TARGET);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    reinterpret_cast<float*>(trailer)[V3D_WIMG_INV_SCALE] = 1.f / sw;
    reinterpret_cast<float*>(trailer)[V3D_WIMG_SCALE] = sw;
    trailer[V3D_WIMG_PREC] = 1u;
  }
  return sw;
}

// ---- the product --------------------------------------------------------------------------------------------------------------------
template <int PREC>
__device__ __forceinline__ f32x4 split_mfma(const u32x4 a, const u32x4 b, const f32x4 c) {
#ifdef SP_EXP_F16S_BF16_MFMA  // experiment only (wrong results): the f16s kernels on the bf16 instruction -- is the f16 MFMA itself slower?
  if constexpr (true)
#else
  if constexpr (PREC == 0)
#endif
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- bf16 in software and on the hardware converter ----------------------------------------------------------------------------------
__device__ __forceinline__ unsigned bf16_rne_bits(float f) {  // (inf / nan: truncated)
  unsigned u = __float_as_uint(f);
  if ((u & 0x7F800000u) == 0x7F800000u) return u >> 16;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }
__device__ __forceinline__ unsigned bf16_pack2(float a, float b) {  // two fp32 -> packed bf16 pair (RNE, v_cvt_pk_bf16_f32)
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ unsigned short bf16_from_f32(float a) { return (unsigned short)(bf16_pack2(a, 0.f) & 0xFFFFu); }
__device__ __forceinline__ void bf16_unpack8(const u32x4 v, float (&x)[8]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    x[2 * i] = __uint_as_float(v[i] << 16);
    x[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u);
  }
}

// ---- the split ------------------------------------------------------------------------------------------------------------------------
// f16s: (x0, x1) -> packed f16 pairs hi = rne(x * s), lo = rne(x * s - hi) in FOUR instructions.  v_fma_mix{lo,hi}_f16 evaluate
// fma(a, b, c) on f32 / f16 sources chosen per operand and round ONCE to f16 into one half of the destination: hi = fma(x, s, 0);
// lo = fma(x, s, -hi) with the f16 half of `hi` read in place -- x * s is exact (s is a power of two) and x * s - hi fits 14 bits, so
// both are the values of the plain expressions (checked bit for bit by tools/mb_f16split.hip), without the multiply, the two
// conversions back and the subtraction (8 VALU operations per pair; the bf16 split takes 6: there is no bf16 mix instruction).
// `s` must be wave-uniform (an SGPR operand).
__device__ __forceinline__ void v3d_split_f16_pair(const float x0, const float x1, const float s, unsigned& hi, unsigned& lo) {
  unsigned h = 0u, l = 0u;
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass only parses the declaration)
  asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(h) : "v"(x0), "s"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(h) : "v"(x1), "s"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(x0), "s"(s), "v"(h));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(x1), "s"(s), "v"(h));
#endif
  hi = h;
  lo = l;
}

// one value -> (hi, lo) 16-bit patterns in plain expressions (pack kernels, densify); PREC 1: of v * s
template <int PREC>
__device__ __forceinline__ void split_one(const float v, const float s, unsigned short& hi, unsigned short& lo) {
  if constexpr (PREC == 0) {
    const unsigned h = bf16_rne_bits(v);
    hi = (unsigned short)h;
    lo = (unsigned short)bf16_rne_bits(v - __uint_as_float(h << 16));
  } else {
    const float a = v * s;
    const _Float16 h = (_Float16)a;
    const _Float16 l = (_Float16)(a - (float)h);
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, l);
  }
}

// (v0, v1) -> packed hi pair and lo pair, both RNE on the hardware converters (v_cvt_pk_bf16_f32) / the mix instructions above: the
// hot epilogues.  PREC 1: of v * s (s: the tensor's power-of-two scale, read through readfirstlane: wave-uniform).
template <int PREC>
__device__ __forceinline__ void split_pair(const float v0, const float v1, const float s, unsigned& hi, unsigned& lo) {
#ifdef SP_EXP_F16S_BF16_SPLIT  // experiment only (wrong results): the f16s kernels with the bf16 split's instructions
  if constexpr (true) {
#else
  if constexpr (PREC == 0) {
#endif
    hi = bf16_pack2(v0, v1);
    lo = bf16_pack2(v0 - __uint_as_float(hi << 16), v1 - __uint_as_float(hi & 0xFFFF0000u));
  } else {
    v3d_split_f16_pair(v0, v1, __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, s))), hi, lo);
  }
}

// 8 fp32 activations -> packed hi / lo fragments
template <int PREC>
__device__ __forceinline__ void split_act(const float (&x)[8], const float s, u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    unsigned h, l;
    split_pair<PREC>(x[2 * i], x[2 * i + 1], s, h, l);
    hi[i] = h;
    lo[i] = l;
  }
}
