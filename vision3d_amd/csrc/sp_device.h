// sp_device.h -- device helpers shared by the packed sparse-convolution kernels (spconv.hip, brick.hip): split-row epilogues on the
// split-precision arithmetic of split_prec.h, scale entries, hand-issued loads with counted waits, LDS-DMA.
#pragma once
#include "v3d_internal.h"
#include "split_prec.h"

// INS = 1: the gathered rows are ALREADY split (row = [hi: C x 16 bit | lo: C x 16 bit], the bytes of the fp32 row): the producing layer
// wrote them that way under THIS layer's scale entry (sp_store_split below), so the lane's two 16-byte loads return its hi and lo
// fragments directly and the main loop has no conversion work at all.  The 8 dwords travel in the same `float[8]` registers the
// fp32 path uses: [0..3] = hi, [4..7] = lo.
template <int PREC, int INS>
__device__ __forceinline__ void split_in(const float (&x)[8], const float s, u32x4& hi, u32x4& lo) {
  if constexpr (INS) {
    hi = u32x4{__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3])};
    lo = u32x4{__float_as_uint(x[4]), __float_as_uint(x[5]), __float_as_uint(x[6]), __float_as_uint(x[7])};
  } else {
    split_act<PREC>(x, s, hi, lo);
  }
}

// Epilogue, second copy of an output row for the NEXT packed layer: the row split into pieces (of v * s: the consumer's scale entry).
// A lane holds D[row][col = j * 16 + r]; lanes r and r ^ 1 hold neighbouring columns of the same row: they exchange their values
// (one DPP move), both split the pair, the even lane stores the hi pair and the odd lane the lo pair -- one 4-byte store per
// value and lane, as many store instructions as the fp32 row takes.  Every lane of a pair must call this (rows are uniform
// across the 16 lanes that share (kg, rr): the callers' `row < n` test keeps pairs together).
template <int PREC, int COUT>
__device__ __forceinline__ void sp_store_split(unsigned short* __restrict__ out_s, const int row, const int col, const int r, const float v,
                                               const float s) {
  const float pv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1 /*quad_perm [1,0,3,2]*/, 0xF, 0xF, true));
  unsigned h, l;
  split_pair<PREC>((r & 1) ? pv : v, (r & 1) ? v : pv, s, h, l);
  *reinterpret_cast<unsigned*>(out_s + (size_t)row * (2 * COUT) + ((r & 1) ? COUT : 0) + (col & ~1)) = (r & 1) ? l : h;
}

// ---- epilogue stores of a 16-row output tile, COALESCED through LDS -------------------------------------------------------------
// Measured in round 6 (profiles/r06_brick_ablation.txt): storing a tile straight from the MFMA accumulator layout -- a lane holds
// D[row = kg * 4 + rr][col = j * 16 + r], so every store instruction of the wave writes eight 32-byte (split rows) or four 64-byte
// (fp32 rows) pieces of four different rows -- costs ~300 clocks per store instruction: 11.5 us of a 45 us 64 -> 64 launch at 56 k
// rows went into the 128 store instructions per lane of its epilogue.  The rows of a tile are CONSECUTIVE rows of the output array,
// i.e. one contiguous block of 16 x ROWB bytes: the wave writes its values into a private LDS staging block (4-byte ds_writes, row
// stride ROWB + 16 so that the four kg row groups fall on different banks) and stores the block with 16-byte stores of consecutive
// lanes -- ROWB / 64 fully coalesced store instructions per tile instead of 4 * NB.  Same bytes in memory.
//   stage: LDS scratch PRIVATE to the wave, SP_STAGE_BYTES(COUT) bytes, 16-byte aligned (no barrier: a wave's LDS operations
//          execute in order); v[j][rr]: the finished values; nv: rows of the tile that exist (rows >= nv are not stored).
#define SP_STAGE_STRIDE(COUT) ((COUT) * 4 + 16)
#define SP_STAGE_BYTES(COUT) (16 * SP_STAGE_STRIDE(COUT))
// NT = threads that flush together (64: a wave's private block; a workgroup's size: a block shared behind a barrier), t = the caller's index in them
template <int COUT, int NT = 64>
__device__ __forceinline__ void sp_stage_flush(const unsigned char* stage, unsigned char* __restrict__ dst_tile, const int nv, const int t) {
  constexpr int ROWB = COUT * 4, CPR = ROWB / 16;  // bytes and 16-byte chunks per row
#pragma unroll
  for (int i = 0; i < (16 * CPR + NT - 1) / NT; i++) {
    const int ch = i * NT + t, row = ch / CPR, wc = ch % CPR;
    if (ch < 16 * CPR && row < nv)
      *reinterpret_cast<uint4*>(dst_tile + (size_t)row * ROWB + wc * 16) = *reinterpret_cast<const uint4*>(stage + row * SP_STAGE_STRIDE(COUT) + wc * 16);
  }
}
// one value D[rowi][col] into a staging block: as fp32 / as its half of a split pair (lanes r, r ^ 1 hold neighbouring columns of the
// same row: every lane of the pair must call this)
template <int COUT>
__device__ __forceinline__ void sp_stage_put_f32(unsigned char* stage, const int rowi, const int col, const float v) {
  *reinterpret_cast<float*>(stage + rowi * SP_STAGE_STRIDE(COUT) + col * 4) = v;
}
template <int PREC, int COUT>
__device__ __forceinline__ void sp_stage_put_split(unsigned char* stage, const int rowi, const int col, const int r, const float v, const float s) {
  const float pv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1 /*quad_perm [1,0,3,2]*/, 0xF, 0xF, true));
  unsigned h, l;
  split_pair<PREC>((r & 1) ? pv : v, (r & 1) ? v : pv, s, h, l);
  *reinterpret_cast<unsigned*>(stage + rowi * SP_STAGE_STRIDE(COUT) + ((r & 1) ? COUT * 2 : 0) + (col & ~1) * 2) = (r & 1) ? l : h;
}
// fp32 rows (cap, COUT): out_tile = first row of the tile
template <int COUT, int NB>
__device__ __forceinline__ void sp_tile_store_f32(unsigned char* stage, float* __restrict__ out_tile, const float (&v)[NB][4], const int nv,
                                                  const int lane) {
  const int r = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int j = 0; j < NB; j++)
#pragma unroll
    for (int rr = 0; rr < 4; rr++) sp_stage_put_f32<COUT>(stage, kg * 4 + rr, j * 16 + r, v[j][rr]);
  sp_stage_flush<COUT>(stage, reinterpret_cast<unsigned char*>(out_tile), nv, lane);
}
// split rows (cap, 2 * COUT) 16-bit = [hi: COUT | lo: COUT] under the consumer's scale `s` (sp_store_split's bytes)
template <int PREC, int COUT, int NB>
__device__ __forceinline__ void sp_tile_store_split(unsigned char* stage, unsigned short* __restrict__ out_s_tile, const float (&v)[NB][4],
                                                    const float s, const int nv, const int lane) {
  const int r = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int j = 0; j < NB; j++)
#pragma unroll
    for (int rr = 0; rr < 4; rr++) sp_stage_put_split<PREC, COUT>(stage, kg * 4 + rr, j * 16 + r, r, v[j][rr], s);
  sp_stage_flush<COUT>(stage, reinterpret_cast<unsigned char*>(out_s_tile), nv, lane);
}

// PREC 1: scale of the input rows, the factor that undoes input and weight scales, and the consumer's limit on this launch's output
struct SpScales {
  float s_in, undo, limit;
};
template <int PREC>
__device__ __forceinline__ SpScales sp_scales(const V3dActScale& as, const unsigned short* wimg, size_t img_elems) {
  SpScales r{1.f, 1.f, 3.0e38f};
  if constexpr (PREC == 1) {
    r.s_in = as.in[0];
    r.undo = as.in[1] * (as.w_inv ? *as.w_inv : reinterpret_cast<const float*>(wimg + img_elems)[V3D_WIMG_INV_SCALE]);
    if (as.next) r.limit = as.next[2];
  }
  return r;
}
// an output beyond the consumer's limit: the frame's summary flag (<= 0: fine, 1: a capacity was hit, 2: out of f16s range)
// (every lane of the wave calls this, at the end of the kernel)
__device__ __forceinline__ void sp_range_check(const V3dActScale& as, const float vmax, const float limit) {
  if (as.flag && vmax > limit) atomicMax(as.flag, V3D_FLAG_RANGE);
  if (as.seen) v3d_mark_seen(as.seen, vmax, limit * (1.f / (float)(1 << V3D_QUIET_BITS)));
}

static __device__ __attribute__((aligned(256))) const float spr_zero_row[128] = {};

__device__ __forceinline__ void asm_gld16(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void asm_gld16_16(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void asm_gld16_128(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off offset:128" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void asm_gld16_144(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off offset:144" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void asm_gld4(int& d, const void* p) { asm volatile("global_load_dword %0, %1, off" : "=v"(d) : "v"(p) : "memory"); }
template <int N> __device__ __forceinline__ void vm_wait_tie(f32x4 (&a)[2]) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a[0]), "+v"(a[1]) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void vm_wait_tie(f32x4 (&a)[4]) { asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void vm_wait_tie(f32x4 (&a)[8]) {
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void vm_wait_tie(f32x4 (&a)[1]) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a[0]) : "n"(N) : "memory"); }
// (the same, additionally ordered behind the instruction that produces `after`: e.g. the last MFMA of a step)
template <int N> __device__ __forceinline__ void vm_wait_tie_after(f32x4 (&a)[1], f32x4& after) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a[0]), "+v"(after) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void vm_wait_tie_after(f32x4 (&a)[2], f32x4& after) { asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a[0]), "+v"(a[1]), "+v"(after) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void vm_wait_tie(int (&a)[1]) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a[0]) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void vm_wait_tie(int (&a)[2]) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a[0]), "+v"(a[1]) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void vm_wait_tie(int (&a)[3]) { asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]) : "n"(N) : "memory"); }

__device__ __forceinline__ void asm_gld16_64(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off offset:64" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void asm_gld16_192(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off offset:192" : "=v"(d) : "v"(p) : "memory"); }
// LDS-DMA of one 16-byte piece per lane: global address per lane, LDS destination = wave-uniform `lds_dst` + lane * 16 (M0 is
// compiler-reserved: saved and restored inside the statement).  No register destination: completion = the wave's vmcnt.
__device__ __forceinline__ void asm_dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// LDS byte address of a __shared__ object: the low half of its generic address (flat aperture base in the high half)
__device__ __forceinline__ unsigned lds_addr_of(const void* p) { return (unsigned)(unsigned long long)p; }
