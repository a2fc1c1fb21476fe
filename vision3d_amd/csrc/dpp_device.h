// dpp_device.h -- wave64 max / min reductions on the DPP data path, shared by the sampling kernels (pointops.hip, keypoints.hip).
#pragma once
#include "v3d_common.h"

// Wave64 / row-of-16 max and min reductions on the DPP data path (VALU latency; __shfl_xor goes through ds_bpermute,
// ~90 clocks per hop).  max/min are idempotent, so lanes whose DPP source is out of range simply combine with their
// own value.  quad swaps, row_shr:4, row_shr:8 leave lane 15 of every row with the row result; row_bcast:15 and
// row_bcast:31 carry it on to lane 63.
#define V3D_DPP_I(v, ctrl) __builtin_amdgcn_update_dpp((v), (v), (ctrl), 0xf, 0xf, false)
template <bool FULL>
__device__ __forceinline__ float v3d_dpp_max_f32(float v) {
#define STEP(ctrl) v = fmaxf(v, __int_as_float(V3D_DPP_I(__float_as_int(v), ctrl)))
  STEP(0xb1); STEP(0x4e); STEP(0x114); STEP(0x118);
  if (FULL) { STEP(0x142); STEP(0x143); }
#undef STEP
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), FULL ? 63 : 15));
}
// Wave64 fp32 sum on the same path (box_voting.hip).  A sum is not idempotent, so a lane whose DPP source is out of range, or whose
// row a step does not write, must add ZERO: `old` is 0.0f.  The quad swaps give every lane its quad's sum; row_shr:4 and row_shr:8
// leave the row's sum in its last quad; row_bcast:15 into rows 1 and 3 (row mask 0xa) and row_bcast:31 into rows 2 and 3 (0xc) carry
// it on, and lane 63 holds the wave's sum, which every lane receives.  The order of the additions is fixed: the result is
// deterministic.
__device__ __forceinline__ float v3d_dpp_sum_f32(float v) {
#define STEP(ctrl, rows) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), (ctrl), (rows), 0xf, false))
  STEP(0xb1, 0xf); STEP(0x4e, 0xf); STEP(0x114, 0xf); STEP(0x118, 0xf); STEP(0x142, 0xa); STEP(0x143, 0xc);
#undef STEP
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
template <bool FULL>
__device__ __forceinline__ int v3d_dpp_min_i32(int v) {
#define STEP(ctrl) v = min(v, V3D_DPP_I(v, ctrl))
  STEP(0xb1); STEP(0x4e); STEP(0x114); STEP(0x118);
  if (FULL) { STEP(0x142); STEP(0x143); }
#undef STEP
  return __builtin_amdgcn_readlane(v, FULL ? 63 : 15);
}
