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
template <bool FULL>
__device__ __forceinline__ int v3d_dpp_min_i32(int v) {
#define STEP(ctrl) v = min(v, V3D_DPP_I(v, ctrl))
  STEP(0xb1); STEP(0x4e); STEP(0x114); STEP(0x118);
  if (FULL) { STEP(0x142); STEP(0x143); }
#undef STEP
  return __builtin_amdgcn_readlane(v, FULL ? 63 : 15);
}
