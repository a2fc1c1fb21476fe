// pillar_plane_device.h -- where a pillar's row lands in the dense head's input (cfg.PILLAR.PLAN; pillar.hip "the plan's front"):
// ONE statement of the live row count, the pixel of a row and the word / bit of that pixel in the inverted occupancy bitmap.
// pillar.hip runs it on the GPU, tests/host/pillar_plan_host_shim.cpp compiles the same text with g++ under the sanitizers.
//
// The map is (B, H, W) pixels of CH channels, two 16-bit planes (hi, lo) laid out [(b * H + y) * W + x][channel]; the bitmap is the
// one v3d_bev_occupancy_bits writes: row (b, y) = ceil(W / 32) words, bit x % 32 of word x / 32, INVERTED (cleared = occupied).
// A row's pixel is (b, y, x) = coordinates[m][0, 2, 3]; the z index is ignored (PillarFeatureNet.canvas writes every row at z = 0).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define V3D_PP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define V3D_PP_HD inline
#endif

namespace v3d {

// rows a launch may touch: the device count clamped to [0, cap] (a stale or hand-fed count never reaches past the buffers)
V3D_PP_HD int pillar_live_rows(int n_voxels, int cap) { return n_voxels < 0 ? 0 : (n_voxels > cap ? cap : n_voxels); }

// pixel index (b * H + y) * W + x of the row with coordinates c[0..3] = (b, z, y, x), or -1 when it lies outside the map: such a row
// is skipped -- never stored, never marked (the voxelizer produces none; a hand-fed list must not write out of bounds)
V3D_PP_HD long long pillar_plane_pixel(const int32_t* c, int B, int H, int W) {
  const int b = c[0], y = c[2], x = c[3];
  if (b < 0 || b >= B || y < 0 || y >= H || x < 0 || x >= W) return -1;
  return ((long long)b * H + y) * W + x;
}

V3D_PP_HD int pillar_occ_words_per_row(int W) { return (W + 31) >> 5; }

// word index and bit mask of pixel `pix` (>= 0) in the bitmap
V3D_PP_HD size_t pillar_occ_word(long long pix, int W) {
  const long long row = pix / W;
  const int x = (int)(pix - row * W);
  return (size_t)row * pillar_occ_words_per_row(W) + (size_t)(x >> 5);
}
V3D_PP_HD uint32_t pillar_occ_bit(long long pix, int W) { return 1u << ((int)(pix % W) & 31); }

}  // namespace v3d
