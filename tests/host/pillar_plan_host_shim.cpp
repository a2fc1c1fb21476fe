// Host-side compile of vision3d_amd/csrc/pillar_plane_device.h (where a pillar's row lands in the dense head's planes and bitmap) as a
// STAND-ALONE program: tests/test_host_pillar_plan.py builds it with -fsanitize=address,undefined and runs it.  Test infrastructure
// only.  The loops below are the two kernels' of csrc/pillar.hip "the plan's front" without the lanes -- one row at a time, every
// store into a buffer of exactly the size the plan allocates, so a pixel, word or row index outside it stops the program.
// Usage: pillar_plan_host_shim  -> prints one line per case and "ok"; any failure returns non-zero.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../vision3d_amd/csrc/pillar_plane_device.h"

namespace {

constexpr int CH = 128;

struct Map {
  int B, H, W;
  std::vector<uint16_t> hi, lo;
  std::vector<uint32_t> occ;
  Map(int B_, int H_, int W_)
      : B(B_), H(H_), W(W_), hi((size_t)B_ * H_ * W_ * CH, 0), lo((size_t)B_ * H_ * W_ * CH, 0),
        occ((size_t)B_ * H_ * v3d::pillar_occ_words_per_row(W_), 0xFFFFFFFFu) {}
};

// pillar_encode_planes_kernel: row m stores the value m + 1 in every channel of its pixel.  .at(): a second, sanitizer-free bound check.
void encode(Map& mp, const std::vector<int32_t>& coords, int n_voxels, int cap) {
  const int M = v3d::pillar_live_rows(n_voxels, cap);
  for (int m = 0; m < M; m++) {
    const long long pix = v3d::pillar_plane_pixel(coords.data() + (size_t)m * 4, mp.B, mp.H, mp.W);
    if (pix < 0) continue;
    for (int c = 0; c < CH; c++) {
      mp.hi.at((size_t)pix * CH + c) = (uint16_t)(m + 1);
      mp.lo.at((size_t)pix * CH + c) = (uint16_t)(m + 1);
    }
    mp.occ.at(v3d::pillar_occ_word(pix, mp.W)) &= ~v3d::pillar_occ_bit(pix, mp.W);
  }
}

// pillar_planes_clear_kernel
void clear(Map& mp, const std::vector<int32_t>& prev, int prev_n, int cap) {
  for (auto& w : mp.occ) w = 0xFFFFFFFFu;
  const int M = v3d::pillar_live_rows(prev_n, cap);
  for (int m = 0; m < M; m++) {
    const long long pix = v3d::pillar_plane_pixel(prev.data() + (size_t)m * 4, mp.B, mp.H, mp.W);
    if (pix < 0) continue;
    for (int c = 0; c < CH; c++) mp.hi.at((size_t)pix * CH + c) = mp.lo.at((size_t)pix * CH + c) = 0;
  }
}

int fail(const char* what, int a, int b) {
  std::printf("FAILED %s (%d, %d)\n", what, a, b);
  return 1;
}

// the definition, pixel by pixel: the LAST in-map row of a pixel among the first `live` rows owns it; its bit is cleared
int check(const Map& mp, const std::vector<int32_t>& coords, int live) {
  const int wpr = (mp.W + 31) / 32;
  for (int b = 0; b < mp.B; b++)
    for (int y = 0; y < mp.H; y++)
      for (int x = 0; x < mp.W; x++) {
        int owner = 0;
        for (int m = 0; m < live; m++)
          if (coords[m * 4] == b && coords[m * 4 + 2] == y && coords[m * 4 + 3] == x) owner = m + 1;
        const size_t pix = ((size_t)b * mp.H + y) * mp.W + x;
        for (int c = 0; c < CH; c++)
          if (mp.hi[pix * CH + c] != owner || mp.lo[pix * CH + c] != owner) return fail("plane value", (int)pix, c);
        const bool bit = (mp.occ[((size_t)b * mp.H + y) * wpr + x / 32] >> (x % 32)) & 1u;
        if (bit != (owner == 0)) return fail("bitmap bit", (int)pix, owner);
      }
  // the padding bits of a row's last word stay set
  for (size_t r = 0; r < (size_t)mp.B * mp.H; r++)
    for (int x = mp.W; x < wpr * 32; x++)
      if (!((mp.occ[r * wpr + x / 32] >> (x % 32)) & 1u)) return fail("padding bit", (int)r, x);
  return 0;
}

std::vector<int32_t> rows_for(int B, int H, int W, int cap, unsigned seed, bool stray) {
  std::vector<int32_t> co((size_t)cap * 4);
  unsigned s = seed;
  auto next = [&s]() { return (s = s * 1664525u + 1013904223u) >> 8; };
  for (int m = 0; m < cap; m++) {
    co[m * 4] = (int)(next() % B);
    co[m * 4 + 1] = (int)(next() % 3) - 1;  // the z index: ignored
    co[m * 4 + 2] = (int)(next() % H);
    co[m * 4 + 3] = (int)(next() % W);
  }
  if (cap > 0) {  // the last pixel of the map, and the word boundaries of a row
    co[0] = B - 1, co[2] = H - 1, co[3] = W - 1;
    if (cap > 2) co[4 + 3] = W > 32 ? 32 : 0, co[8 + 3] = W > 31 ? 31 : W - 1;
  }
  if (stray && cap > 8) {  // rows outside the map on every side, and far outside
    const int32_t bad[6][4] = {{-1, 0, 0, 0}, {B, 0, 0, 0}, {0, 0, -1, 0}, {0, 0, H, 0}, {0, 0, 0, -1}, {0, 0, 0, W}};
    for (int i = 0; i < 6; i++)
      for (int k = 0; k < 4; k++) co[(3 + i) * 4 + k] = bad[i][k];
    co[4] = 0x7FFFFFFF, co[4 + 2] = 0x7FFFFFFF, co[4 + 3] = 0x7FFFFFFF;
    co[8 + 2] = INT32_MIN;
  }
  return co;
}

}  // namespace

int main() {
  const int shapes[4][3] = {{1, 20, 16}, {3, 7, 33}, {2, 5, 65}, {1, 1, 1}};
  int cases = 0;
  for (const auto& sh : shapes)
    for (int cap : {0, 1, 5, 40, 257})
      for (int stray = 0; stray < 2; stray++) {
        const int B = sh[0], H = sh[1], W = sh[2];
        const std::vector<int32_t> co = rows_for(B, H, W, cap, 17u * cap + W, stray != 0);
        for (int n : {INT32_MIN, -1, 0, 1, cap / 2, cap, cap + 1, 0x7FFFFFFF}) {  // the device count: below, at and above the capacity
          Map mp(B, H, W);
          encode(mp, co, n, cap);
          const int live = n < 0 ? 0 : (n > cap ? cap : n);
          if (check(mp, co, live)) return fail("encode", cap, n);
          // a second frame on the same (persistent) planes: clear by the first list, write the second
          const std::vector<int32_t> co2 = rows_for(B, H, W, cap, 99u + cap, false);
          clear(mp, co, n, cap);
          encode(mp, co2, cap, cap);
          if (check(mp, co2, cap)) return fail("clear + encode", cap, n);
          cases++;
        }
      }
  std::printf("pillar_plan_host_shim: %d cases\nok\n", cases);
  return 0;
}
