// cell_grid_device.h -- a frame's points binned into square (x, y) cells: the ONE statement of the frame layout, of the cell
// coordinate and of the grid's shape.  cell_grid.hip builds such a frame (one workgroup per frame); the ball query over the grid
// (pointops.hip) and the VectorPool search (vector_pool.hip) walk it with a wave per query.
//
// A frame of N points in the workspace:
//   [0, CG_HEADER_BYTES)              CgHeader
//   [CG_HEADER_BYTES, ...)            cell_start[CG_MAX_KEYS + 1]: the first record of key (index chunk * ny + cell y) * nx + cell x;
//                                     entry nkeys = nx * ny * nch holds the number of binned points
//   [cg_record_offset(), ...)         N records float4 (x, y, z, index bits), sorted by key; points with a non-finite x or y are
//                                     left out
//
// Host-compilable (V3D_HD as in rotated_iou.h): tests/host/cell_grid_host_shim.cpp checks the shape rule and the cell coordinate
// with g++ on the text the device compiles.  Must be compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define V3D_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define V3D_HD inline
#endif

#define CG_MAX_KEYS 32768  // (index chunk, cell) keys of the LDS histogram: 128 KB of the build workgroup's LDS
#define CG_HEADER_BYTES 32
// Steps of the shape rule at most.  The cell grows by 1.5 per step, and from the smallest positive float to beyond the largest
// is log(2^277) / log(1.5) = 474 steps: the rule has bailed out on a cell that is no longer finite before the bound is reached
// (and at once on a cell that would never grow: 0, negative, NaN).
#define CG_SHAPE_STEPS 512

struct CgHeader {  // first words of a frame's workspace, written by the build kernel
  float x0, y0, inv_c;     // inv_c == 0: nothing was gridded (see cg_cell)
  int nx, ny, nch, chunk;  // cells along x / y, index chunks, points per chunk
};

V3D_HD size_t cg_record_offset() { return (CG_HEADER_BYTES + (CG_MAX_KEYS + 1) * 4 + 15) / 16 * 16; }
V3D_HD size_t cg_frame_bytes(int N) { return cg_record_offset() + (size_t)N * 16; }

// Cell coordinate of x along an axis that starts at x0: the SAME expression for the binned points and for the queries.  Two values
// less than r apart, in cells of at least 1.01 r, differ by less than r * inv_c <= 1 / 1.01 before rounding and by at most
// 2 * 32768 * 2^-23 ~ 0.008 more after it (two roundings each, at most CG_MAX_KEYS cells along an axis): their floors differ by at
// most one.  inv_c == 0 marks the single cell of an extent that could not be gridded: every value is in cell 0 ((x - x0) * inv_c
// may be inf * 0 there, and a NaN must not become an index).
V3D_HD float cg_cell(float x, float x0, float inv_c) { return inv_c == 0.f ? 0.f : floorf((x - x0) * inv_c); }

// The grid over the bounds [xlo, xhi] x [ylo, yhi] of a frame's finite points: cells no smaller than cell_min, grown by 1.5 until
// (cells along x) * (cells along y) fits CG_MAX_KEYS; the keys left over go to index chunks, max_chunks at most (records are sorted
// by (index / chunk, cell): a search that wants the lowest indices walks the chunks in order and can stop early; max_chunks = 1: by
// cell alone).  xlo > xhi (no finite point): no cells, nx = ny = 0.  An extent no finite cell can grid (xhi - xlo overflows), or a
// cell_min that never grows: ONE cell, nx = ny = nch = 1 and inv_c = 0 -- every query of the frame walks every record, slow and
// correct, since the cells only have to be a superset.  At most CG_SHAPE_STEPS steps; *steps (nullable) receives their number.
V3D_HD CgHeader cg_shape(float xlo, float xhi, float ylo, float yhi, float cell_min, int N, int max_chunks, int* steps = nullptr) {
  CgHeader t;
  t.x0 = xlo, t.y0 = ylo, t.inv_c = 0.f, t.nx = 0, t.ny = 0, t.nch = 1, t.chunk = N > 0 ? N : 1;
  int step = 0;
  if (xlo <= xhi) {  // at least one finite point
    t.nx = t.ny = 1;
    float c = cell_min;
    for (; step < CG_SHAPE_STEPS && c > 0.f && c < HUGE_VALF; step++, c *= 1.5f) {  // (a cell that is positive and finite)
      const float inv_c = 1.f / c;
      const float fx = cg_cell(xhi, xlo, inv_c), fy = cg_cell(yhi, ylo, inv_c);  // (the largest cell along each axis)
      if (fx < (float)CG_MAX_KEYS && fy < (float)CG_MAX_KEYS && ((long long)fx + 1) * ((long long)fy + 1) <= CG_MAX_KEYS) {
        t.inv_c = inv_c, t.nx = (int)fx + 1, t.ny = (int)fy + 1;
        const int left = CG_MAX_KEYS / (t.nx * t.ny);
        t.nch = max_chunks < left ? max_chunks : left;
        t.chunk = (N + t.nch - 1) / t.nch;
        break;
      }
    }
  }
  if (steps) *steps = step;
  return t;
}
