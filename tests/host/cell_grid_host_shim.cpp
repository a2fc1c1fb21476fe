// Host-side compile of vision3d_amd/csrc/cell_grid_device.h (the grid-shape rule and the cell coordinate of the cell grids) so that
// the CPU test-suite can check them without a GPU.  Test infrastructure only.
#include "../../vision3d_amd/csrc/cell_grid_device.h"

// bounds (n, 4) = xlo, xhi, ylo, yhi; -> header_f (n, 3) = x0, y0, inv_c; header_i (n, 4) = nx, ny, nch, chunk; steps (n)
extern "C" void host_cg_shape(const float* bounds, const float* cell_min, const int* N, const int* max_chunks, int n, float* header_f,
                              int* header_i, int* steps) {
  for (int i = 0; i < n; i++) {
    const float* b = bounds + 4 * (size_t)i;
    const CgHeader h = cg_shape(b[0], b[1], b[2], b[3], cell_min[i], N[i], max_chunks[i], steps + i);
    header_f[3 * (size_t)i] = h.x0, header_f[3 * (size_t)i + 1] = h.y0, header_f[3 * (size_t)i + 2] = h.inv_c;
    header_i[4 * (size_t)i] = h.nx, header_i[4 * (size_t)i + 1] = h.ny, header_i[4 * (size_t)i + 2] = h.nch, header_i[4 * (size_t)i + 3] = h.chunk;
  }
}

extern "C" void host_cg_cell(const float* x, const float* x0, const float* inv_c, int n, float* out) {
  for (int i = 0; i < n; i++) out[i] = cg_cell(x[i], x0[i], inv_c[i]);
}

extern "C" int host_cg_constants(int which) {
  return which == 0 ? CG_MAX_KEYS : which == 1 ? CG_SHAPE_STEPS : which == 2 ? CG_HEADER_BYTES : (int)cg_record_offset();
}
