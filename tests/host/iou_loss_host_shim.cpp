// Host-side compile of vision3d_amd/csrc/iou_loss_device.h (the DEVICE pair function of the rotated 3-D IoU loss) so that the CPU
// test-suite can check its logic against tests/iou_loss_ref.py without a GPU.  Test infrastructure only.
#include <cstddef>
#include "../../vision3d_amd/csrc/iou_loss_device.h"

// a, b: (n, 7); term, iou: (n); da, db: (n, 7).  Polygons as plain locals (stride 1).
extern "C" void host_iou3d_loss(const float* a, const float* b, int n, int kind, float* term, float* iou, float* da, float* db) {
  for (int i = 0; i < n; i++) {
    float ga[7], gb[7];
    v3d::iou3d_loss_pair_local(a + 7 * (size_t)i, b + 7 * (size_t)i, kind, term[i], iou[i], ga, gb);
    for (int k = 0; k < 7; k++) {
      da[7 * (size_t)i + k] = ga[k];
      db[7 * (size_t)i + k] = gb[k];
    }
  }
}

// The same pairs through the STRIDED form the kernels use (element e of "lane" L at [e * 64 + L], the per-wave LDS slab of the
// device): 64 pairs share one slab, exactly as 64 lanes do.  Must equal the plain form bit for bit.
extern "C" void host_iou3d_loss_strided(const float* a, const float* b, int n, int kind, float* term, float* iou, float* da, float* db) {
  static v3d::P2 slab[2 * V3D_IOU_LOSS_POLY * 64];
  for (int i = 0; i < n; i++) {
    float ga[7], gb[7];
    v3d::iou3d_loss_pair_lds(a + 7 * (size_t)i, b + 7 * (size_t)i, kind, slab + (i & 63), term[i], iou[i], ga, gb);
    for (int k = 0; k < 7; k++) {
      da[7 * (size_t)i + k] = ga[k];
      db[7 * (size_t)i + k] = gb[k];
    }
  }
}
