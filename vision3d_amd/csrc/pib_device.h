// pib_device.h -- the point-in-rotated-box test shared by points_in_boxes_kernel (iou_nms.hip) and the fused augmentation
// (augment.hip): vision3d/core/geometry.py:4-65.  Corner arithmetic in fp64 exactly where numpy promotes (geometry.py:21);
// cos / sin evaluated on the float32 yaw.  Compiled with -ffp-contract=off like every geometry kernel.
// The sample-database extraction (database.hip) tests against float64 annotation boxes: same corners-in-double test, z limits
// in double as well (PibBoxD), corners from host-evaluated cos / sin (pib_prep_row).
#pragma once
#include <math.h>

template <typename Z>
struct PibBoxT {
  double cx[4], cy[4];
  Z zlo, zhi;  // the z comparison runs in Z: float32 boxes compare in float32, float64 boxes in float64 (geometry.py:33-38)
};
typedef PibBoxT<float> PibBox;
typedef PibBoxT<double> PibBoxD;

// bx = (x, y, z, w, l, h, yaw), float32
__device__ __forceinline__ PibBox pib_prep(const float* bx) {
  const float cf = cosf(bx[6]), sf = sinf(bx[6]);
  const double ux[4] = {-0.5, 0.5, 0.5, -0.5}, uy[4] = {-0.5, -0.5, 0.5, 0.5};
  PibBox pb;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const double lx = (double)bx[3] * ux[v], ly = (double)bx[4] * uy[v];
    pb.cx[v] = ((double)cf * lx + (double)(-sf) * ly) + (double)bx[0];
    pb.cy[v] = ((double)sf * lx + (double)cf * ly) + (double)bx[1];
  }
  pb.zlo = bx[2] - bx[5] / 2;
  pb.zhi = bx[2] + bx[5] / 2;
  return pb;
}

// row = (cos yaw, sin yaw, x, y, w, l, zlo, zhi), float64: the yaw's cos / sin and the z limits evaluated by the caller (numpy, in the
// dtype of its boxes), the corners built here with the multiplies and adds of pib_prep
__device__ __forceinline__ PibBoxD pib_prep_row(const double* row) {
  const double c = row[0], s = row[1];
  const double ux[4] = {-0.5, 0.5, 0.5, -0.5}, uy[4] = {-0.5, -0.5, 0.5, 0.5};
  PibBoxD pb;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const double lx = row[4] * ux[v], ly = row[5] * uy[v];
    pb.cx[v] = (c * lx + (-s) * ly) + row[2];
    pb.cy[v] = (s * lx + c * ly) + row[3];
  }
  pb.zlo = row[6];
  pb.zhi = row[7];
  return pb;
}

template <typename Z>
__device__ __forceinline__ bool pib_inside(const PibBoxT<Z>& pb, float px, float py, float pz, bool use_z) {
  bool in = true;
  if (use_z) in = ((Z)pz > pb.zlo) && ((Z)pz < pb.zhi);
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int pv = (v + 3) & 3;
    const double sx = -(pb.cx[v] - pb.cx[pv]), sy = -(pb.cy[v] - pb.cy[pv]);
    const double vx = pb.cx[v] - (double)px, vy = pb.cy[v] - (double)py;
    in = in && (sx * vy - sy * vx > 0);
  }
  return in;
}
