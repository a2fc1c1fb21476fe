// iou_loss_device.h -- rotated 3-D IoU / DIoU loss of ONE aligned pair of (x, y, z, w, l, h, yaw) boxes, z = centre, yaw in
// RADIANS, with its gradient with respect to all 14 numbers.  fp32, one IEEE operation per operator as written.
//
// The geometry is the true one -- that of points-in-boxes (pib_device.h): w lies along u = (cos yaw, sin yaw), l along
// v = (-sin yaw, cos yaw) -- and NOT the reading of rotated_iou.h (radians taken as degrees), which stays what the
// parity operators evaluate.  The definition is this repository's: tests/iou_loss_ref.py restates it in float64 by another
// algorithm, ops/iou_loss.py:iou3d_loss_torch states these very expressions in torch.
//
//   A_bev  = area of the intersection of the two BEV rectangles
//   oh     = max(min(zhi_a, zhi_b) - max(zlo_a, zlo_b), 0);  inter = A_bev * oh;  union = vol_a + vol_b - inter
//   IoU    = inter / union (0 where union <= 0);  term = 1 - IoU  ["iou"]  |  1 - IoU + rho2 / c2  ["diou"]
//   rho2   = squared distance of the centres (3-D), c2 = squared diagonal of the smallest world-aligned cuboid around both boxes
//            (x half-extent (|cos| w + |sin| l) / 2, y half-extent (|sin| w + |cos| l) / 2, z half-extent h / 2); c2 == 0: no penalty
//   bad rows: any of the 14 numbers non-finite, or any size <= 0: IoU = 0, term = 1, zero gradient -- decided BEFORE the clipper.
//            A pair of finite numbers whose arithmetic overflows fp32 on the way (a volume beyond 3.4e38) is given the same result.
//
// Area: rectangle a is clipped by the four half-planes of b (Sutherland-Hodgman); every output edge carries the label of the
// rectangle edge it lies on (0-3: edge of a, 4-7: edge of b), eight 4-bit labels in one register.  A convex polygon gains at most
// one vertex per half-plane: <= 8 vertices, and every store is bounded by 8 whatever the inputs (a NaN distance compares as
// "outside": such a vertex is dropped).  The vertices outside a half-plane are held to one run (il_one_run), which keeps that count
// where edges coincide and rounding decides the signs.  The area is the shoelace sum.
// Gradient: dA / dp = sum over the polygon's edges of length * (n . velocity of the edge's midpoint under p), p a parameter of the
// box that OWNS the edge, n the owner edge's outward normal: (1, 0) / (0, 1) for the centre, half the length for the size the
// edge bounds, length * (m x n) for the yaw (m = midpoint - owner's centre).  The velocity is affine along an edge, so the
// midpoint rule is exact.  At kinks (identical boxes, coincident edges, touching z faces) the result is a finite one-sided value.
//
// The two ping-pong polygons are indexed at run time: as plain locals they would live in scratch (rotated_iou.h:61-65), so the
// algorithm is written against P2View<S>: stride 1 over locals (host build), stride 64 over a per-wave LDS slab (kernels).
#pragma once
#include "rotated_iou.h"

#define V3D_IOU_LOSS_IOU 0
#define V3D_IOU_LOSS_DIOU 1
#define V3D_IOU_LOSS_POLY 8  // vertices of one polygon; a lane's slab holds two

namespace v3d {

V3D_HD bool il_finite(float x) { return fabsf(x) <= 3.4028235e38f; }  // false for NaN and +-Inf

// A convex polygon has ONE run of vertices outside a half-plane.  Where edges coincide (identical boxes, a shared face) the distances
// of the vertices on the boundary are rounding noise of either sign, and their signs can spell several runs -- in, out, in, out --
// each of which would add a vertex, past the eight a polygon may hold (dropped vertices: an IoU of 0.33 for two identical boxes).
// out: bit i = vertex i lies outside; seed: the vertex farthest outside (and every vertex whose distance is NaN).  -> the bits of the
// runs that hold a seed; the vertices of the other runs count as inside.  One run: `out` itself, so no decision of a pair in general
// position changes.
V3D_HD uint32_t il_one_run(uint32_t out, uint32_t seed, int n) {
  const uint32_t full = (1u << n) - 1u;
  uint32_t reach = seed & out;
  for (int k = 1; k < V3D_IOU_LOSS_POLY; k++) {
    const uint32_t up = ((reach << 1) | (reach >> (n - 1))) & full, down = ((reach >> 1) | (reach << (n - 1))) & full;
    reach |= out & (up | down);
  }
  return reach;
}

// Clip polygon `in` (n vertices, labels lab_in: label i = the edge from vertex i to vertex i + 1) by the half-plane
// n . (p - c) <= h whose boundary carries label `own`; -> the vertex count, at most 8.
template <class A>
V3D_HD int il_clip(A in, int n, uint32_t lab_in, A out, uint32_t& lab_out, float nx, float ny, float cx, float cy, float h, uint32_t own) {
  int m = 0;
  uint32_t lo = 0u;
  if (n > V3D_IOU_LOSS_POLY) n = V3D_IOU_LOSS_POLY;
  if (n > 0) {
    uint32_t outside = 0u, seed = 0u;  // a vertex is inside where d <= 0 (NaN: outside)
    float d_far = 0.f;
    int far = -1;
    for (int i = 0; i < n; i++) {
      const P2 p = in[i];
      const float d = (nx * (p.x - cx) + ny * (p.y - cy)) - h;
      if (!(d <= 0.f)) {
        outside |= 1u << i;
        if (d != d) {
          seed |= 1u << i;
        } else if (far < 0 || d > d_far) {
          far = i;
          d_far = d;
        }
      }
    }
    if (far >= 0) seed |= 1u << far;
    outside = il_one_run(outside, seed, n);
    P2 cur = in[0];
    float dc = (nx * (cur.x - cx) + ny * (cur.y - cy)) - h;
    for (int i = 0; i < n; i++) {
      const int i_n = i + 1 < n ? i + 1 : 0;
      const P2 nxt = in[i_n];
      const float dn = (nx * (nxt.x - cx) + ny * (nxt.y - cy)) - h;
      const uint32_t lab = (lab_in >> (4 * i)) & 7u;
      const bool ic = ((outside >> i) & 1u) == 0u, in_n = ((outside >> i_n) & 1u) == 0u;
      if (ic && m < V3D_IOU_LOSS_POLY) {
        out[m] = cur;
        lo |= lab << (4 * m);
        m++;
      }
      if (ic != in_n && m < V3D_IOU_LOSS_POLY) {
        const float t = dc / (dc - dn);
        out[m] = P2{cur.x + t * (nxt.x - cur.x), cur.y + t * (nxt.y - cur.y)};
        lo |= (ic ? own : lab) << (4 * m);  // leaving: the next edge runs along the boundary; entering: the rest of edge `lab`
        m++;
      }
      cur = nxt;
      dc = dn;
    }
  }
  lab_out = lo;
  return m;
}

// One pair.  a, b: 7 floats each; P, Q: views of 8 points each (work space); kind: V3D_IOU_LOSS_*.
// -> term, iou, da[7] = d term / d a, db[7] = d term / d b.
template <class A>
V3D_HD void iou3d_loss_pair(const float* a, const float* b, int kind, A P, A Q, float& term, float& iou, float (&da)[7], float (&db)[7]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    ok = ok && il_finite(a[k]) && il_finite(b[k]);
    da[k] = 0.f;
    db[k] = 0.f;
  }
  ok = ok && a[3] > 0.f && a[4] > 0.f && a[5] > 0.f && b[3] > 0.f && b[4] > 0.f && b[5] > 0.f;
  term = 1.f;
  iou = 0.f;
  if (!ok) return;

  // ---- BEV: everything relative to a's centre
  const float ca = cosf(a[6]), sa = sinf(a[6]), cb = cosf(b[6]), sb = sinf(b[6]);
  const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  const float hwa = a[3] * 0.5f, hla = a[4] * 0.5f, hwb = b[3] * 0.5f, hlb = b[4] * 0.5f;
  const float wx = hwa * ca, wy = hwa * sa, lx = -(hla * sa), ly = hla * ca;  // half-size vectors of a
  P[0] = P2{-wx - lx, -wy - ly};  // counter-clockwise: edge 0 on the -v face, 1 on +u, 2 on +v, 3 on -u
  P[1] = P2{wx - lx, wy - ly};
  P[2] = P2{wx + lx, wy + ly};
  P[3] = P2{lx - wx, ly - wy};
  uint32_t lab = 0x3210u, lab2;
  int n = 4;
  n = il_clip(P, n, lab, Q, lab2, sb, -cb, dx, dy, hlb, 4u);   // b's edge 0: outward normal -v_b
  n = il_clip(Q, n, lab2, P, lab, cb, sb, dx, dy, hwb, 5u);    // 1: +u_b
  n = il_clip(P, n, lab, Q, lab2, -sb, cb, dx, dy, hlb, 6u);   // 2: +v_b
  n = il_clip(Q, n, lab2, P, lab, -cb, -sb, dx, dy, hwb, 7u);  // 3: -u_b

  float area = 0.f;
  float gax = 0.f, gay = 0.f, gaw = 0.f, gal = 0.f, gat = 0.f, gbx = 0.f, gby = 0.f, gbw = 0.f, gbl = 0.f, gbt = 0.f;  // dA / d(x, y, w, l, yaw)
  if (n >= 3) {
    float twice = 0.f;
    P2 p = P[0];
    for (int i = 0; i < n; i++) {
      const P2 q = P[i + 1 < n ? i + 1 : 0];
      twice += p.x * q.y - q.x * p.y;
      const float ex = q.x - p.x, ey = q.y - p.y;
      const float len = sqrtf(ex * ex + ey * ey);
      const uint32_t e = (lab >> (4 * i)) & 7u;
      const bool of_b = e >= 4u, odd = (e & 1u) != 0u, pos = (e & 3u) == 1u || (e & 3u) == 2u;
      const float ux = of_b ? cb : ca, uy = of_b ? sb : sa;
      float nx = odd ? ux : -uy, ny = odd ? uy : ux;  // +u or +v of the owner
      nx = pos ? nx : -nx;
      ny = pos ? ny : -ny;
      const float mx = 0.5f * (p.x + q.x) - (of_b ? dx : 0.f), my = 0.5f * (p.y + q.y) - (of_b ? dy : 0.f);
      const float gx = len * nx, gy = len * ny, gh = 0.5f * len, gt = len * (mx * ny - my * nx);
      gax += of_b ? 0.f : gx;
      gay += of_b ? 0.f : gy;
      gaw += of_b || !odd ? 0.f : gh;
      gal += of_b || odd ? 0.f : gh;
      gat += of_b ? 0.f : gt;
      gbx += of_b ? gx : 0.f;
      gby += of_b ? gy : 0.f;
      gbw += of_b && odd ? gh : 0.f;
      gbl += of_b && !odd ? gh : 0.f;
      gbt += of_b ? gt : 0.f;
      p = q;
    }
    area = fmaxf(0.5f * twice, 0.f);
  }

  // ---- z overlap, volumes, IoU
  const float hza = a[5] * 0.5f, hzb = b[5] * 0.5f;
  const float top = fminf(hza, dz + hzb), bot = fmaxf(-hza, dz - hzb);
  const float oh = fmaxf(top - bot, 0.f);
  const bool live = oh > 0.f, top_a = hza < dz + hzb, bot_a = -hza > dz - hzb;  // which box owns the overlap's faces
  const float ta = live && top_a ? 1.f : 0.f, tb = live && !top_a ? 1.f : 0.f;
  const float ba = live && bot_a ? 1.f : 0.f, bb = live && !bot_a ? 1.f : 0.f;
  const float inter = area * oh;
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  const float uni = va + vb - inter;
  float t_da[7], t_db[7];
#pragma unroll
  for (int k = 0; k < 7; k++) t_da[k] = t_db[k] = 0.f;
  float val = 1.f, r_iou = 0.f;
  if (uni > 0.f) {
    r_iou = inter / uni;
    val = 1.f - r_iou;
    // d inter and d vol per parameter; d IoU = ((union + inter) d inter - inter d vol) / union^2
    const float di_a[7] = {oh * gax, oh * gay, area * (ta - ba), oh * gaw, oh * gal, area * (0.5f * (ta + ba)), oh * gat};
    const float di_b[7] = {oh * gbx, oh * gby, area * (tb - bb), oh * gbw, oh * gbl, area * (0.5f * (tb + bb)), oh * gbt};
    const float dv_a[7] = {0.f, 0.f, 0.f, a[4] * a[5], a[3] * a[5], a[3] * a[4], 0.f};
    const float dv_b[7] = {0.f, 0.f, 0.f, b[4] * b[5], b[3] * b[5], b[3] * b[4], 0.f};
    const float ui = uni + inter, u2 = uni * uni;
#pragma unroll
    for (int k = 0; k < 7; k++) {
      t_da[k] = -((ui * di_a[k] - inter * dv_a[k]) / u2);
      t_db[k] = -((ui * di_b[k] - inter * dv_b[k]) / u2);
    }
  }

  if (kind == V3D_IOU_LOSS_DIOU) {
    const float aca = fabsf(ca), asa = fabsf(sa), acb = fabsf(cb), asb = fabsf(sb);
    const float hxa = (aca * a[3] + asa * a[4]) * 0.5f, hya = (asa * a[3] + aca * a[4]) * 0.5f;
    const float hxb = (acb * b[3] + asb * b[4]) * 0.5f, hyb = (asb * b[3] + acb * b[4]) * 0.5f;
    const float rho2 = dx * dx + dy * dy + dz * dz;
    const bool xhi_a = hxa >= dx + hxb, xlo_a = -hxa <= dx - hxb, yhi_a = hya >= dy + hyb, ylo_a = -hya <= dy - hyb;
    const bool zhi_a = hza >= dz + hzb, zlo_a = -hza <= dz - hzb;
    const float ex = fmaxf(hxa, dx + hxb) - fminf(-hxa, dx - hxb);
    const float ey = fmaxf(hya, dy + hyb) - fminf(-hya, dy - hyb);
    const float ez = fmaxf(hza, dz + hzb) - fminf(-hza, dz - hzb);
    const float c2 = ex * ex + ey * ey + ez * ez;
    if (c2 > 0.f) {
      const float pen = rho2 / c2;
      val += pen;
      // extent = hi - lo: d / d centre = [owns hi] - [owns lo], d / d half-extent = [owns hi] + [owns lo]
      const float cxa = (xhi_a ? 1.f : 0.f) - (xlo_a ? 1.f : 0.f), cxb = (xhi_a ? 0.f : 1.f) - (xlo_a ? 0.f : 1.f);
      const float cya = (yhi_a ? 1.f : 0.f) - (ylo_a ? 1.f : 0.f), cyb = (yhi_a ? 0.f : 1.f) - (ylo_a ? 0.f : 1.f);
      const float cza = (zhi_a ? 1.f : 0.f) - (zlo_a ? 1.f : 0.f), czb = (zhi_a ? 0.f : 1.f) - (zlo_a ? 0.f : 1.f);
      const float sxa = (xhi_a ? 1.f : 0.f) + (xlo_a ? 1.f : 0.f), sxb = (xhi_a ? 0.f : 1.f) + (xlo_a ? 0.f : 1.f);
      const float sya = (yhi_a ? 1.f : 0.f) + (ylo_a ? 1.f : 0.f), syb = (yhi_a ? 0.f : 1.f) + (ylo_a ? 0.f : 1.f);
      const float sza = (zhi_a ? 1.f : 0.f) + (zlo_a ? 1.f : 0.f), szb = (zhi_a ? 0.f : 1.f) + (zlo_a ? 0.f : 1.f);
      // d |cos| / d yaw = -sign(cos) sin, d |sin| / d yaw = sign(sin) cos
      const float dca = ca >= 0.f ? -sa : sa, dsa = sa >= 0.f ? ca : -ca, dcb = cb >= 0.f ? -sb : sb, dsb = sb >= 0.f ? cb : -cb;
      const float hxa_t = (dca * a[3] + dsa * a[4]) * 0.5f, hya_t = (dsa * a[3] + dca * a[4]) * 0.5f;
      const float hxb_t = (dcb * b[3] + dsb * b[4]) * 0.5f, hyb_t = (dsb * b[3] + dcb * b[4]) * 0.5f;
      // half of d c2 per parameter: ex d ex + ey d ey + ez d ez
      const float hc_a[7] = {ex * cxa, ey * cya, ez * cza, ex * (sxa * (0.5f * aca)) + ey * (sya * (0.5f * asa)),
                             ex * (sxa * (0.5f * asa)) + ey * (sya * (0.5f * aca)), ez * (sza * 0.5f), ex * (sxa * hxa_t) + ey * (sya * hya_t)};
      const float hc_b[7] = {ex * cxb, ey * cyb, ez * czb, ex * (sxb * (0.5f * acb)) + ey * (syb * (0.5f * asb)),
                             ex * (sxb * (0.5f * asb)) + ey * (syb * (0.5f * acb)), ez * (szb * 0.5f), ex * (sxb * hxb_t) + ey * (syb * hyb_t)};
      const float hr_b[7] = {dx, dy, dz, 0.f, 0.f, 0.f, 0.f};  // half of d rho2 / d b; that of a is its negative
#pragma unroll
      for (int k = 0; k < 7; k++) {
        t_da[k] += (2.f * (-hr_b[k] - pen * hc_a[k])) / c2;
        t_db[k] += (2.f * (hr_b[k] - pen * hc_b[k])) / c2;
      }
    }
  }

  bool fin = il_finite(val) && il_finite(r_iou);
#pragma unroll
  for (int k = 0; k < 7; k++) fin = fin && il_finite(t_da[k]) && il_finite(t_db[k]);
  if (!fin) return;  // fp32 overflow of finite inputs: the bad-row result
  term = val;
  iou = r_iou;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    da[k] = t_da[k];
    db[k] = t_db[k];
  }
}

// The pair with its polygons as plain locals (host build; on the device: scratch).
V3D_HD void iou3d_loss_pair_local(const float* a, const float* b, int kind, float& term, float& iou, float (&da)[7], float (&db)[7]) {
  P2 p[V3D_IOU_LOSS_POLY], q[V3D_IOU_LOSS_POLY];
  iou3d_loss_pair(a, b, kind, P2View<1>{p}, P2View<1>{q}, term, iou, da, db);
}

// The pair with its polygons in a per-wave LDS slab of 2 * 8 * 64 points: `slab` = the wave's slab + this lane's index.
V3D_HD void iou3d_loss_pair_lds(const float* a, const float* b, int kind, P2* slab, float& term, float& iou, float (&da)[7], float (&db)[7]) {
  iou3d_loss_pair(a, b, kind, P2View<64>{slab}, P2View<64>{slab + V3D_IOU_LOSS_POLY * 64}, term, iou, da, db);
}

}  // namespace v3d
