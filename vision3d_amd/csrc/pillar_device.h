// pillar_device.h -- the per-pillar arithmetic of the pillar feature encoder (PointPillars, arXiv 1812.05784; opt-in, cfg.PILLAR):
// ONE statement of the feature row, the dot product, the activation, the winner rule, the input moments and the closed forms that
// turn those moments into the BatchNorm statistics and its backward.  pillar.hip runs it on the GPU, tests/host/pillar_host_shim.cpp
// compiles the same text with g++; detector/pillar.py:forward_torch states it in torch, tests/pillar_ref.py in float64.
//
// A pillar m holds P point slots of C channels (x, y, z first), n = occupancy of them real.  With K = C + 6:
//   mean   = (row 0 + row 1 + ... + row n-1 of xyz, in that order) / n
//   centre = idx * v + o per axis, o = v / 2 + lower bound (one fp32 number, made by the caller)
//   f(p)   = [point's C channels | xyz - mean | xyz - centre] for p < n, all zero for p >= n
//   y      = w[0] * f[0], then fmaf(w[k], f[k], y) for k = 1 .. K-1
//   a      = max(fmaf(y, scale, shift), 0)          (BatchNorm folded to scale / shift, then ReLU)
//   out    = max over the P rows of a; the padded rows all have a = max(shift, 0)
// Winner rule: candidates are taken in the order row 0 .. n-1, padded; a candidate replaces the best only when strictly greater, so
// the lowest real row wins a tie and the padded candidate (winner -1) wins only when strictly above every real row.
// fp32, one IEEE operation per operator as written (-ffp-contract=off; fmaf where it says fmaf).
//
// Moments (double): S[k] = sum over all real rows of f[k]; S[K + i (i + 1) / 2 + j] = sum of f[i] * f[j], j <= i.  The padded rows add
// nothing but count in N = M * P.  y is linear in f, so over the N rows  mean_y = w . S1 / N  and  var_y = w' Cov w  with
// Cov[i][j] = S2[i][j] / N - (S1[i] / N)(S1[j] / N): the batch statistics of every channel without a pass over the pre-activations.
// Backward: d_rows reaches one row per (pillar, channel), the winner -- g = d_rows where out > 0, else 0.  With G0 = sum g,
// Gy = sum g * y(winner), Gf[k] = sum g * f(winner)[k] (a padded winner has f = 0, y = 0) and s = 1 / sqrt(var + eps):
//   d_beta = G0;  d_gamma = s (Gy - mean_y G0)
//   dW[k]  = gamma s (Gf[k] - d_beta / N * S1[k] - d_gamma / N * s (sum_i S2[k][i] w[i] - mean_y S1[k]))
// -- the "all rows" sums of the BatchNorm gradient are closed forms in the same moments.
//
// The DYNAMIC encoder (DynamicPillarVFE of MVF, arXiv 1910.06528; opt-in, cfg.PILLAR.DYNAMIC) -- every point of a pillar counts.  The
// pillars are those of the dynamic voxelizer: points (N, C) flat, point_voxel (N) the row of every point (outside [0, M): dropped),
// voxel_mean (M, C), occupancy (M) the true counts (>= 1), coordinates (M, 4).  Per kept point i of pillar v:
//   f = [point | xyz - voxel_mean[v, :3] | xyz - centre(v)],  y = pillar_dot(W_c, f),  a = pillar_activation(y, scale, shift)
//   rows[v][c] = max of a over the pillar's points; there is no padded candidate (every pillar has a point)
// winner[v][c] = the FLAT index of the point that reaches the maximum, the lowest among equals (pillar_offer_lowest): the result does
// not depend on the order in which a pillar's points are visited.  Training: the moments run over the kept points only, N = N_kept =
// their number (= sum of occupancy), known on the device alone -- it travels as one more double behind the moments; pillar_bn_stats,
// pillar_fold_counted and pillar_bwd_channel_counted take it as their N.  One kept point is legal: variance 0, rows = relu(beta)
// exactly, gradient to beta alone (stated by the two _counted forms).  tests/host/pillar_dynamic_host_shim.cpp compiles this text with g++, detector/pillar.py
// (DynamicPillarFeatureNet.forward_torch) states it in torch, tests/pillar_dynamic_ref.py in float64.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define V3D_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define V3D_HD inline
#endif

#define V3D_PILLAR_MAX_P 64
#define V3D_PILLAR_MIN_C 3
#define V3D_PILLAR_MAX_C 8
#define V3D_PILLAR_MAX_K (V3D_PILLAR_MAX_C + 6)
#define V3D_PILLAR_MAX_MOMENTS (V3D_PILLAR_MAX_K + V3D_PILLAR_MAX_K * (V3D_PILLAR_MAX_K + 1) / 2)

namespace v3d {

struct PillarGeom {  // per axis (x, y, z): cell size and v / 2 + lower bound, fp32
  float v[3], o[3];
};

V3D_HD int pillar_moments(int K) { return K + K * (K + 1) / 2; }
V3D_HD int pillar_s2(int K, int i, int j) { return i >= j ? K + i * (i + 1) / 2 + j : K + j * (j + 1) / 2 + i; }

V3D_HD float pillar_centre(int idx, float v, float o) { return (float)idx * v + o; }

// xyz of the rows at xyz[p * ld + 0..2]; n >= 1.
V3D_HD void pillar_mean(const float* xyz, int ld, int n, float* mean) {
  float s0 = xyz[0], s1 = xyz[1], s2 = xyz[2];
  for (int p = 1; p < n; p++) {
    s0 += xyz[p * ld];
    s1 += xyz[p * ld + 1];
    s2 += xyz[p * ld + 2];
  }
  const float d = (float)n;
  mean[0] = s0 / d;
  mean[1] = s1 / d;
  mean[2] = s2 / d;
}

template <int C>
V3D_HD void pillar_feature_row(const float* pt, const float* mean, const float* centre, float* f) {
#pragma unroll
  for (int k = 0; k < C; k++) f[k] = pt[k];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    f[C + k] = pt[k] - mean[k];
    f[C + 3 + k] = pt[k] - centre[k];
  }
}

template <int K>
V3D_HD float pillar_dot(const float* w, const float* f) {
  float y = w[0] * f[0];
#pragma unroll
  for (int k = 1; k < K; k++) y = fmaf(w[k], f[k], y);
  return y;
}

V3D_HD float pillar_activation(float y, float scale, float shift) {
  const float z = fmaf(y, scale, shift);
  return z > 0.f ? z : 0.f;
}

// The winner rule.  Start from best = -1 (below every activation), win = -1; offer row 0 .. n-1 with their index, then, where n < P,
// the padded candidate with index -1.
V3D_HD void pillar_offer(float a, int index, float& best, int& win) {
  if (a > best) {
    best = a;
    win = index;
  }
}

// The winner rule of the DYNAMIC encoder (below): candidates carry the flat index of their point and arrive in any order; a candidate
// replaces the best when strictly greater, or equal with a lower index -- the lowest index that reaches the maximum wins whatever the
// order.  Start from best = -1, win = -1 (the first real candidate is strictly greater); a NaN activation never wins.
V3D_HD void pillar_offer_lowest(float a, int index, float& best, int& win) {
  if (a > best || (a == best && index < win)) {
    best = a;
    win = index;
  }
}

// One point of the dynamic encoder (flat index i) offered to the NCH channels a lane owns.
template <int K, int NCH>
V3D_HD void pillar_offer_point(const float* f, int i, const float (*w)[K], const float* scale, const float* shift, float* best, int* win) {
#pragma unroll
  for (int j = 0; j < NCH; j++) pillar_offer_lowest(pillar_activation(pillar_dot<K>(w[j], f), scale[j], shift[j]), i, best[j], win[j]);
}

// One real row offered to the NCH channels a lane owns (w[j]: the K weights of its j-th channel).
template <int K, int NCH>
V3D_HD void pillar_offer_row(const float* f, int p, const float (*w)[K], const float* scale, const float* shift, float* best, int* win) {
#pragma unroll
  for (int j = 0; j < NCH; j++) pillar_offer(pillar_activation(pillar_dot<K>(w[j], f), scale[j], shift[j]), p, best[j], win[j]);
}

template <int K>
V3D_HD void pillar_moments_add(const float* f, double* S) {
#pragma unroll
  for (int i = 0; i < K; i++) {
    S[i] += (double)f[i];
#pragma unroll
    for (int j = 0; j <= i; j++) S[K + i * (i + 1) / 2 + j] += (double)f[i] * (double)f[j];
  }
}

// Batch statistics of y = w . f over N rows from the moments: mean and BIASED variance, double.  Cov is symmetric: the K means are
// divided once, every pair (i, j < i) is visited once and counted twice -- K + K (K + 1) / 2 divisions, all of them in this function.
V3D_HD void pillar_bn_stats(int K, const double* S, double N, const float* w, double& mean, double& var) {
  double mu[V3D_PILLAR_MAX_K];
  double m = 0.0, v = 0.0;
  for (int i = 0; i < K; i++) {
    mu[i] = S[i] / N;
    m += (double)w[i] * mu[i];
  }
  for (int i = 0; i < K; i++) {
    const double wi = (double)w[i];
    v += wi * wi * (S[K + i * (i + 1) / 2 + i] / N - mu[i] * mu[i]);
    for (int j = 0; j < i; j++) v += 2.0 * (wi * (double)w[j]) * (S[K + i * (i + 1) / 2 + j] / N - mu[i] * mu[j]);
  }
  mean = m;
  var = v > 0.0 ? v : 0.0;
}

// Eval / training fold: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (double, rounded once by the caller).
V3D_HD void pillar_fold(double mean, double var, double gamma, double beta, double eps, double& scale, double& shift) {
  scale = gamma / sqrt(var + eps);
  shift = beta - mean * scale;
}

// The fold of the dynamic encoder's training forward, where N is counted on the device and may be 1.  With ONE row the batch mean of
// every channel is that row's y and the variance is 0 by construction, so (y - mean) is zero whatever y: the normalised value is
// beta exactly.  The general fold would compute that zero as fp32 y minus a double mean times 1 / sqrt(eps) -- about 30 times the
// rounding of y -- so the one-row batch states its result instead: scale = 0, shift = beta, a = relu(beta).
V3D_HD void pillar_fold_counted(double N, double mean, double var, double gamma, double beta, double eps, double& scale, double& shift) {
  if (N == 1.0) {
    scale = 0.0;
    shift = beta;
  } else {
    pillar_fold(mean, var, gamma, beta, eps, scale, shift);
  }
}

// The backward of one channel from its winner sums (header comment); dW: K doubles.
V3D_HD void pillar_bwd_channel(int K, const double* S, double N, const float* w, double gamma, double eps, double G0, double Gy,
                               const double* Gf, double* dW, double& d_gamma, double& d_beta) {
  double mean, var;
  pillar_bn_stats(K, S, N, w, mean, var);
  const double s = 1.0 / sqrt(var + eps);
  d_beta = G0;
  d_gamma = s * (Gy - mean * G0);
  const double b_n = d_beta / N, g_n = d_gamma / N;
  for (int k = 0; k < K; k++) {
    double s2w = 0.0;
    for (int i = 0; i < K; i++) s2w += S[pillar_s2(K, k, i)] * (double)w[i];
    const double xf = s * (s2w - mean * S[k]);  // sum over all rows of xhat * f[k]
    dW[k] = gamma * s * (Gf[k] - b_n * S[k] - g_n * xf);
  }
}

// ... of the dynamic encoder (N counted on the device).  One row: the output is relu(beta) whatever W and gamma (pillar_fold_counted),
// so the gradient reaches beta alone -- stated, not left to the cancellation of the closed forms.
V3D_HD void pillar_bwd_channel_counted(int K, const double* S, double N, const float* w, double gamma, double eps, double G0, double Gy,
                                       const double* Gf, double* dW, double& d_gamma, double& d_beta) {
  if (N == 1.0) {
    for (int k = 0; k < K; k++) dW[k] = 0.0;
    d_gamma = 0.0;
    d_beta = G0;
  } else {
    pillar_bwd_channel(K, S, N, w, gamma, eps, G0, Gy, Gf, dW, d_gamma, d_beta);
  }
}

}  // namespace v3d
