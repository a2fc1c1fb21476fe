// Host-side compile of vision3d_amd/csrc/pillar_device.h for the DYNAMIC pillar encoder, so that the CPU test-suite can check its
// logic against tests/pillar_dynamic_ref.py without a GPU.  Test infrastructure only.  The loops below are the kernels' (csrc/pillar.hip,
// "dynamic encoder") without the lanes and without the point lists: every pillar's points are found by walking the flat array --
// ascending, or descending with `reverse` (the winner rule must give the same answer in either order).
#include <cstdint>
#include <vector>
#include "../../vision3d_amd/csrc/pillar_device.h"

namespace {

template <int C>
void feature(const float* points, const float* mean, const int32_t* coords, int i, int v, const float* geom, float* f) {
  float centre[3];
  for (int k = 0; k < 3; k++) centre[k] = v3d::pillar_centre(coords[(size_t)v * 4 + 3 - k], geom[k], geom[3 + k]);
  v3d::pillar_feature_row<C>(points + (size_t)i * C, mean + (size_t)v * C, centre, f);
}

template <int C>
void encode(const float* points, const int32_t* pv, int N, const float* mean, const int32_t* coords, int M, const float* geom, const float* W,
            int CH, const float* scale, const float* shift, float* rows, int32_t* winner, int reverse) {
  constexpr int K = C + 6;
  std::vector<float> best((size_t)M * CH, -1.f);
  for (size_t i = 0; i < (size_t)M * CH; i++) winner[i] = -1;
  for (int step = 0; step < N; step++) {
    const int i = reverse ? N - 1 - step : step, v = pv[i];
    if (v < 0 || v >= M) continue;
    float f[K];
    feature<C>(points, mean, coords, i, v, geom, f);
    for (int c = 0; c < CH; c++) {
      float w[1][K];
      for (int k = 0; k < K; k++) w[0][k] = W[(size_t)c * K + k];
      v3d::pillar_offer_point<K, 1>(f, i, w, scale + c, shift + c, &best[(size_t)v * CH + c], &winner[(size_t)v * CH + c]);
    }
  }
  for (size_t i = 0; i < (size_t)M * CH; i++) rows[i] = winner[i] >= 0 ? best[i] : 0.f;
}

// S: K + K (K + 1) / 2 moments, then the number of kept points.
template <int C>
void moments(const float* points, const int32_t* pv, int N, const float* mean, const int32_t* coords, int M, const float* geom, double* S) {
  constexpr int K = C + 6;
  const int nm = v3d::pillar_moments(K);
  for (int i = 0; i <= nm; i++) S[i] = 0.0;
  for (int i = 0; i < N; i++) {
    const int v = pv[i];
    if (v < 0 || v >= M) continue;
    float f[K];
    feature<C>(points, mean, coords, i, v, geom, f);
    v3d::pillar_moments_add<K>(f, S);
    S[nm] += 1.0;
  }
}

template <int C>
void backward(const float* points, const int32_t* pv, int N, const float* mean, const int32_t* coords, int M, const float* geom, const float* W,
              int CH, const float* gamma, float eps, const float* rows, const int32_t* winner, const float* d_rows, const double* S, double* dW,
              double* d_gamma, double* d_beta) {
  constexpr int K = C + 6;
  std::vector<double> G((size_t)CH * (K + 2), 0.0);
  for (int m = 0; m < M; m++) {
    for (int c = 0; c < CH; c++) {
      const size_t at = (size_t)m * CH + c;
      const int win = winner[at];
      if (!(rows[at] > 0.f) || win < 0 || win >= N || pv[win] != m) continue;
      float f[K];
      feature<C>(points, mean, coords, win, m, geom, f);
      const double g = (double)d_rows[at];
      double* Gc = G.data() + (size_t)c * (K + 2);
      Gc[0] += g;
      Gc[1] += g * (double)v3d::pillar_dot<K>(W + (size_t)c * K, f);
      for (int k = 0; k < K; k++) Gc[2 + k] += g * (double)f[k];
    }
  }
  const double n_kept = S[v3d::pillar_moments(K)];
  for (int c = 0; c < CH; c++) {
    const double* Gc = G.data() + (size_t)c * (K + 2);
    v3d::pillar_bwd_channel_counted(K, S, n_kept, W + (size_t)c * K, (double)gamma[c], (double)eps, Gc[0], Gc[1], Gc + 2, dW + (size_t)c * K, d_gamma[c],
                            d_beta[c]);
  }
}

}  // namespace

#define DISPATCH(C_, CALL)           \
  switch (C_) {                      \
    case 3: CALL(3); return 0;       \
    case 4: CALL(4); return 0;       \
    case 5: CALL(5); return 0;       \
    case 6: CALL(6); return 0;       \
    case 7: CALL(7); return 0;       \
    case 8: CALL(8); return 0;       \
    default: return -3;              \
  }

extern "C" int host_pillar_dynamic_encode(const float* points, const int32_t* pv, int N, const float* mean, const int32_t* coords, int M, int C,
                                          const float* geom, const float* W, int CH, const float* scale, const float* shift, float* rows,
                                          int32_t* winner, int reverse) {
#define CALL(N_) encode<N_>(points, pv, N, mean, coords, M, geom, W, CH, scale, shift, rows, winner, reverse)
  DISPATCH(C, CALL)
#undef CALL
}

extern "C" int host_pillar_dynamic_moments(const float* points, const int32_t* pv, int N, const float* mean, const int32_t* coords, int M, int C,
                                           const float* geom, double* S) {
#define CALL(N_) moments<N_>(points, pv, N, mean, coords, M, geom, S)
  DISPATCH(C, CALL)
#undef CALL
}

// mean, var, scale, shift: CH doubles each (the kernel rounds each once to fp32); N = the count behind the moments.
extern "C" void host_pillar_dynamic_bn(int K, const double* S, const float* W, int CH, const float* gamma, const float* beta, float eps,
                                       double* mean, double* var, double* scale, double* shift) {
  const double n_kept = S[v3d::pillar_moments(K)];
  for (int c = 0; c < CH; c++) {
    v3d::pillar_bn_stats(K, S, n_kept, W + (size_t)c * K, mean[c], var[c]);
    v3d::pillar_fold_counted(n_kept, mean[c], var[c], (double)gamma[c], (double)beta[c], (double)eps, scale[c], shift[c]);
  }
}

extern "C" int host_pillar_dynamic_backward(const float* points, const int32_t* pv, int N, const float* mean, const int32_t* coords, int M, int C,
                                            const float* geom, const float* W, int CH, const float* gamma, float eps, const float* rows,
                                            const int32_t* winner, const float* d_rows, const double* S, double* dW, double* d_gamma,
                                            double* d_beta) {
#define CALL(N_) backward<N_>(points, pv, N, mean, coords, M, geom, W, CH, gamma, eps, rows, winner, d_rows, S, dW, d_gamma, d_beta)
  DISPATCH(C, CALL)
#undef CALL
}
