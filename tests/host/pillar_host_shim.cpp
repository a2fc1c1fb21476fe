// Host-side compile of vision3d_amd/csrc/pillar_device.h (the per-pillar arithmetic of the pillar feature encoder) so that the CPU
// test-suite can check its logic against tests/pillar_ref.py without a GPU.  Test infrastructure only.  The loops below are the
// kernels' (csrc/pillar.hip) without the lanes: one pillar at a time, rows in order, channels one by one.
#include <cstdint>
#include <vector>
#include "../../vision3d_amd/csrc/pillar_device.h"

namespace {

// The n feature rows of pillar m into f (n, K); -> n.
template <int C>
int stage(const float* feat, const int32_t* occ, const int32_t* coords, int m, int P, const float* geom, float* f) {
  constexpr int K = C + 6;
  const int n = occ[m] < 0 ? 0 : (occ[m] > P ? P : occ[m]);
  if (n == 0) return 0;
  const float* pts = feat + (size_t)m * P * C;
  float mean[3], centre[3];
  v3d::pillar_mean(pts, C, n, mean);
  for (int k = 0; k < 3; k++) centre[k] = v3d::pillar_centre(coords[(size_t)m * 4 + 3 - k], geom[k], geom[3 + k]);
  for (int p = 0; p < n; p++) v3d::pillar_feature_row<C>(pts + (size_t)p * C, mean, centre, f + (size_t)p * K);
  return n;
}

template <int C>
void encode(const float* feat, const int32_t* occ, const int32_t* coords, int M, int P, const float* geom, const float* W, int CH,
            const float* scale, const float* shift, float* rows, int32_t* winner) {
  constexpr int K = C + 6;
  std::vector<float> f((size_t)P * K);
  for (int m = 0; m < M; m++) {
    const int n = stage<C>(feat, occ, coords, m, P, geom, f.data());
    for (int c = 0; c < CH; c++) {
      float w[1][K], best = -1.f;
      int win = -1;
      for (int k = 0; k < K; k++) w[0][k] = W[(size_t)c * K + k];
      for (int p = 0; p < n; p++) v3d::pillar_offer_row<K, 1>(f.data() + (size_t)p * K, p, w, scale + c, shift + c, &best, &win);
      if (n < P) v3d::pillar_offer(v3d::pillar_activation(0.f, scale[c], shift[c]), -1, best, win);
      rows[(size_t)m * CH + c] = best;
      winner[(size_t)m * CH + c] = win;
    }
  }
}

template <int C>
void moments(const float* feat, const int32_t* occ, const int32_t* coords, int M, int P, const float* geom, double* S) {
  constexpr int K = C + 6;
  std::vector<float> f((size_t)P * K);
  for (int i = 0; i < v3d::pillar_moments(K); i++) S[i] = 0.0;
  for (int m = 0; m < M; m++) {
    const int n = stage<C>(feat, occ, coords, m, P, geom, f.data());
    for (int p = 0; p < n; p++) v3d::pillar_moments_add<K>(f.data() + (size_t)p * K, S);
  }
}

template <int C>
void backward(const float* feat, const int32_t* occ, const int32_t* coords, int M, int P, const float* geom, const float* W, int CH,
              const float* gamma, float eps, const float* rows, const int32_t* winner, const float* d_rows, const double* S, double* dW,
              double* d_gamma, double* d_beta) {
  constexpr int K = C + 6;
  std::vector<float> f((size_t)P * K);
  std::vector<double> G((size_t)CH * (K + 2), 0.0);
  for (int m = 0; m < M; m++) {
    const int n = stage<C>(feat, occ, coords, m, P, geom, f.data());
    for (int c = 0; c < CH; c++) {
      const size_t at = (size_t)m * CH + c;
      const int win = winner[at];
      const double g = rows[at] > 0.f && win >= -1 && win < n ? (double)d_rows[at] : 0.0;
      double* Gc = G.data() + (size_t)c * (K + 2);
      Gc[0] += g;
      if (win >= 0 && win < n) {
        const float* fr = f.data() + (size_t)win * K;
        Gc[1] += g * (double)v3d::pillar_dot<K>(W + (size_t)c * K, fr);
        for (int k = 0; k < K; k++) Gc[2 + k] += g * (double)fr[k];
      }
    }
  }
  for (int c = 0; c < CH; c++) {
    const double* Gc = G.data() + (size_t)c * (K + 2);
    v3d::pillar_bwd_channel(K, S, (double)M * (double)P, W + (size_t)c * K, (double)gamma[c], (double)eps, Gc[0], Gc[1], Gc + 2,
                            dW + (size_t)c * K, d_gamma[c], d_beta[c]);
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

extern "C" int host_pillar_encode(const float* feat, const int32_t* occ, const int32_t* coords, int M, int P, int C, const float* geom,
                                  const float* W, int CH, const float* scale, const float* shift, float* rows, int32_t* winner) {
#define CALL(N) encode<N>(feat, occ, coords, M, P, geom, W, CH, scale, shift, rows, winner)
  DISPATCH(C, CALL)
#undef CALL
}

extern "C" int host_pillar_moments(const float* feat, const int32_t* occ, const int32_t* coords, int M, int P, int C, const float* geom,
                                   double* S) {
#define CALL(N) moments<N>(feat, occ, coords, M, P, geom, S)
  DISPATCH(C, CALL)
#undef CALL
}

// mean, var, scale, shift: CH doubles each (the kernel rounds each once to fp32).
extern "C" void host_pillar_bn(int K, const double* S, double N, const float* W, int CH, const float* gamma, const float* beta, float eps,
                               double* mean, double* var, double* scale, double* shift) {
  for (int c = 0; c < CH; c++) {
    v3d::pillar_bn_stats(K, S, N, W + (size_t)c * K, mean[c], var[c]);
    v3d::pillar_fold(mean[c], var[c], (double)gamma[c], (double)beta[c], (double)eps, scale[c], shift[c]);
  }
}

extern "C" int host_pillar_backward(const float* feat, const int32_t* occ, const int32_t* coords, int M, int P, int C, const float* geom,
                                    const float* W, int CH, const float* gamma, float eps, const float* rows, const int32_t* winner,
                                    const float* d_rows, const double* S, double* dW, double* d_gamma, double* d_beta) {
#define CALL(N) backward<N>(feat, occ, coords, M, P, geom, W, CH, gamma, eps, rows, winner, d_rows, S, dW, d_gamma, d_beta)
  DISPATCH(C, CALL)
#undef CALL
}
