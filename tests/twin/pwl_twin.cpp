// pwl_twin.cpp -- TEST-ONLY host twin of the fused layer's backward with the paper's piecewise-linear curves.
//
// Compiles curl_amd/csrc/curl_math_bwd.h (the header layer_pwl_bwd.inc's kernels include) for the host and loops its per-pixel
// pullback (curl_layer_pwl_bwd) and the per-curve chain rule (knot_bwd_pwl) over host arrays, with the {knot, slope} table the
// kernels stage.  tests/test_twin_pwl_bwd.py checks it against float64 autograd through a PWL restatement of the layer.
// The product never loads this library.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../curl_amd/csrc/curl_math_bwd.h"

using namespace curlm;

namespace {
// every curve's sums in float64: T[c][0] = sum G, T[c][1 + j] = sum G clamp01(s - j)
struct HostAcc {
  std::vector<double>* T;
  const int* K;
  void operator()(int c, float s, float G) {
    std::vector<double>& t = T[c];
    t[0] += (double)G;
    for (int j = 0; j + 1 < K[c]; ++j) t[1 + j] += (double)(G * clamp01(s - (float)j));
  }
};
}  // namespace

extern "C" {

// img, gout, gimg, fwd [B,3,HW]; mask [B,HW] or NULL (binary: the mask is 0/1); raw [B, 3 Kl + 3 Kr + 4 Kh] (L, R, H back to
// back); greg [B] or NULL; graw like raw.  fwd: the forward output the pullback recomputed.
int twin_layer_pwl_bwd(const float* img, const float* mask, int binary, const float* raw, const float* gout, const float* greg,
                       float* gimg, float* graw, float* fwd, int B, long HW, int Kl, int Kr, int Kh) {
  const int n = 3 * Kl + 3 * Kr + 4 * Kh;
  int K[10], off[10];
  for (int c = 0, o = 0; c < 10; ++c) K[c] = c < 3 ? Kl : c < 6 ? Kr : Kh, off[c] = o, o += K[c];
  std::vector<float> C(n), tab(2 * n);
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < n; ++t) C[t] = (float)std::exp((double)raw[(size_t)b * n + t]);
    for (int c = 0; c < 10; ++c)
      for (int j = 0; j < K[c]; ++j) {
        const int t = off[c] + j;
        tab[2 * t] = C[t];
        tab[2 * t + 1] = j + 1 < K[c] ? C[t + 1] - C[t] : 0.0f;  // OpLayerTab::stage_value
      }
    std::vector<double> T[10];
    for (int c = 0; c < 10; ++c) T[c].assign(K[c], 0.0);
    HostAcc acc{T, K};
    for (long i = 0; i < HW; ++i) {
      const float* p = img + (size_t)b * 3 * HW + i;
      const float* g = gout + (size_t)b * 3 * HW + i;
      const float m = mask ? mask[(size_t)b * HW + i] : 1.0f;
      const Px in{p[0], p[HW], p[2 * HW]}, go{g[0], g[HW], g[2 * HW]};
      Px y;
      const Px gi = binary ? curl_layer_pwl_bwd<true, true>(in, m, tab.data(), Kl, Kr, Kh, go, acc, y)
                           : curl_layer_pwl_bwd<false, true>(in, m, tab.data(), Kl, Kr, Kh, go, acc, y);
      float* q = gimg + (size_t)b * 3 * HW + i;
      q[0] = gi.c0, q[HW] = gi.c1, q[2 * HW] = gi.c2;
      float* f = fwd + (size_t)b * 3 * HW + i;
      f[0] = y.c0, f[HW] = y.c1, f[2 * HW] = y.c2;
    }
    const double gr = greg ? (double)greg[b] : 0.0;
    for (int c = 0; c < 10; ++c)
      for (int kk = 0; kk < K[c]; ++kk)
        graw[(size_t)b * n + off[c] + kk] = knot_bwd_pwl(C.data() + off[c], K[c], T[c].data(), gr, kk);
  }
  return 0;
}

}  // extern "C"
