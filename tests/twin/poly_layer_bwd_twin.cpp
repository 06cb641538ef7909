// poly_layer_bwd_twin.cpp -- TEST-ONLY host twin of the stand-alone polynomial layer's backward.
//
// Compiles curl_amd/csrc/curl_math_poly.h (the header the gfx950 kernels include) for the host and loops its two pieces over
// host arrays, as kernels/poly_layer_bwd.inc does on the device: the per-pixel image gradient (poly_deriv_stage +
// poly_img_grad_n) and the per-tile coefficient accumulation (coef_grad_accumulate, a lane's groups of 4 pixels in the
// kernel's order; the 256 lane sums of a tile added in float32, the tile rows in float64).  The product never loads this.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../curl_amd/csrc/curl_math_poly.h"

using namespace curlm;

template <int V>
static void img_grad(const float* img, const float* coeffs, const float* gout, float* gimg, int B, long HW) {
  constexpr int NC = PolyEval<V>::kCoeffs, ND = 3 * V * PolyDeriv<V>::kTerms;
  for (int b = 0; b < B; ++b) {
    float D[ND];
    for (int j = 0; j < ND; ++j) D[j] = poly_deriv_stage<V>(coeffs + (size_t)b * 3 * NC, j);
    for (long i = 0; i < HW; ++i) {
      float vars[V][1], g[3][1], r[V][1];
      for (int k = 0; k < V; ++k) vars[k][0] = img[((size_t)b * V + k) * HW + i];
      for (int o = 0; o < 3; ++o) g[o][0] = gout[((size_t)b * 3 + o) * HW + i];
      poly_img_grad_n<V, 1>(r, vars, g, D);
      for (int k = 0; k < V; ++k) gimg[((size_t)b * V + k) * HW + i] = r[k][0];
    }
  }
}

template <int V, int C>
static void coef_tile_chunk(const float* pv, const float* pg, long HW, long tile, int steps, float* row) {
  constexpr int NC = PolyEval<V>::kCoeffs, T = PolyEval<V>::kChunk, NPAIR = (T + 1) / 2;
  const long groups = (HW + 3) / 4;
  float sum[3][T] = {};
  for (int lane = 0; lane < 256; ++lane) {
    grad_pair acc[3][NPAIR] = {};
    for (int k = 0; k < steps; ++k) {
      const long grp = (tile * steps + k) * 256 + lane;
      for (int e = 0; e < 4; ++e) {
        const long px = 4 * grp + e;
        const bool live = grp < groups && px < HW;
        const long at = px < HW ? px : HW - 1;
        float v[V], g[3];
        for (int c = 0; c < V; ++c) v[c] = pv[(size_t)c * HW + at];
        for (int o = 0; o < 3; ++o) g[o] = live ? pg[(size_t)o * HW + at] : 0.0f;
        coef_grad_accumulate<V, C>(acc, v, g);
      }
    }
    for (int o = 0; o < 3; ++o)
      for (int j = 0; j < T; ++j) sum[o][j] += grad_pair_get(acc[o], j);
  }
  for (int o = 0; o < 3; ++o)
    for (int j = 0; j < T; ++j)
      if (C * T + j < NC) row[o * NC + C * T + j] = sum[o][j];
}

template <int V>
static void coef_grad(const float* img, const float* gout, float* gcoef, int B, long HW, int steps) {
  constexpr int NC = PolyEval<V>::kCoeffs;
  const long per = 1024L * steps, tiles = (HW + per - 1) / per;
  std::vector<float> row(3 * NC);
  for (int b = 0; b < B; ++b) {
    std::vector<double> total(3 * NC, 0.0);
    for (long t = 0; t < tiles; ++t) {
      const float* pv = img + (size_t)b * V * HW;
      const float* pg = gout + (size_t)b * 3 * HW;
      coef_tile_chunk<V, 0>(pv, pg, HW, t, steps, row.data());
      if constexpr (PolyEval<V>::kChunks > 1) {
        coef_tile_chunk<V, 1>(pv, pg, HW, t, steps, row.data());
        coef_tile_chunk<V, 2>(pv, pg, HW, t, steps, row.data());
      }
      for (int k = 0; k < 3 * NC; ++k) total[k] += (double)row[k];
    }
    for (int k = 0; k < 3 * NC; ++k) gcoef[(size_t)b * 3 * NC + k] = (float)total[k];
  }
}

extern "C" {

// grad_img [B,V,H*W] of the layer, per pixel
int twin_poly_layer_img_grad(const float* img, const float* coeffs, const float* gout, float* gimg, int B, long HW, int V) {
  if (V == 5) img_grad<5>(img, coeffs, gout, gimg, B, HW);
  else if (V == 3) img_grad<3>(img, coeffs, gout, gimg, B, HW);
  else return -1;
  return 0;
}

// grad_coeffs [B,3,NC] of the layer, tiles of 1024 * steps pixels
int twin_poly_layer_coef_grad(const float* img, const float* gout, float* gcoef, int B, long HW, int V, int steps) {
  if (V == 5) coef_grad<5>(img, gout, gcoef, B, HW, steps);
  else if (V == 3) coef_grad<3>(img, gout, gcoef, B, HW, steps);
  else return -1;
  return 0;
}

// the generated derivative tables, for the table test: idx, mul [V][kTerms]
int twin_poly_deriv_tables(int V, int* idx, int* mul) {
  if (V == 5) {
    for (int i = 0; i < 5; ++i)
      for (int u = 0; u < 56; ++u) idx[i * 56 + u] = PolyDeriv<5>::src(i, u), mul[i * 56 + u] = (int)PolyDeriv<5>::mul(i, u);
    return 56;
  }
  if (V == 3) {
    for (int i = 0; i < 3; ++i)
      for (int u = 0; u < 20; ++u) idx[i * 20 + u] = PolyDeriv<3>::src(i, u), mul[i * 20 + u] = (int)PolyDeriv<3>::mul(i, u);
    return 20;
  }
  return -1;
}

}  // extern "C"
