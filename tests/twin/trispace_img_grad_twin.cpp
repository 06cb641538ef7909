// trispace_img_grad_twin.cpp -- TEST-ONLY host twin of the fused polynomial model's image gradient.
//
// Compiles curl_amd/csrc/curl_math_poly.h (the header the gfx950 kernels include) for the host and loops its per-pixel
// function over host arrays as kernels/trispace_img_grad.inc does on the device: the image's table staged once
// (trispace_img_grad_stage), then trispace_img_grad_n per pixel with the pixel's own coordinates.  The product never loads
// this.  With -DTWIN_MAIN it is a stand-alone program (for a sanitizer build): both forms, both flags, on a small
// pseudo-random image with the colours of the discontinuities in its first row; exit status 0 when every value is finite.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../curl_amd/csrc/curl_math_poly.h"

using namespace curlm;

template <int V>
static void img_grad(const float* img, const float* coeffs, const float* gout, float* gimg, int B, int H, int W, bool residual_only) {
  constexpr int NC = PolyEval<V>::kCoeffs, NL = TriImgGrad<V>::kFloats;
  const size_t HW = (size_t)H * W;
  const float fW = (float)W, fH = (float)H, rW = 1.0f / fW, rH = 1.0f / fH;
  std::vector<float> tab(NL);
  for (int b = 0; b < B; ++b) {
    for (int j = 0; j < NL; ++j) tab[j] = trispace_img_grad_stage<V>(coeffs + (size_t)b * 9 * NC, j);
    const float* pi = img + (size_t)b * 3 * HW;
    const float* pg = gout + (size_t)b * 3 * HW;
    float* q = gimg + (size_t)b * 3 * HW;
    for (int row = 0; row < H; ++row)
      for (int col = 0; col < W; ++col) {
        const size_t i = (size_t)row * W + col;
        const PxN<1> in{{pi[i]}, {pi[HW + i]}, {pi[2 * HW + i]}}, g{{pg[i]}, {pg[HW + i]}, {pg[2 * HW + i]}};
        const float xw[1] = {V == 5 ? div_small((float)col, fW, rW) : 0.0f}, yh[1] = {V == 5 ? div_small((float)row, fH, rH) : 0.0f};
        PxN<1> r;
        trispace_img_grad_n<V, 1>(in, xw, yh, tab.data(), g, residual_only, r);
        q[i] = r.c0[0], q[HW + i] = r.c1[0], q[2 * HW + i] = r.c2[0];
      }
  }
}

extern "C" {

// grad_img [B,3,H,W] of the fused model; num_coeffs 126 or 35
int twin_trispace_img_grad(const float* img, const float* coeffs, const float* gout, float* gimg, int B, int H, int W,
                           int num_coeffs, int residual_only) {
  if (num_coeffs == 126) img_grad<5>(img, coeffs, gout, gimg, B, H, W, residual_only != 0);
  else if (num_coeffs == 35) img_grad<3>(img, coeffs, gout, gimg, B, H, W, residual_only != 0);
  else return -1;
  return 0;
}

}  // extern "C"

#ifdef TWIN_MAIN
int main() {
  const int B = 2, H = 9, W = 13;
  const size_t HW = (size_t)H * W;
  uint32_t state = 12345u;
  auto unit = [&]() { return (float)((state = state * 1664525u + 1013904223u) >> 8) * (1.0f / 16777216.0f); };
  std::vector<float> img(B * 3 * HW), gout(B * 3 * HW), gimg(B * 3 * HW);
  for (auto& v : img) v = unit();
  for (auto& v : gout) v = 2.0f * unit() - 1.0f;
  const float first_row[6][3] = {{0, 0, 0}, {1, 1, 1}, {0.5f, 0.5f, 0.5f}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 6; ++k)
      for (int c = 0; c < 3; ++c) img[((size_t)b * 3 + c) * HW + k] = first_row[k][c];
  int bad = 0;
  for (int nc : {126, 35})
    for (int ro = 0; ro < 2; ++ro) {
      std::vector<float> coeffs((size_t)B * 9 * nc);
      for (auto& v : coeffs) v = 0.6f * unit() - 0.3f;
      if (twin_trispace_img_grad(img.data(), coeffs.data(), gout.data(), gimg.data(), B, H, W, nc, ro)) return 2;
      double sum = 0.0;
      for (float v : gimg) bad += !std::isfinite(v), sum += v;
      printf("num_coeffs %d residual_only %d: sum %.9g\n", nc, ro, sum);
    }
  return bad ? 1 : 0;
}
#endif
