// stage_twin.cpp -- TEST-ONLY host twin of the stand-alone curve ops', converters' and stages' backward.
//
// Compiles curl_amd/csrc/curl_math_bwd.h (the header stage_bwd.inc's kernels include) for the host and loops its per-pixel
// stage functions (adjust3_bwd, adjust_hsv_bwd, lab_stage_bwd, hsv_stage_bwd, the converters' *_bwd) and the per-curve chain
// rule (knots_bwd) over host arrays.  tests/test_twin_stage_bwd.py checks it against float64 autograd through the oracle.
// twin_layer_uneven: the fused layer with a shorter last curve per segment (tests/test_knot_paths.py).
// The product never loads this library.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../curl_amd/csrc/curl_math_bwd.h"

using namespace curlm;

// exp'd knots and collapsed curves of one image's segment; torch.chunk: the last curve holds K_last knots
static void prep_segment(const float* raw, int ncurves, int K, int K_last, Affine* k, float* knots) {
  for (int c = 0; c < ncurves; ++c) {
    const int Kc = c == ncurves - 1 ? K_last : K;
    float* C = knots + c * K;
    for (int j = 0; j < Kc; ++j) C[j] = (float)std::exp((double)raw[c * K + j]);
    float r;
    collapse_curve(C, Kc, k[c].a, k[c].b, r);
  }
}

extern "C" {

// op: 0 adjust_rgb / adjust_lab, 1 adjust_hsv, 2 the Lab stage, 3 the HSV stage.  mask: NULL = none; binary: the mask is 0/1.
int twin_stage_bwd(int op, const float* img, const float* mask, int binary, const float* raw, const float* gout,
                   const float* greg, float* gimg, float* graw, int B, long HW, int K, int K_last) {
  const int nc = (op == 1 || op == 3) ? 4 : 3, n_all = (nc - 1) * K + K_last;
  std::vector<float> knots(n_all);
  for (int b = 0; b < B; ++b) {
    Affine k[4];
    prep_segment(raw + (size_t)b * n_all, nc, K, K_last, k, knots.data());
    double P[4] = {0, 0, 0, 0}, Q[4] = {0, 0, 0, 0};
    for (long i = 0; i < HW; ++i) {
      const float* p = img + (size_t)b * 3 * HW + i;
      const float* g = gout + (size_t)b * 3 * HW + i;
      const float m = mask ? mask[(size_t)b * HW + i] : 1.0f;
      const Px in{p[0], p[HW], p[2 * HW]}, go{g[0], g[HW], g[2 * HW]};
      float Pf[4] = {0, 0, 0, 0}, Qf[4] = {0, 0, 0, 0};
      Px gi;
      if (op == 0) gi = adjust3_bwd(in, k, go, Pf, Qf);
      else if (op == 1) gi = adjust_hsv_bwd(in, k, go, Pf, Qf);
      else if (op == 2) gi = binary ? lab_stage_bwd<true>(in, m, k, go, Pf, Qf) : lab_stage_bwd<false>(in, m, k, go, Pf, Qf);
      else gi = binary ? hsv_stage_bwd<true>(in, m, k, go, Pf, Qf) : hsv_stage_bwd<false>(in, m, k, go, Pf, Qf);
      for (int c = 0; c < nc; ++c) P[c] += Pf[c], Q[c] += Qf[c];
      float* q = gimg + (size_t)b * 3 * HW + i;
      q[0] = gi.c0, q[HW] = gi.c1, q[2 * HW] = gi.c2;
    }
    const double gr = greg ? (double)greg[b] : 0.0;
    for (int c = 0; c < nc; ++c)
      knots_bwd(knots.data() + c * K, c == nc - 1 ? K_last : K, P[c], Q[c], gr, graw + (size_t)b * n_all + c * K);
  }
  return 0;
}

// The fused layer, forward (gout == NULL: out, reg) or backward (gimg, gL, gR, gH), as curl_twin.cpp's twin_layer(1, ...) and
// twin_layer_bwd, with torch.chunk's uneven splits: segment s (L, R, H) has K[s] knots per curve, K_last[s] in its last one.
int twin_layer_uneven(const float* img, const float* mask, int binary, const float* rawL, const float* rawR, const float* rawH,
                      const float* gout, const float* greg, float* out, float* reg, float* gimg, float* gL, float* gR, float* gH,
                      int B, long HW, const int* K, const int* K_last) {
  const float* raw[3] = {rawL, rawR, rawH};
  float* graw[3] = {gL, gR, gH};
  const int nc[3] = {3, 3, 4}, first[3] = {0, 3, 6};
  int n[3];
  std::vector<float> knots[3];
  for (int s = 0; s < 3; ++s) n[s] = (nc[s] - 1) * K[s] + K_last[s], knots[s].resize(n[s]);
  for (int b = 0; b < B; ++b) {
    LayerCoef k;
    Affine* seg[3] = {k.lab, k.rgb, k.hsv};
    float seg_reg[3];
    for (int s = 0; s < 3; ++s) {
      seg_reg[s] = 0.0f;
      for (int c = 0; c < nc[s]; ++c) {
        const int Kc = c == nc[s] - 1 ? K_last[s] : K[s];
        float* C = knots[s].data() + c * K[s];
        for (int j = 0; j < Kc; ++j) C[j] = (float)std::exp((double)raw[s][(size_t)b * n[s] + c * K[s] + j]);
        float r;
        collapse_curve(C, Kc, seg[s][c].a, seg[s][c].b, r);
        seg_reg[s] += r;
      }
    }
    if (!gout) reg[b] = (seg_reg[0] + seg_reg[1]) + seg_reg[2];
    double P[10] = {0}, Q[10] = {0};
    for (long i = 0; i < HW; ++i) {
      const float* p = img + (size_t)b * 3 * HW + i;
      const float m = mask ? mask[(size_t)b * HW + i] : 1.0f;
      const Px x{p[0], p[HW], p[2 * HW]};
      Px y;
      if (!gout) {
        if (binary && m == 0.0f) y = Px{0.0f, 0.0f, 0.0f};
        else y = binary ? curl_layer<true>(x, m, k) : curl_layer<false>(x, m, k);
      } else {
        const float* g = gout + (size_t)b * 3 * HW + i;
        const Px go{g[0], g[HW], g[2 * HW]};
        float Pf[10] = {0}, Qf[10] = {0};
        y = binary ? curl_layer_bwd<true>(x, m, k, go, Pf, Qf) : curl_layer_bwd<false>(x, m, k, go, Pf, Qf);
        for (int c = 0; c < 10; ++c) P[c] += Pf[c], Q[c] += Qf[c];
      }
      float* q = (gout ? gimg : out) + (size_t)b * 3 * HW + i;
      q[0] = y.c0, q[HW] = y.c1, q[2 * HW] = y.c2;
    }
    if (!gout) continue;
    const double gr = greg ? (double)greg[b] : 0.0;
    for (int s = 0; s < 3; ++s)
      for (int c = 0; c < nc[s]; ++c)
        knots_bwd(knots[s].data() + c * K[s], c == nc[s] - 1 ? K_last[s] : K[s], P[first[s] + c], Q[first[s] + c], gr,
                  graw[s] + (size_t)b * n[s] + c * K[s]);
  }
  return 0;
}

// op: 0 rgb2lab, 1 lab2rgb, 2 rgb2hsv, 3 hsv2rgb
int twin_convert_bwd(int op, const float* in, const float* gout, float* gin, int B, long HW) {
  for (int b = 0; b < B; ++b)
    for (long i = 0; i < HW; ++i) {
      const float* p = in + (size_t)b * 3 * HW + i;
      const float* g = gout + (size_t)b * 3 * HW + i;
      const Px x{p[0], p[HW], p[2 * HW]}, go{g[0], g[HW], g[2 * HW]};
      const Px gi = op == 0 ? rgb2lab_bwd(x, go) : op == 1 ? lab2rgb_bwd(x, go) : op == 2 ? rgb2hsv_bwd(x, go) : hsv2rgb_bwd(x, go);
      float* q = gin + (size_t)b * 3 * HW + i;
      q[0] = gi.c0, q[HW] = gi.c1, q[2 * HW] = gi.c2;
    }
  return 0;
}

}  // extern "C"
