// poly_orders_twin.cpp -- TEST-ONLY host twin of the polynomial forward at every order.
//
// Compiles curl_amd/csrc/curl_math_poly.h (the header the gfx950 kernels include) for the host and evaluates the three output
// polynomials of ChannelPolyLayer(degree, V, 3) per pixel with the generated Horner scheme of that degree (PolyEval<V, D>),
// from the reference-order table as poly3_n's SEQ = false form and from the consumption-order table staged as the kernels
// stage it in LDS (SEQ = true).  Also hands out the generated consumption-order tables.  The product never loads this.
#include <cstddef>
#include <vector>

#include "../../curl_amd/csrc/curl_math_poly.h"

using namespace curlm;

template <int V, int D>
static void layer(const float* img, const float* coeffs, float* out, int B, long HW, int seq) {
  constexpr int NC = PolyEval<V, D>::kCoeffs, NS = PolyEval<V, D>::kSeqStride;
  for (int b = 0; b < B; ++b) {
    const float* table = coeffs + (size_t)b * 3 * NC;
    float staged[3 * NS];
    for (int j = 0; j < 3 * NS; ++j) staged[j] = table[poly_seq_index<V, D>(j)];  // the kernels' own staging rule
    for (long i = 0; i < HW; ++i) {
      float v[V][1], o[3][1];
      for (int k = 0; k < V; ++k) v[k][0] = img[((size_t)b * V + k) * HW + i];
      if (seq) poly3_n<V, 1, true, D>(o, v, staged);
      else poly3_n<V, 1, false, D>(o, v, table);
      for (int c = 0; c < 3; ++c) out[((size_t)b * 3 + c) * HW + i] = o[c][0];
    }
  }
}

template <int V, int D>
static int order_table(int* out) {
  for (int p = 0; p < PolyEval<V, D>::kCoeffs; ++p) out[p] = PolyEval<V, D>::order(p);
  return PolyEval<V, D>::kCoeffs;
}

#define EACH_ORDER(V, D, CALL)        \
  if (V == 5 && D == 4) return CALL(5, 4); \
  if (V == 5 && D == 3) return CALL(5, 3); \
  if (V == 5 && D == 2) return CALL(5, 2); \
  if (V == 5 && D == 1) return CALL(5, 1); \
  if (V == 3 && D == 4) return CALL(3, 4); \
  if (V == 3 && D == 3) return CALL(3, 3); \
  if (V == 3 && D == 2) return CALL(3, 2); \
  if (V == 3 && D == 1) return CALL(3, 1);

extern "C" {

// out [B,3,HW] = the degree-`degree` polynomials of img [B,V,HW] under coeffs [B,3,C(V + degree, degree)]; 0, or -1 for a
// (V, degree) without a scheme
int twin_poly_order_layer(const float* img, const float* coeffs, float* out, int B, long HW, int V, int degree, int seq) {
#define LAYER(V_, D_) (layer<V_, D_>(img, coeffs, out, B, HW, seq), 0)
  EACH_ORDER(V, degree, LAYER)
#undef LAYER
  return -1;
}

// table[pos] = the reference index of the coefficient the scheme consumes pos-th; returns the count, or -1
int twin_poly_order_table(int V, int degree, int* table) {
#define TABLE(V_, D_) order_table<V_, D_>(table)
  EACH_ORDER(V, degree, TABLE)
#undef TABLE
  return -1;
}

// the padded stride of one polynomial in the staged (LDS) layout: a multiple of 4 floats
int twin_poly_order_stride(int V, int degree) {
#define STRIDE(V_, D_) PolyEval<V_, D_>::kSeqStride
  EACH_ORDER(V, degree, STRIDE)
#undef STRIDE
  return -1;
}
}
