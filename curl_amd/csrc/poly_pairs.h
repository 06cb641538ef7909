// poly_pairs.h -- the polynomial family in numbers.  Plain C++: the kernels' header (curl_math_poly.h), the host side of the C
// ABI (kernels/host_api.inc) and the compiled binding (fastcall.cpp) all read the counts from here.
#pragma once

constexpr int poly_binomial(int n, int k) {  // C(n, k)
  int c = 1;
  for (int i = 1; i <= k; ++i) c = c * (n - k + i) / i;
  return c;
}
// coefficients of one polynomial of total degree <= D in V variables: one per monomial
constexpr int poly_count(int V, int D) { return poly_binomial(V + D, D); }

// The public (variables, order) pairs: the spatial (5) and the non-spatial (3) model and layer at orders 4..1.  Their counts --
// 126, 56, 21, 6 and 35, 20, 10, 4 -- are all different, so a count names its pair.
struct PolyPair {
  int V, D;
};
constexpr PolyPair kPolyPairs[8] = {{5, 4}, {5, 3}, {5, 2}, {5, 1}, {3, 4}, {3, 3}, {3, 2}, {3, 1}};
constexpr bool is_poly_pair(int V, int D) {
  for (const PolyPair& p : kPolyPairs)
    if (p.V == V && p.D == D) return true;
  return false;
}
constexpr bool is_poly_count(int count, int D) {  // `count` is the count of a public pair of order D
  for (const PolyPair& p : kPolyPairs)
    if (p.D == D && poly_count(p.V, p.D) == count) return true;
  return false;
}
