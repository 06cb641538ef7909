// trispace_img_grad.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// image gradient of the fused polynomial model: d loss / d img of curl_trispace_fwd_f32 (autograd of model.py:499-520 w.r.t.
// the image; arithmetic: curl_math_poly.h trispace_img_grad_n; DESIGN.md 3a)
// ------------------------------------------------------------------------------------------------
// One per-pixel pass: reads img and grad_out (6 planes), writes grad_img (3 planes).  No scratch buffer, no atomics, no second
// pass -- the result is a function of the pixel alone (and of its coordinates), so it is bit-reproducible and does not depend
// on the batch or on which instantiation ran.  The image's 9 forward and 27 derivative polynomials sit in LDS in Horner
// consumption order (trispace_img_grad_stage); a workgroup stages them once and walks kTriImgGradSteps groups of 256 lanes,
// a lane owning VEC pixels per group (float4 per plane, or one pixel of any size or alignment): a tile of
// 256 * VEC * kTriImgGradSteps pixels per table.  n = HW / VEC.
constexpr unsigned kTriImgGradSteps = 4;
constexpr int kTriImgGradLock = 2;  // pixels in lock step through the polynomials (4: 198 VGPRs and 544 B of scratch per lane)
// pixels H .. H + N - 1 of a lane's VEC, N in lock step; then the rest (a recursion, not a loop: every index a constant)
template <int V, int VEC, int H, class T>
__device__ __forceinline__ void tri_img_grad_part(float (&r)[3][VEC], const T (&x)[3], const T (&w)[3], unsigned row, unsigned col,
                                                  unsigned W, float fW, float fH, float rW, float rH, const float* tab,
                                                  bool residual_only) {
  constexpr int N = VEC < kTriImgGradLock ? VEC : kTriImgGradLock;
  if constexpr (H < VEC) {
    PxN<N> in, g, o;
    float xw[N], yh[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
      in.c0[e] = lane(x[0], H + e), in.c1[e] = lane(x[1], H + e), in.c2[e] = lane(x[2], H + e);
      g.c0[e] = lane(w[0], H + e), g.c1[e] = lane(w[1], H + e), g.c2[e] = lane(w[2], H + e);
      xw[e] = yh[e] = 0.0f;
      if constexpr (V == 5) {  // cat_coords (model.py:487-497): column / width, row / height of each pixel
        xw[e] = div_small((float)col, fW, rW), yh[e] = div_small((float)row, fH, rH);
        if (++col == W) col = 0, ++row;
      }
    }
    CURL_FENCE();
    trispace_img_grad_n<V, N>(in, xw, yh, tab, g, residual_only, o);
    CURL_FENCE();
#pragma unroll
    for (int e = 0; e < N; ++e) r[0][H + e] = o.c0[e], r[1][H + e] = o.c1[e], r[2][H + e] = o.c2[e];
    tri_img_grad_part<V, VEC, H + N>(r, x, w, row, col, W, fW, fH, rW, rH, tab, residual_only);
  }
}
template <int V, int VEC>
__global__ __launch_bounds__(256, 2) void trispace_img_grad_kernel(const float* img, const float* coeffs, const float* gout,
                                                                   float* gin, unsigned n, unsigned W, float fW, float fH,
                                                                   int residual_only) {
  typedef typename Pack<VEC>::T T;
  constexpr int NC = PolyEval<V>::kCoeffs, NL = TriImgGrad<V>::kFloats;
  __shared__ __attribute__((aligned(16))) float s_tab[NL];
  const unsigned b = blockIdx.y;
  const size_t plane = (size_t)n;
  const T* pi = reinterpret_cast<const T*>(img) + (size_t)b * 3 * plane;
  const T* pg = reinterpret_cast<const T*>(gout) + (size_t)b * 3 * plane;
  T* q = reinterpret_cast<T*>(gin) + (size_t)b * 3 * plane;
  unsigned i = blockIdx.x * (256u * kTriImgGradSteps) + threadIdx.x;
  T x[3], w[3];
  auto fetch = [&](unsigned at) {  // clamped: always a valid group; lanes past the end store nothing
    const unsigned c = min(at, n - 1u);
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = ld<true>(pi + (size_t)k * plane + c), w[k] = ld<true>(pg + (size_t)k * plane + c);
  };
  fetch(i);  // before the staging barrier
  const float* table = coeffs + (size_t)b * 9 * NC;
  for (int j = threadIdx.x; j < NL; j += 256) s_tab[j] = trispace_img_grad_stage<V>(table, j);
  __syncthreads();
  const float rW = 1.0f / fW, rH = 1.0f / fH;
#pragma unroll 1
  for (unsigned k = 0; k < kTriImgGradSteps; ++k) {
    if (i >= n) return;  // (no barrier below)
    float r[3][VEC];
    unsigned row = 0, col = 0;
    if constexpr (V == 5) row = (i * VEC) / W, col = i * VEC - row * W;
    tri_img_grad_part<V, VEC, 0>(r, x, w, row, col, W, fW, fH, rW, rH, s_tab, residual_only != 0);
    const unsigned at = i;
    i += 256u;
    if (k + 1 < kTriImgGradSteps) fetch(i);  // the lane's next group, read before this one is stored
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T y;
#pragma unroll
      for (int e = 0; e < VEC; ++e) set_lane(y, e, r[c][e]);
      st<true>(q + (size_t)c * plane + at, y);
    }
  }
}
