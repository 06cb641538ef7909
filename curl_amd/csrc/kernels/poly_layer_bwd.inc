// poly_layer_bwd.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// backward of the stand-alone polynomial layer (autograd of ChannelPolyLayer(degree 4) / Deg4MobilePolyLayer.forward,
// model.py:295-333, 399-415): out[b][o][px] = P_o(img[b][:, px]), the V variables read straight from memory.
//   grad_coeffs[b][o][t] = sum_px grad_out[b][o][px] * m_t(img[b][:, px])          poly_layer_coef_grad_kernel + the tile sum
//   grad_img[b][i][px]   = sum_o grad_out[b][o][px] * dP_o/dv_i(img[b][:, px])     poly_layer_img_grad_kernel
// Two launches, not one kernel: the coefficient gradient is tiled by monomial CHUNK (three workgroups per tile for V = 5,
// each holding 3 x 42 accumulators in registers), the image gradient is per pixel and wants every pixel once.  Either is
// left out when its gradient is not wanted (arithmetic: curl_math_poly.h; DESIGN.md 3a).
// ------------------------------------------------------------------------------------------------
// One pass over the V planes of img and the 3 of grad_out, no intermediate image: nothing to recompute (the tri-space
// backward's pass 1 exists for the converters).  A lane owns GROUPS of 4 consecutive pixels -- one float4 per plane when
// VEC == 4, four clamped scalar loads when VEC == 1 (any size or alignment) -- so both instantiations add the same pixels in
// the same order: the result does not depend on the alignment of the call.  A tile = `steps` x 256 groups; block
// (tile, chunk C, image b) accumulates g[o] * m_t in register pairs, reduces over the block (wave_sum_many -> LDS), writes
// one row of partials; trispace_coef_final_kernel sums the rows in a fixed order in float64.  No atomics.
struct PolyLayerGradArgs {
  const float* img;
  const float* gout;
  float* partial;
  unsigned HW, groups;          // groups = ceil(HW / 4)
  unsigned tiles, steps, items;  // groups per lane and tile; items = B * tiles
};
template <int V, int C, int VEC>
__device__ __forceinline__ void poly_layer_coef_block(const PolyLayerGradArgs& a, unsigned b, unsigned tile,
                                                      float (*sPart)[3 * PolyEval<V>::kChunk]) {
  constexpr int NC = PolyEval<V>::kCoeffs, T = PolyEval<V>::kChunk, NPAIR = (T + 1) / 2;
  const unsigned HW = a.HW;
  const float* pv = a.img + (size_t)b * V * HW;
  const float* pg = a.gout + (size_t)b * 3 * HW;
  grad_pair acc[3][NPAIR];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int k = 0; k < NPAIR; ++k) acc[o][k] = grad_pair{0.0f, 0.0f};
  auto fetch = [&](v4f (&d)[V + 3], unsigned group) {  // clamped: always valid pixels, masked below
    if constexpr (VEC == 4) {
      const size_t at = 4 * (size_t)min(group, a.groups - 1u);  // HW % 4 == 0: the whole group is inside
#pragma unroll
      for (int k = 0; k < V; ++k) d[k] = *reinterpret_cast<const v4f*>(pv + (size_t)k * HW + at);
#pragma unroll
      for (int o = 0; o < 3; ++o) d[V + o] = *reinterpret_cast<const v4f*>(pg + (size_t)o * HW + at);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const size_t at = min(4u * min(group, a.groups - 1u) + e, HW - 1u);
#pragma unroll
        for (int k = 0; k < V; ++k) d[k][e] = pv[(size_t)k * HW + at];
#pragma unroll
        for (int o = 0; o < 3; ++o) d[V + o][e] = pg[(size_t)o * HW + at];
      }
    }
  };
  unsigned i = tile * 256u * a.steps + threadIdx.x;
  v4f cur[V + 3], nxt[V + 3];
  fetch(cur, i);
  for (unsigned k = 0; k < a.steps; ++k) {
    fetch(nxt, i + 256u);  // next step's operands are in flight while this step computes
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool live = i < a.groups && 4u * i + e < HW;
      float v[V], g[3];
#pragma unroll
      for (int c = 0; c < V; ++c) v[c] = cur[c][e];
#pragma unroll
      for (int o = 0; o < 3; ++o) g[o] = live ? cur[V + o][e] : 0.0f;
      coef_grad_accumulate<V, C>(acc, v, g);
      CURL_FENCE();  // one pixel's monomials at a time; the wait for the prefetch stays at the end of the step
    }
#pragma unroll
    for (int c = 0; c < V + 3; ++c) cur[c] = nxt[c];
    i += 256u;
  }
  const int wave = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    float e[T];
#pragma unroll
    for (int j = 0; j < T; ++j) e[j] = grad_pair_get(acc[o], j);
    wave_sum_many(e, sPart[wave] + o * T, lane_id);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 3 * T; idx += 256) {
    const int o = idx / T, j = idx - o * T, t = C * T + j;
    if (t < NC)
      a.partial[((size_t)b * a.tiles + tile) * 3 * NC + o * NC + t] =
          (sPart[0][idx] + sPart[1][idx]) + (sPart[2][idx] + sPart[3][idx]);
  }
}
// 1-D grid.  Workgroups are dealt round-robin to the 8 XCDs (id % 8); the kChunks blocks of one tile re-read the same planes,
// so they get ids 8 apart: same XCD, same L2, dispatched together (as trispace_coef_grad_kernel).
template <int V, int VEC>
__global__ __launch_bounds__(256) void poly_layer_coef_grad_kernel(PolyLayerGradArgs a) {
  constexpr int CH = PolyEval<V>::kChunks;
  __shared__ float sPart[4][3 * PolyEval<V>::kChunk];
  const unsigned n = blockIdx.x, group = n / (8u * CH), r = n - group * (8u * CH);
  const unsigned chunk = r >> 3, item = group * 8u + (r & 7u);  // block-uniform
  if (item >= a.items) return;
  const unsigned tile = item % a.tiles, b = item / a.tiles;
  if (chunk == 0) poly_layer_coef_block<V, 0, VEC>(a, b, tile, sPart);
  if constexpr (CH > 1) {
    if (chunk == 1) poly_layer_coef_block<V, 1, VEC>(a, b, tile, sPart);
    if (chunk == 2) poly_layer_coef_block<V, 2, VEC>(a, b, tile, sPart);
  }
}

// The image gradient, shaped as poly_layer_kernel: a lane owns VEC pixels (float4 per plane, or one pixel of any size or
// alignment), the image's 3 V derivative polynomials sit in LDS in the order the degree-3 Horner scheme consumes them
// (poly_deriv_stage), and the lane's VEC scalar chains share every coefficient read.  n = HW / VEC.
template <int V, int VEC>
__global__ __launch_bounds__(256, 4) void poly_layer_img_grad_kernel(const float* in, const float* coeffs, const float* gout,
                                                                     float* gin, unsigned n) {
  typedef typename Pack<VEC>::T T;
  constexpr int NC = PolyEval<V>::kCoeffs, ND = 3 * V * PolyDeriv<V>::kTerms;
  __shared__ __attribute__((aligned(16))) float s_D[ND];
  const unsigned img = blockIdx.y;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const size_t plane = (size_t)n;
  const T* p = reinterpret_cast<const T*>(in) + (size_t)img * V * plane + min(i, n - 1u);
  const T* pg = reinterpret_cast<const T*>(gout) + (size_t)img * 3 * plane + min(i, n - 1u);
  T x[V], w[3];
#pragma unroll
  for (int k = 0; k < V; ++k) x[k] = ld<true>(p + (size_t)k * plane);  // before the staging barrier
#pragma unroll
  for (int o = 0; o < 3; ++o) w[o] = ld<true>(pg + (size_t)o * plane);
  const float* table = coeffs + (size_t)img * 3 * NC;
  for (int j = threadIdx.x; j < ND; j += 256) s_D[j] = poly_deriv_stage<V>(table, j);
  __syncthreads();
  if (i >= n) return;
  float vars[V][VEC], g[3][VEC], r[V][VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
#pragma unroll
    for (int k = 0; k < V; ++k) vars[k][e] = lane(x[k], e);
#pragma unroll
    for (int o = 0; o < 3; ++o) g[o][e] = lane(w[o], e);
  }
  poly_img_grad_n<V, VEC>(r, vars, g, s_D);
  T* q = reinterpret_cast<T*>(gin) + (size_t)img * V * plane + i;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    T y;
#pragma unroll
    for (int e = 0; e < VEC; ++e) set_lane(y, e, r[k][e]);
    st<true>(q + (size_t)k * plane, y);
  }
}
