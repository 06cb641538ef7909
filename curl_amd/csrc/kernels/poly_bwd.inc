// poly_bwd.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// backward of the polynomial path: d loss / d coeffs  (autograd of model.py:499-520 w.r.t. R, L, H)
// ------------------------------------------------------------------------------------------------
// Three kernels: per-pixel pullbacks (pass 1) -> 72 B/px of intermediates in HBM -> outer products per (space, monomial chunk)
// (pass 2) -> fixed-order tile sum (pass 3).  The intermediates make the HBM traffic 7.5x the 24 B/px the backward needs
// (counters: profiles/r04/poly_bwd_three_kernel_pmc.log) -- and are NOT what bounds it: both passes issue VALU instructions
// in ~80 % of their quad-cycles.  Round 4 built the one-pass form (12 waves per workgroup: six waves consume one (space, chunk)
// each, six produce the intermediates into LDS tile buffers): traffic 2x, instructions +10 % (row folds per 64-column strip),
// issue slots 43 % used behind one barrier per tile at three waves per SIMD: 1 275 us against 723 per 8 frames.  Kept as
// tools/experiments/patches/r04_poly_bwd_fused.patch; logs profiles/r04/poly_bwd_fused_*.log.
#define TRI_BWD_N 2  // pixels per lane in pass 1: one packed Horner chain (4 per lane spilled: 9 KB scratch)
// pass 1: per pixel, the 9 colour variables (planes 0..8) and the 9 upstream gradients g_P[s][o] (planes 9..17)
template <int V>
__global__ __launch_bounds__(256, 2) void trispace_bwd_px_kernel(const float* img, const float* coeffs, const float* gout,
                                                                 float* pxbuf, unsigned HW, unsigned W, float fW, float fH,
                                                                 int residual_only, int vec_ok) {
  constexpr int NC = PolyEval<V>::kCoeffs, N = TRI_BWD_N;
  typedef float VT __attribute__((ext_vector_type(N)));
  constexpr int NS = PolyEval<V>::kSeqStride;
  __shared__ __attribute__((aligned(16))) float s_coef[9 * NS];
  const unsigned b = blockIdx.y;
  const float* table = coeffs + (size_t)b * 9 * NC;
  for (int i = threadIdx.x; i < 9 * NS; i += 256) s_coef[i] = table[poly_seq_index<V>(i)];
  __syncthreads();
  const unsigned i0 = (blockIdx.x * 256u + threadIdx.x) * N;
  if (i0 >= HW) return;
  const float* pi = img + (size_t)b * 3 * HW;
  const float* pg = gout + (size_t)b * 3 * HW;
  PxN<N> in, g;
  float xw[N], yh[N];
  if (vec_ok) {  // HW % N == 0 and planes aligned to the vector: i0 + N - 1 < HW
    auto unpack = [](float (&d)[N], const float* p) {
      VT t = *(const VT*)p;
#pragma unroll
      for (int k = 0; k < N; ++k) d[k] = t[k];
    };
    unpack(in.c0, pi + i0), unpack(in.c1, pi + HW + i0), unpack(in.c2, pi + 2 * (size_t)HW + i0);
    unpack(g.c0, pg + i0), unpack(g.c1, pg + HW + i0), unpack(g.c2, pg + 2 * (size_t)HW + i0);
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      unsigned i = min(i0 + k, HW - 1);
      in.c0[k] = pi[i], in.c1[k] = pi[HW + i], in.c2[k] = pi[2 * (size_t)HW + i];
      g.c0[k] = pg[i], g.c1[k] = pg[HW + i], g.c2[k] = pg[2 * (size_t)HW + i];
    }
  }
  unsigned row = i0 / W, col = i0 - row * W;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    xw[k] = (float)col / fW, yh[k] = (float)row / fH;
    if (++col == W) col = 0, ++row;
  }
  float vars[3][3][N], gP[3][3][N];
  trispace_bwd_n<V, N, true>(in, xw, yh, s_coef, g, residual_only != 0, vars, gP);
  float* q = pxbuf + (size_t)b * 18 * HW;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* qv = q + (size_t)(s * 3 + c) * HW + i0;
      float* qg = q + (size_t)(9 + s * 3 + c) * HW + i0;
      if (vec_ok) {
        VT tv, tg;
#pragma unroll
        for (int k = 0; k < N; ++k) tv[k] = vars[s][c][k], tg[k] = gP[s][c][k];
        *(VT*)qv = tv, *(VT*)qg = tg;
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (i0 + k < HW) qv[k] = vars[s][c][k], qg[k] = gP[s][c][k];
      }
    }
}
// pass 1 for the spatial form, row-tiled like OpTriSpaceRows: the forward recompute runs on the row's collapsed
// 70-coefficient polynomials (69 FMAs per output instead of 125).  grid.x = blocks per row x rows.
__global__ __launch_bounds__(256, 2) void trispace_bwd_px_rows_kernel(const float* img, const float* coeffs, const float* gout,
                                                                      float* pxbuf, unsigned HW, unsigned W, unsigned H,
                                                                      unsigned units, unsigned segs, int residual_only,
                                                                      int vec_ok) {
  constexpr int NC4 = PolyEval<4>::kCoeffs, NC5 = PolyEval<5>::kCoeffs, N = TRI_BWD_N;
  typedef float VT __attribute__((ext_vector_type(N)));
  constexpr int NS4 = PolyEval<4>::kSeqStride;
  __shared__ __attribute__((aligned(16))) float s_coef[9 * NS4];
  const unsigned b = blockIdx.y, row = blockIdx.x / segs, seg = blockIdx.x - row * segs;
  const unsigned u = seg * blockDim.x + threadIdx.x;
  const bool live = u < units;
  const unsigned col0 = u * N, i0 = row * W + col0;
  const float* pi = img + (size_t)b * 3 * HW;
  const float* pg = gout + (size_t)b * 3 * HW;
  PxN<N> in, g;
  float xw[N], yh[N];
  if (live) {  // the pixel loads go first: they do not depend on the staging below
    if (vec_ok) {  // W % N == 0 and planes aligned to the vector: col0 + N - 1 < W
      auto unpack = [](float (&d)[N], const float* p) {
        VT t = *(const VT*)p;
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] = t[k];
      };
      unpack(in.c0, pi + i0), unpack(in.c1, pi + HW + i0), unpack(in.c2, pi + 2 * (size_t)HW + i0);
      unpack(g.c0, pg + i0), unpack(g.c1, pg + HW + i0), unpack(g.c2, pg + 2 * (size_t)HW + i0);
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        unsigned i = row * W + min(col0 + k, W - 1);
        in.c0[k] = pi[i], in.c1[k] = pi[HW + i], in.c2[k] = pi[2 * (size_t)HW + i];
        g.c0[k] = pg[i], g.c1[k] = pg[HW + i], g.c2[k] = pg[2 * (size_t)HW + i];
      }
    }
  }
  {
    // the image's 9 x 126 raw coefficients into LDS (8-byte pairs, four loads in flight), then the row's folds from one
    // 16-byte table row + LDS reads each -- as the forward stages them (stream.inc, OpTriSpaceRows::stage_value); read
    // through the index table straight from global memory, a fold was a chain of ~12 dependent loads
    typedef float f2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) float s_raw[(9 * NC5 + 3) & ~3];
    constexpr unsigned n2 = 9 * NC5 / 2;
    const f2* tg = reinterpret_cast<const f2*>(coeffs + (size_t)b * 9 * NC5);
    for (unsigned j0 = 0; j0 < n2; j0 += 4u * blockDim.x) {
      f2 r[4];
#pragma unroll
      for (unsigned k = 0; k < 4; ++k) r[k] = tg[min(j0 + k * blockDim.x + threadIdx.x, n2 - 1u)];
#pragma unroll
      for (unsigned k = 0; k < 4; ++k) {
        const unsigned j = j0 + k * blockDim.x + threadIdx.x;
        if (j < n2) reinterpret_cast<f2*>(s_raw)[j] = r[k];
      }
    }
    __syncthreads();
    const float y = (float)row / (float)H;
    for (unsigned i = threadIdx.x; i < 9u * NS4; i += blockDim.x) {
      unsigned q = i / NS4, pos = i - q * NS4;
      s_coef[i] = pos < (unsigned)NC4 ? collapse_coef_fold(s_raw + q * NC5, (int)pos, y) : 0.0f;
    }
  }
  __syncthreads();
  if (!live) return;
  const float fW = (float)W, rW = 1.0f / fW;
#pragma unroll
  for (int k = 0; k < N; ++k) xw[k] = div_small((float)(col0 + k), fW, rW), yh[k] = 0.0f;
  float vars[3][3][N], gP[3][3][N];
  trispace_bwd_n<4, N, true>(in, xw, yh, s_coef, g, residual_only != 0, vars, gP);
  float* q = pxbuf + (size_t)b * 18 * HW;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* qv = q + (size_t)(s * 3 + c) * HW + i0;
      float* qg = q + (size_t)(9 + s * 3 + c) * HW + i0;
      if (vec_ok) {
        VT tv, tg;
#pragma unroll
        for (int k = 0; k < N; ++k) tv[k] = vars[s][c][k], tg[k] = gP[s][c][k];
        *(VT*)qv = tv, *(VT*)qg = tg;
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (col0 + k < W) qv[k] = vars[s][c][k], qg[k] = gP[s][c][k];
      }
    }
}
// pass 2: block (tile of 256*ppt pixels; space s and monomial chunk C; image b) accumulates g_P[s][o] * m_t in
// registers, reduces over the block, writes one row of partials.
struct CoefGradArgs {
  const float* pxbuf;
  float* partial;
  unsigned HW, W, tiles, ppt, items;  // items = B * 3 * tiles work items (image, space, tile)
  unsigned step_rows, step_cols;      // 256 / W, 256 % W: how (row, col) advances per loop step
  float fW, fH;
};
template <int V, int C>
__device__ __forceinline__ void coef_grad_block(const CoefGradArgs& a, unsigned b, unsigned s, unsigned tile,
                                                float (*sPart)[3 * PolyEval<V>::kChunk]) {
  constexpr int NC = PolyEval<V>::kCoeffs, T = PolyEval<V>::kChunk;
  const unsigned HW = a.HW;
  const float* base = a.pxbuf + (size_t)b * 18 * HW + (size_t)(s * 3) * HW;
  constexpr int NPAIR = (T + 1) / 2;
  grad_pair acc[3][NPAIR];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int k = 0; k < NPAIR; ++k) acc[o][k] = grad_pair{0.0f, 0.0f};
  unsigned i = tile * 256u * a.ppt + threadIdx.x;
  unsigned row = i / a.W, col = i - row * a.W;
  const float rW = 1.0f / a.fW, rH = 1.0f / a.fH;
  auto fetch = [&](float (&d)[6], unsigned at) {  // clamped: always a valid pixel, masked below
    const float* p = base + min(at, HW - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = p[(size_t)c * HW], d[3 + c] = p[(size_t)(9 + c) * HW];
  };
  float cur[6], nxt[6];
  fetch(cur, i);
  for (unsigned k = 0; k < a.ppt; ++k) {
    fetch(nxt, i + 256u);  // next step's operands are in flight while this step computes
    float v[V], g[3];
    const bool live = i < HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = cur[c], g[c] = live ? cur[3 + c] : 0.0f;
    if (V == 5) {
      v[V - 2] = div_small((float)col, a.fW, rW);
      v[V - 1] = div_small((float)row, a.fH, rH);
    }
    coef_grad_accumulate<V, C>(acc, v, g);
    CURL_FENCE();  // keep the wait for the prefetch at the end of the step
#pragma unroll
    for (int c = 0; c < 6; ++c) cur[c] = nxt[c];
    i += 256u, row += a.step_rows, col += a.step_cols;
    if (col >= a.W) col -= a.W, ++row;
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
    int o = idx / T, j = idx - o * T;
    int t = C * T + j;
    if (t < NC)
      a.partial[((size_t)b * a.tiles + tile) * 9 * NC + (s * 3 + o) * NC + t] =
          (sPart[0][idx] + sPart[1][idx]) + (sPart[2][idx] + sPart[3][idx]);
  }
}
// 1-D grid.  Workgroups are dealt round-robin to the 8 XCDs (id % 8); the kChunks blocks of one work item re-read
// the same 6 planes of the tile, so they get ids 8 apart: same XCD, same L2, dispatched together.
template <int V>
__global__ __launch_bounds__(256) void trispace_coef_grad_kernel(CoefGradArgs a) {
  constexpr int CH = PolyEval<V>::kChunks;
  __shared__ float sPart[4][3 * PolyEval<V>::kChunk];
  const unsigned n = blockIdx.x, group = n / (8u * CH), r = n - group * (8u * CH);
  const unsigned chunk = r >> 3, item = group * 8u + (r & 7u);  // block-uniform
  if (item >= a.items) return;
  const unsigned tile = item % a.tiles, bs = item / a.tiles, s = bs % 3u, b = bs / 3u;
  if (chunk == 0) coef_grad_block<V, 0>(a, b, s, tile, sPart);
  if constexpr (CH > 1) {
    if (chunk == 1) coef_grad_block<V, 1>(a, b, s, tile, sPart);
    if (chunk == 2) coef_grad_block<V, 2>(a, b, s, tile, sPart);
  }
}
// pass 2 of the SPATIAL form, in column strips.  A thread keeps one image column (2^cw_log2 columns x 256 >> cw_log2 row
// phases per block) and walks down `steps` rows: its x = column / W never changes, so it accumulates over the 70 monomials
// of (c0, c1, c2, y) only -- two chunks of 35, 105 accumulators -- and multiplies by the powers of x once, on the way into
// the wave reduction (coef_grad_expand_foldx; PolyFoldX in poly_horner.inc).  Per pixel and space: 2 x (35 monomials +
// 105 FMAs) instead of 3 x (42 + 126).  Loads stay coalesced (a wave = 64 consecutive columns of one row).
struct CoefGradStripArgs {
  const float* pxbuf;
  float* partial;
  unsigned HW, W, H;
  unsigned cw_log2, steps;     // block shape; rows per thread
  unsigned n_cb, n_rt, items;  // column blocks, row tiles; items = B * 3 * n_cb * n_rt
  float fW, fH;
};
#define STRIP_SPART (3 * kPolyFoldXMaxSlices * kPolyFoldXMaxSlice)
template <int C, int S>
__device__ __forceinline__ void strip_reduce_slices(const foldx_pair (&acc)[kFoldXPairs], float x, float* dst, int lane_id) {
  if constexpr (S < PolyFoldX<C>::kSlices) {
    constexpr int L = PolyFoldX<C>::kSlice;
    float e[L];
    coef_grad_expand_foldx<C, S>(e, acc, x);
    wave_sum_many(e, dst + S * kPolyFoldXMaxSlice, lane_id);
    strip_reduce_slices<C, S + 1>(acc, x, dst, lane_id);
  }
}
template <int C>
__device__ __forceinline__ void coef_grad_strip_block(const CoefGradStripArgs& a, unsigned b, unsigned s, unsigned tile,
                                                      float (*sPart)[STRIP_SPART]) {
  constexpr int NC = PolyEval<5>::kCoeffs;
  const unsigned HW = a.HW, cb = tile % a.n_cb, rt = tile / a.n_cb;
  const unsigned cw = 1u << a.cw_log2, rp = 256u >> a.cw_log2;
  const unsigned col = cb * cw + (threadIdx.x & (cw - 1u)), colc = min(col, a.W - 1u);
  unsigned row = rt * a.steps * rp + (threadIdx.x >> a.cw_log2);
  const float* base = a.pxbuf + (size_t)b * 18 * HW + (size_t)(s * 3) * HW + colc;
  const float rW = 1.0f / a.fW, rH = 1.0f / a.fH;
  const float x = div_small((float)colc, a.fW, rW);
  foldx_pair acc[3][kFoldXPairs];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int k = 0; k < kFoldXPairs; ++k) acc[o][k] = foldx_pair{0.0f, 0.0f};
  auto fetch = [&](float (&d)[6], unsigned r) {  // clamped: always a valid pixel, masked below
    const float* p = base + (size_t)min(r, a.H - 1u) * a.W;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = p[(size_t)c * HW], d[3 + c] = p[(size_t)(9 + c) * HW];
  };
  float cur[6], nxt[6];
  fetch(cur, row);
  for (unsigned k = 0; k < a.steps; ++k) {
    fetch(nxt, row + rp);  // next step's operands are in flight while this step computes
    const bool live = col < a.W && row < a.H;
    float v[3], g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = cur[c], g[c] = live ? cur[3 + c] : 0.0f;
    coef_grad_accumulate_foldx<C>(acc, v, div_small((float)min(row, a.H - 1u), a.fH, rH), g);
    CURL_FENCE();  // keep the wait for the prefetch at the end of the step
#pragma unroll
    for (int c = 0; c < 6; ++c) cur[c] = nxt[c];
    row += rp;
  }
  const int wave = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
#pragma unroll
  for (int o = 0; o < 3; ++o)
    strip_reduce_slices<C, 0>(acc[o], x, sPart[wave] + o * kPolyFoldXMaxSlices * kPolyFoldXMaxSlice, lane_id);
  __syncthreads();
  constexpr int per_o = kPolyFoldXMaxSlices * kPolyFoldXMaxSlice;
  for (int idx = threadIdx.x; idx < 3 * per_o; idx += 256) {
    const int o = idx / per_o, r = idx - o * per_o;
    const unsigned t = kPolyFoldXIndex[C][r / kPolyFoldXMaxSlice][r % kPolyFoldXMaxSlice];
    if (t != 0xFFFFu)
      a.partial[((size_t)b * (a.n_cb * a.n_rt) + tile) * 9 * NC + (s * 3 + o) * NC + t] =
          (sPart[0][idx] + sPart[1][idx]) + (sPart[2][idx] + sPart[3][idx]);
  }
}
// 1-D grid, the two chunk blocks of one item 8 ids apart (same XCD, same L2: they read the same 6 planes)
__global__ __launch_bounds__(256) void trispace_coef_grad_strip_kernel(CoefGradStripArgs a) {
  constexpr int CH = kPolyFoldXChunks;
  static_assert(CH == 2, "two chunks of 35");
  __shared__ float sPart[4][STRIP_SPART];
  const unsigned n = blockIdx.x, group = n / (8u * CH), r = n - group * (8u * CH);
  const unsigned chunk = r >> 3, item = group * 8u + (r & 7u);  // block-uniform
  if (item >= a.items) return;
  const unsigned tiles = a.n_cb * a.n_rt, tile = item % tiles, bs = item / tiles, s = bs % 3u, b = bs / 3u;
  if (chunk == 0) coef_grad_strip_block<0>(a, b, s, tile, sPart);
  else coef_grad_strip_block<1>(a, b, s, tile, sPart);
}
// pass 3: fixed-order float64 sum of the tile partials -> grad_coeffs [B,3,3,NC].  A block = 32 outputs x 8 tile phases:
// thread (output, phase) adds tiles phase, phase + 8, ... in order, then the 8 phase sums are added in phase order -- a
// fixed order (bit-reproducible), 8 independent chains per output instead of one walk over every tile.
#define COEF_FINAL_OUTS 32
__global__ __launch_bounds__(256) void trispace_coef_final_kernel(const float* partial, float* gcoef, unsigned tiles, int n) {
  __shared__ double s[8][COEF_FINAL_OUTS];
  const unsigned b = blockIdx.y;
  const int kl = threadIdx.x & (COEF_FINAL_OUTS - 1), ph = threadIdx.x / COEF_FINAL_OUTS;
  const int k = blockIdx.x * COEF_FINAL_OUTS + kl;
  double a = 0.0;
  if (k < n) {
    const float* p = partial + (size_t)b * tiles * n + k;
    a = walk_sum8(p, (size_t)ph * n, 8 * (size_t)n, (size_t)tiles * n);  // tiles ph, ph + 8, ...: eight loads in flight (layer_bwd.inc)
  }
  s[ph][kl] = a;
  __syncthreads();
  if (ph == 0 && k < n) {
    double r = s[0][kl];
#pragma unroll
    for (int q = 1; q < 8; ++q) r += s[q][kl];
    gcoef[(size_t)b * n + k] = (float)r;
  }
}
