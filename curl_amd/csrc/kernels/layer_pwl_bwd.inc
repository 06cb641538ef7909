// layer_pwl_bwd.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// backward of the fused layer with the paper's piecewise-linear curves (CURL_F_PWL, OpLayerTab<0>)
// ------------------------------------------------------------------------------------------------
// The shape of layer_bwd_kernel / knots_bwd_kernel: a per-pixel pass recomputes the tape in registers, writes grad_img and one
// row of block partials; a per-image pass sums the rows in a fixed order in float64 and applies the chain rule.  What differs is
// the width of a row: a PWL curve of K knots owes K sums (curl_math_bwd.h curl_layer_pwl_bwd: sum G and sum G clamp01(s - j),
// j = 0 .. K-2) instead of the affine form's two, so a row is n_knots floats -- curve after curve, in the knots' own order.
struct PwlBwdArgs : BwdArgs {  // the tile's arguments (bwd_tile.inc; partial rows are n_knots floats), and
  int kl, kr, kh;              // knots per curve (even splits only)
};

// The 16-wide chunks of a curve's sums: index t of a curve is sum G (t = 0) or sum G clamp01(s - (t - 1)); a curve's LDS slot
// of one wave holds round_up(K, 16) floats, so a chunk's wave sum (wave_sum_many, 16 values) never writes into the next curve.
__device__ __forceinline__ int pwl_pad16(int K) { return (K + 15) & ~15; }

// One curve's sums over the lane's VEC pixels (s[e], G[e]), then over the wave, into the wave's LDS slot `dst`.  Chunks of
// 16 with a run-time trip count: 16 accumulators live at any K (256 knots neither spill nor need a template per K).
template <int VEC>
__device__ __forceinline__ void pwl_curve_sums(const float (&s)[VEC], const float (&G)[VEC], int K, float* dst, int lane_id) {
  for (int t0 = 0; t0 < K; t0 += 16) {
    float acc[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      // t = 0: weight 1 (s - (-inf) clamps to 1); past the curve's last index the weights go to a padding slot nobody reads
      const float j = (t0 + jj == 0) ? -__builtin_inff() : (float)(t0 + jj - 1);
      float a = 0.0f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) a = fmaf(G[e], clamp01(s[e] - j), a);
      acc[jj] = a;
    }
    wave_sum_many(acc, dst + t0, lane_id);
  }
}

// Where the per-pixel pullback leaves a curve's (s, G): registers of the lane, one pair per curve and pixel.
template <int VEC>
struct PwlTape {
  float s[MAX_CURVES][VEC], G[MAX_CURVES][VEC];
  int e;  // the pixel being pulled back (a compile-time constant once the pixel loop is unrolled)
  __device__ __forceinline__ void operator()(int c, float sv, float g) { s[c][e] = sv, G[c][e] = g; }
};

template <int VEC, int MK, bool GIN = true>
__global__ __launch_bounds__(256, 1) void layer_pwl_bwd_kernel(PwlBwdArgs a) {
  typedef typename Pack<VEC>::T T;
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  const int kl = a.kl, kr = a.kr, kh = a.kh;
  const int n_knots = 3 * kl + 3 * kr + 4 * kh;
  const int pl = pwl_pad16(kl), pr = pwl_pad16(kr), ph = pwl_pad16(kh);
  const int n_pad = 3 * pl + 3 * pr + 4 * ph;  // one wave's slots
  float* s_tab = s_dyn;                  // [2 n_knots] {knot, slope} pairs, OpLayerTab<0>'s table
  float* s_part = s_dyn + 2 * n_knots;   // [4][n_pad] the waves' sums
  const unsigned img = blockIdx.y;
  const unsigned chunk = blockIdx.x;
  const unsigned bid = img * a.blocks_per_image + chunk;
  const float* row = a.coef + (size_t)img * a.coef_stride;
  BwdTile<VEC, MK, GIN> tile;
  tile.load(a.in, a.gout, a.mask, img, chunk, a.n, a.mask_first);
  // the image's table, staged while the pixel loads are in flight: knot j, and slope j = C[j+1] - C[j] inside its curve, 0 for a
  // curve's last knot (OpLayerTab::stage_value, the same floats)
  for (int t = threadIdx.x; t < n_knots; t += 256) {
    const float c = row[WS_KNOTS + t];
    const int in_curve = t < 3 * kl ? t % kl : t < 3 * kl + 3 * kr ? (t - 3 * kl) % kr : (t - 3 * kl - 3 * kr) % kh;
    const int Kc = t < 3 * kl ? kl : t < 3 * kl + 3 * kr ? kr : kh;
    s_tab[2 * t] = c;
    s_tab[2 * t + 1] = in_curve + 1 < Kc ? row[WS_KNOTS + t + 1] - c : 0.0f;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
  float* my_part = s_part + wave * n_pad;
  T y0, y1, y2;
  if (GIN && tile.dead) y0 = T(0.0f), y1 = T(0.0f), y2 = T(0.0f);
  if (!tile.dead) {
    PwlTape<VEC> tape;
    float dep = 0.0f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float m = tile.m(e);
      Px pin = tile.pin(e), gin = tile.gin(e);
      if (!tile.valid()) m = 0.0f;  // lanes past the end contribute nothing (G = 0 on every curve)
      // one pixel after the other (bwd_tile.inc, at BwdTile::m)
      asm volatile("" : "+v"(pin.c0), "+v"(pin.c1), "+v"(pin.c2), "+v"(gin.c0), "+v"(gin.c1), "+v"(gin.c2) : "v"(dep));
      tape.e = e;
      Px fwd;
      Px gi = curl_layer_pwl_bwd<MK != CURL_MASK_F32, GIN>(pin, m, s_tab, kl, kr, kh, gin, tape, fwd);
      dep = gi.c0;
      if constexpr (GIN) {
        set_lane(y0, e, gi.c0);
        set_lane(y1, e, gi.c1);
        set_lane(y2, e, gi.c2);
      }
    }
    // the ten curves' sums, curve by curve, into this wave's slots
    int off = 0;
#pragma unroll
    for (int c = 0; c < MAX_CURVES; ++c) {
      const int K = c < 3 ? kl : c < 6 ? kr : kh, P = c < 3 ? pl : c < 6 ? pr : ph;
      pwl_curve_sums<VEC>(tape.s[c], tape.G[c], K, my_part + off, lane_id);
      off += P;
    }
  } else {
    for (int t = lane_id; t < n_pad; t += 64) my_part[t] = 0.0f;
  }
  if constexpr (GIN) {
    if (a.gin) tile.store(a.gin, row, a.stamp, y0, y1, y2);
  }
  __syncthreads();
  // the block's row: the four waves' sums added in a fixed order, in the knots' layout (curve c at its first knot)
  for (int t = threadIdx.x; t < n_knots; t += 256) {
    int slot;
    if (t < 3 * kl) slot = (t / kl) * pl + t % kl;
    else if (t < 3 * kl + 3 * kr) slot = 3 * pl + ((t - 3 * kl) / kr) * pr + (t - 3 * kl) % kr;
    else slot = 3 * pl + 3 * pr + ((t - 3 * kl - 3 * kr) / kh) * ph + (t - 3 * kl - 3 * kr) % kh;
    a.partial[(size_t)bid * n_knots + t] =
        (s_part[slot] + s_part[n_pad + slot]) + (s_part[2 * n_pad + slot] + s_part[3 * n_pad + slot]);
  }
}
// dynamic LDS of layer_pwl_bwd_kernel: the table and four waves' slots
static inline size_t pwl_bwd_lds_bytes(int kl, int kr, int kh) {
  const int n_knots = 3 * kl + 3 * kr + 4 * kh;
  const int n_pad = 3 * ((kl + 15) & ~15) + 3 * ((kr + 15) & ~15) + 4 * ((kh + 15) & ~15);
  return (size_t)(2 * n_knots + 4 * n_pad) * sizeof(float);
}

// One workgroup per (curve, image): thread t < phases * K walks column t % K of the curve's slice of the rows, every
// phases-th row from row t / K (walk_sum8: eight loads in flight, float64), then the phase sums of a column are added in phase
// order -- a fixed order, bit-reproducible -- and each knot gets the chain rule (curl_math_bwd.h knot_bwd_pwl).
#define PWL_KNOTS_THREADS 1024
__global__ __launch_bounds__(PWL_KNOTS_THREADS) void layer_pwl_knots_bwd_kernel(KnotsBwdArgs a) {
  __shared__ double sAcc[PWL_KNOTS_THREADS];
  __shared__ double sT[CURL_MAX_KNOTS];
  const unsigned c = blockIdx.x, b = blockIdx.y;
  int K0 = a.K[0], K1 = a.K[1], K2 = a.K[2];
  float *g0 = a.graw[0], *g1 = a.graw[1], *g2 = a.graw[2];
  asm volatile("" : "+s"(K0), "+s"(K1), "+s"(K2), "+s"(g0), "+s"(g1), "+s"(g2));  // (knots_bwd_kernel: no indexed argument loads)
  const int n_knots = 3 * K0 + 3 * K1 + 4 * K2;
  const int seg = c < 3 ? 0 : c < 6 ? 1 : 2;
  const int K = seg == 0 ? K0 : seg == 1 ? K1 : K2;
  const int local = (int)c - (seg == 0 ? 0 : seg == 1 ? 3 : 6);
  const int off = (seg == 0 ? 0 : seg == 1 ? 3 * K0 : 3 * K0 + 3 * K1) + local * K;  // the curve's first knot in a row
  float* g = (seg == 0 ? g0 : seg == 1 ? g1 : g2) + (size_t)b * (seg == 2 ? 4 : 3) * K + local * K;
  const float* row = a.ws + (size_t)b * a.ws_stride;
  const bool row_ok = reinterpret_cast<const unsigned*>(row)[WS_STAMP] == ws_stamp((unsigned)n_knots, a.ws_stride);
  const float greg_f = a.greg ? a.greg[b] : 0.0f;
  const int phases = PWL_KNOTS_THREADS / K;
  const float* part = a.partial + (size_t)b * a.blocks_per_image * n_knots;
  const int t = (int)threadIdx.x;
  if (t < phases * K)
    sAcc[t] = walk_sum8(part, (size_t)(t / K) * n_knots + off + t % K, (size_t)phases * n_knots,
                        (size_t)a.blocks_per_image * n_knots);
  __syncthreads();
  if (t < K) {
    double r = sAcc[t];
    for (int p = 1; p < phases; ++p) r += sAcc[t + p * K];
    sT[t] = r;
  }
  __syncthreads();
  if (t < K) {
    const float v = knot_bwd_pwl(row + WS_KNOTS + off, K, sT, (double)greg_f, t);
    g[t] = row_ok ? v : __builtin_nanf("");
  }
}
