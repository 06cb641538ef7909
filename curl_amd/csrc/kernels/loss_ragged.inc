// loss_ragged.inc -- part of curl_kernels.hip (one translation unit; included after msssim_ragged.inc, whose plan walk,
// pooling and pair reduction it uses, and loss.inc; not compiled alone).
// ------------------------------------------------------------------------------------------------
// the CURLLoss statistics of a batch of byte images of different sizes (include/curl_hip_ragged_loss.h)
// ------------------------------------------------------------------------------------------------
// Six launches for the whole batch, whatever B is -- msssim_ragged.inc's walk on ONE channel, the clamped L of model.py:100-105:
//   level 0     the grid is the sum of the images' 32x32 tiles.  A workgroup finds its image and checks its descriptor as
//               msssim_ragged_bytes_kernel does, stages its tile plus the 5-pixel halo of prediction and target as BYTES (zero
//               outside the image and where the mask byte is 0), runs loss_terms -- curl_math_loss.h's per-pixel form of what
//               loss_terms_kernel runs four pixels at a time -- on the tile's own pixels (four term contributions, the two L
//               values, the count from the mask byte) and rgb2lab, the converter inside it, on the halo ring (the two L values
//               alone: the converter's operations are written out one by one, so a pixel has one L whichever tile stages
//               it), then the window passes on the two L tiles, in float64 (ls_ssim_plane below), and the 16x16 piece of
//               the level-1 planes (ms_pool_store).  (The
//               per-pixel form, not loss_terms_n: its cone is formed with contraction off, so equal colours give equal cones
//               and an output scored against itself has rgb = lab = hsv = 0 exactly; loss_terms_n's fused
//               v s cos - v' s' cos' leaves the rounding residue of one product there.)  Outside the image the L tiles hold
//               0.0f (conv2d's padding); a masked-out pixel inside it holds the L the converter gives black.  No
//               full-resolution float plane is written.
//   levels 1-4  the same walk on the workspace's two float planes per level, one launch per level.
//   finish      B workgroups: per level the fixed-order float64 sum of the image's pairs -> the two means over h*w values, and
//               the fixed-order sums of its level-0 tiles' four terms and count.
// A level-0 workgroup writes SEVEN float64 (its pair, as there; four term sums and the count into the term partials): zeros
// when its descriptor fails a check; a stale or foreign plan writes nothing at all.  No atomics, no memset.
constexpr unsigned kLsStamp = 0x4C535231u, kLsOp = 6u;
constexpr int kLsTerms = 5;       // sum|p-t|, sum cos, sum|lab|, sum|cone|, count
constexpr int kLsRing = 2 * SSIM_R * SSIM_IN + 2 * SSIM_R * SSIM_TILE;  // the halo's positions: 740 of 1764
enum { LH_TERMS_OFF = 28 };       // header word beside msssim_ragged.inc's MH_*: (i64) byte offset of the term partials

// a level's two float planes (prediction L, target L) lie inside the workspace's plane region
__device__ __forceinline__ bool ls_planes_ok(const MsLevel& v, unsigned long long planes_bytes) {
  return v.planes % 4u == 0u && v.planes <= planes_bytes && 8ull * v.h * v.w <= planes_bytes - v.planes;
}

typedef unsigned char LsBytes[2][3][SSIM_IN][SSIM_IN];  // prediction / target, channel, the tile + halo
// a staged pixel as to_tensor gives it: byte / 255 correctly rounded
__device__ __forceinline__ Px ls_px(const LsBytes& s8, int k, int ly, int lx) {
  return Px{u8_to_unit((float)s8[k][0][ly][lx]), u8_to_unit((float)s8[k][1][ly][lx]), u8_to_unit((float)s8[k][2][ly][lx])};
}

// The window passes of the L statistics, in FLOAT64 on the float32 L tiles.  msssim_ragged.inc's ms_ssim_plane forms the five
// blurs in float32; on ONE channel that misses the float64 oracle: a variance is blur(x^2) - blur(x)^2 against C2 = 9e-4, a
// float32 rounding of blur(x^2) is 2e-8 -- 1e-5 of the denominator once a plane is pooled flat -- and on a flat plane it is the
// same rounding at every pixel, so nothing averages out (DESIGN.md 3a.9).  Here the horizontal pass goes into a float64 row
// buffer, three quantities at a time (a, b, ab; then a^2, b^2: 33 264 B, which also holds the staged bytes before the L tiles
// exist), and the vertical pass and metric.py:139-163 stay in float64 registers.  The weights are g[k] * gscale: g the
// reference's float32 window (ls_window, host side) and gscale the factor that gives the separable window the total of the
// reference's 2-D float32 window round(g_i g_j).  The caller has a barrier behind the staging of sa / sb.
typedef double LsRow[3][SSIM_IN][SSIM_TILE + 1];
static_assert(sizeof(LsRow) >= sizeof(LsBytes), "the staged bytes fit the row buffer they share LDS with");

template <int Q>  // the horizontal pass of Q quantities: Q = 3: a, b, ab; Q = 2: a^2, b^2
__device__ __forceinline__ void ls_rows(const MsIn& sa, const MsIn& sb, LsRow& sh, const SsimArgs& p, double gscale) {
  const int r = p.radius, off = SSIM_R - r;
  for (int i = threadIdx.x; i < SSIM_IN * SSIM_TILE; i += 256) {
    const int ly = i / SSIM_TILE, cx = i - ly * SSIM_TILE;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = 0; k <= 2 * r; ++k) {
      const double w = (double)p.g[k] * gscale, va = (double)sa[ly][cx + off + k], vb = (double)sb[ly][cx + off + k];
      if (Q == 3) s0 = fma(w, va, s0), s1 = fma(w, vb, s1), s2 = fma(w, va * vb, s2);
      else s0 = fma(w, va * va, s0), s1 = fma(w, vb * vb, s1);
    }
    sh[0][ly][cx] = s0, sh[1][ly][cx] = s1;
    if (Q == 3) sh[2][ly][cx] = s2;
  }
}

__device__ __forceinline__ void ls_ssim_plane(const MsIn& sa, const MsIn& sb, LsRow& sh, const SsimArgs& p, double gscale, int ty0, int tx0,
                                              int H, int W, double& sum_s, double& sum_c) {
  constexpr int kRows = SSIM_TILE / 8;  // output rows per lane
  const int r = p.radius, off = SSIM_R - r;
  const int tx = threadIdx.x & 31, tyb = threadIdx.x >> 5;
  double m1[kRows], m2[kRows], e12[kRows];
  ls_rows<3>(sa, sb, sh, p, gscale);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int oy = tyb + 8 * j;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int k = 0; k <= 2 * r; ++k) {
      const double w = (double)p.g[k] * gscale;
      const int ly = oy + off + k;
      a = fma(w, sh[0][ly][tx], a), b = fma(w, sh[1][ly][tx], b), c = fma(w, sh[2][ly][tx], c);
    }
    m1[j] = a, m2[j] = b, e12[j] = c;
  }
  __syncthreads();  // the row buffer is free again
  ls_rows<2>(sa, sb, sh, p, gscale);
  __syncthreads();
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int oy = tyb + 8 * j, y = ty0 + oy, x = tx0 + tx;
    double e11 = 0.0, e22 = 0.0;
    for (int k = 0; k <= 2 * r; ++k) {
      const double w = (double)p.g[k] * gscale;
      const int ly = oy + off + k;
      e11 = fma(w, sh[0][ly][tx], e11), e22 = fma(w, sh[1][ly][tx], e22);
    }
    if (y < H && x < W) {  // metric.py:139-163
      const double m11 = m1[j] * m1[j], m22 = m2[j] * m2[j], m12 = m1[j] * m2[j];
      const double A1 = 2.0 * m12 + C1, B1 = m11 + m22 + C1;
      const double A2 = 2.0 * (e12[j] - m12) + C2, B2 = (e11 - m11) + (e22 - m22) + C2;
      const double T = A2 / B2;
      sum_s += A1 / B1 * T, sum_c += T;
    }
  }
}

// the workgroup's term sums and count: ms_write_pair's reduction on five values
__device__ __forceinline__ void ls_write_terms(double (&v)[kLsTerms], double (&sred)[4][kLsTerms], double* out) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kLsTerms; ++k) v[k] += __shfl_xor(v[k], off, 64);
  }
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int k = 0; k < kLsTerms; ++k) sred[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)kLsTerms) {
    const unsigned k = threadIdx.x;
    out[k] = (sred[0][k] + sred[1][k]) + (sred[2][k] + sred[3][k]);
  }
}

// level 0, from the bytes.  Launched with 256 lanes on the plan's level-0 grid.  partial: level 0's first pair; terms: the
// first workgroup's five term sums.
__global__ __launch_bounds__(256) void loss_ragged_bytes_kernel(SsimArgs win, const int* plan, const uint8_t* a_arena, const uint8_t* b_arena,
                                                                const uint8_t* mask_arena, unsigned char* workspace, double* partial,
                                                                double* terms, unsigned long long a_bytes, unsigned long long b_bytes,
                                                                unsigned long long mask_bytes, unsigned long long planes_bytes,
                                                                unsigned long long hash, unsigned stamp, unsigned B, double gscale) {
  const MsRaggedArgs p{plan, a_arena, b_arena, mask_arena, workspace, partial, a_bytes, b_bytes, mask_bytes, planes_bytes, hash, stamp, B};
  __shared__ MsIn sa, sb;  // the two L tiles
  __shared__ LsRow sh;     // the float64 row buffer; before the L tiles exist, the staged bytes
  LsBytes& s8 = *reinterpret_cast<LsBytes*>(&sh);
  __shared__ double sred[4][2];
  __shared__ double sterm[4][kLsTerms];
  // 1. whose plan is this?  A stale or foreign one: no output at all
  if (ragged_word(p.plan, MH_STAMP) != p.stamp || ragged_word64(p.plan, MH_HASH) != p.hash) return;

  // 2. the workgroup's image
  const unsigned wg = blockIdx.x;
  const int* d = ms_find(p.plan, p.B, 0u, wg);
  const MsLevel v = ms_level(d, 0u), n = ms_level(d, 1u);
  const unsigned chunk = wg - v.first;
  const unsigned long long rgb_off = ragged_word64(d, MD_RGB_OFF), mask_off = ragged_word64(d, MD_MASK_OFF);

  // 3. the descriptor's extents against the three arenas and the workspace, before any address is formed.  Workgroup-uniform.
  const unsigned long long px = (unsigned long long)v.h * v.w;
  bool ok = ms_level_ok(v, chunk) && ms_halves(v, n) && ls_planes_ok(n, p.planes_bytes);
  ok = ok && rgb_off <= p.a_bytes && px * 3u <= p.a_bytes - rgb_off && rgb_off <= p.b_bytes && px * 3u <= p.b_bytes - rgb_off;
  ok = ok && (!p.mask || (mask_off <= p.mask_bytes && px <= p.mask_bytes - mask_off));

  double sum_s = 0.0, sum_c = 0.0;
  double acc[kLsTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (ok) {
    const int H = (int)v.h, W = (int)v.w, tx0 = (int)(chunk % v.tiles_x) * SSIM_TILE, ty0 = (int)(chunk / v.tiles_x) * SSIM_TILE;
    const uint8_t* pa = p.a + rgb_off;
    const uint8_t* pb = p.b + rgb_off;
    const uint8_t* pm = p.mask ? p.mask + mask_off : nullptr;
    // 4. the tile + halo as bytes: 6 per pixel, 0 outside the image and where the mask byte is 0 (model.py:90's `* mask`)
    for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += 256) {
      const int ly = i / SSIM_IN, lx = i - ly * SSIM_IN, y = ty0 + ly - SSIM_R, x = tx0 + lx - SSIM_R;
      unsigned a0 = 0u, a1 = 0u, a2 = 0u, b0 = 0u, b1 = 0u, b2 = 0u;
      if ((y >= 0) & (y < H) & (x >= 0) & (x < W)) {
        const size_t q = (size_t)y * W + x;
        if (!pm || pm[q] != 0) a0 = pa[3 * q], a1 = pa[3 * q + 1], a2 = pa[3 * q + 2], b0 = pb[3 * q], b1 = pb[3 * q + 1], b2 = pb[3 * q + 2];
      }
      s8[0][0][ly][lx] = (unsigned char)a0, s8[0][1][ly][lx] = (unsigned char)a1, s8[0][2][ly][lx] = (unsigned char)a2;
      s8[1][0][ly][lx] = (unsigned char)b0, s8[1][1][ly][lx] = (unsigned char)b1, s8[1][2][ly][lx] = (unsigned char)b2;
    }
    __syncthreads();
    // 5. the tile's own pixels, four per lane ONE AFTER THE OTHER (loss.inc says what interleaved chains cost in VGPRs): the
    //    four terms, the count and the two L values.  A masked-out pixel is black on both sides: exact zeros in all four terms.
#pragma unroll 1
    for (int j = 0; j < SSIM_TILE * SSIM_TILE / 256; ++j) {
      const int i = (int)threadIdx.x + 256 * j, ly = SSIM_R + i / SSIM_TILE, lx = SSIM_R + i % SSIM_TILE;
      const int y = ty0 + ly - SSIM_R, x = tx0 + lx - SSIM_R;
      float lp = 0.0f, lt = 0.0f;  // outside the image: conv2d's padding
      if (y < H && x < W) {
        const float m = (!pm || pm[(size_t)y * W + x] != 0) ? 1.0f : 0.0f;  // data.py:190's `mask > 0`
        const LossPx o = loss_terms(ls_px(s8, 0, ly, lx), ls_px(s8, 1, ly, lx), m);
        acc[0] += (double)o.rgb_l1, acc[1] += (double)o.cos_sim, acc[2] += (double)o.lab_l1, acc[3] += (double)o.hsv_l1;
        acc[4] += (double)m;
        lp = o.Lp, lt = o.Lt;
      }
      sa[ly][lx] = lp, sb[ly][lx] = lt;
    }
    // 6. the halo ring: the two L values alone, by the converter loss_terms runs (rgb2lab on prediction and on target)
    for (int r = threadIdx.x; r < kLsRing; r += 256) {
      int ly, lx;
      if (r < 2 * SSIM_R * SSIM_IN) {  // the rows above and below the tile, full width
        const int row = r / SSIM_IN;
        ly = row < SSIM_R ? row : row + SSIM_TILE, lx = r - row * SSIM_IN;
      } else {                         // the columns left and right of it
        const int q = r - 2 * SSIM_R * SSIM_IN, row = q / (2 * SSIM_R), c = q - row * (2 * SSIM_R);
        ly = SSIM_R + row, lx = c < SSIM_R ? c : c + SSIM_TILE;
      }
      const int y = ty0 + ly - SSIM_R, x = tx0 + lx - SSIM_R;
      float lp = 0.0f, lt = 0.0f;
      if ((y >= 0) & (y < H) & (x >= 0) & (x < W)) {
        lp = clamp01(rgb2lab(ls_px(s8, 0, ly, lx)).c0), lt = clamp01(rgb2lab(ls_px(s8, 1, ly, lx)).c0);
      }
      sa[ly][lx] = lp, sb[ly][lx] = lt;
    }
    __syncthreads();  // (the staged bytes are dead from here: the row buffer takes their place)
    // 7. the window passes on the one channel, and the level-1 planes' piece
    float* next = reinterpret_cast<float*>(p.ws + n.planes);  // prediction L [h/2][w/2], then target L
    ls_ssim_plane(sa, sb, sh, win, gscale, ty0, tx0, H, W, sum_s, sum_c);
    ms_pool_store(sa, sb, next, next + (size_t)n.h * n.w, ty0, tx0, (int)n.h, (int)n.w);
  }
  ms_write_pair(sum_s, sum_c, sred, p.partial + 2 * (size_t)wg);  // (every thread is here: `ok` is workgroup-uniform)
  ls_write_terms(acc, sterm, terms + kLsTerms * (size_t)wg);
}

// levels 1..4 (win.level), on the workspace's two float planes per level: msssim_ragged_level_kernel on one channel.  Launched
// with 256 lanes on the plan's grid of that level.
__global__ __launch_bounds__(256) void loss_ragged_level_kernel(SsimArgs win, const int* plan, unsigned char* workspace, double* partial,
                                                                unsigned long long planes_bytes, unsigned long long hash, unsigned stamp,
                                                                unsigned B, double gscale) {
  __shared__ MsIn sa, sb;
  __shared__ LsRow sh;
  __shared__ double sred[4][2];
  if (ragged_word(plan, MH_STAMP) != stamp || ragged_word64(plan, MH_HASH) != hash) return;

  const unsigned wg = blockIdx.x, level = (unsigned)win.level;
  const bool has_next = level + 1u < (unsigned)kMsLevels;
  const int* d = ms_find(plan, B, level, wg);
  const MsLevel v = ms_level(d, level), n = ms_level(d, has_next ? level + 1u : level);
  const unsigned chunk = wg - v.first;
  bool ok = level >= 1u && level < (unsigned)kMsLevels && ms_level_ok(v, chunk) && ls_planes_ok(v, planes_bytes);
  ok = ok && (!has_next || (ms_halves(v, n) && ls_planes_ok(n, planes_bytes)));

  double sum_s = 0.0, sum_c = 0.0;
  if (ok) {
    const int H = (int)v.h, W = (int)v.w, tx0 = (int)(chunk % v.tiles_x) * SSIM_TILE, ty0 = (int)(chunk / v.tiles_x) * SSIM_TILE;
    const float* pa = reinterpret_cast<const float*>(workspace + v.planes);
    const float* pb = pa + (size_t)v.h * v.w;
    float* next = reinterpret_cast<float*>(workspace + n.planes);
    for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += 256) {  // tile + halo, zero outside the image (conv2d padding)
      const int ly = i / SSIM_IN, lx = i - ly * SSIM_IN, y = ty0 + ly - SSIM_R, x = tx0 + lx - SSIM_R;
      const bool in = (y >= 0) & (y < H) & (x >= 0) & (x < W);
      sa[ly][lx] = in ? pa[(size_t)y * W + x] : 0.0f;
      sb[ly][lx] = in ? pb[(size_t)y * W + x] : 0.0f;
    }
    __syncthreads();
    ls_ssim_plane(sa, sb, sh, win, gscale, ty0, tx0, H, W, sum_s, sum_c);
    if (has_next) ms_pool_store(sa, sb, next, next + (size_t)n.h * n.w, ty0, tx0, (int)n.h, (int)n.w);
  }
  ms_write_pair(sum_s, sum_c, sred, partial + 2 * (size_t)wg);
}

// one fixed-order float64 sum over the workgroup's 256 lanes (s: 256 doubles of LDS, free again on return)
__device__ __forceinline__ double ls_tree_sum(double a, double* s) {
  s[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// the finish.  Workgroup j takes descriptor j.  stats: [B][3][5]: row 0 the fixed-order sums of its level-0 tiles' four terms
// and count, rows 1 / 2 per level the means over the level's h*w values of the SSIM and the contrast-structure map
// (msssim_ragged_finish_kernel's walk).  pairs / tiles0 are the HOST plan's counts of pairs and of level-0 workgroups: what
// lies outside them is not read, and its figures are NaN.  Launched with 256 lanes.
__global__ __launch_bounds__(256) void loss_ragged_finish_kernel(const int* plan, const double* partial, const double* terms, double* stats,
                                                                 unsigned long long hash, unsigned stamp, unsigned B, unsigned pairs,
                                                                 unsigned tiles0) {
  __shared__ double s0[256];
  if (ragged_word(plan, MH_STAMP) != stamp || ragged_word64(plan, MH_HASH) != hash) return;
  const int* d = plan + kMsHeaderWords + blockIdx.x * kMsDescWords;
  const unsigned index = ragged_word(d, MD_INDEX);
  if (index >= B) return;
  double* out = stats + (size_t)index * 3 * kMsLevels;
  {
    const MsLevel v = ms_level(d, 0u);
    const bool ok = v.first <= tiles0 && v.tiles <= tiles0 - v.first;
    const double* q = terms + kLsTerms * (size_t)v.first;
#pragma unroll 1
    for (int k = 0; k < kLsTerms; ++k) {
      double a = 0.0;
      if (ok)
        for (unsigned t = threadIdx.x; t < v.tiles; t += 256u) a += q[kLsTerms * (size_t)t + k];
      const double r = ls_tree_sum(a, s0);
      if (threadIdx.x == 0u) out[k] = ok ? r : __builtin_nan("");
    }
  }
#pragma unroll 1
  for (int l = 0; l < kMsLevels; ++l) {
    const MsLevel v = ms_level(d, (unsigned)l);
    const unsigned pair = ragged_word(d, kMsLevelWord + (unsigned)l * kMsLevelWords + ML_PAIR);
    const bool ok = v.h >= 1u && v.w >= 1u && (unsigned long long)v.h * v.w <= (1ull << 30) && pair <= pairs && v.tiles <= pairs - pair;
    double a = 0.0, b = 0.0;
    if (ok) {
      const double* q = partial + 2 * (size_t)pair;
      for (unsigned t = threadIdx.x; t < v.tiles; t += 256u) a += q[2 * (size_t)t], b += q[2 * (size_t)t + 1];
    }
    const double ra = ls_tree_sum(a, s0), rb = ls_tree_sum(b, s0);
    if (threadIdx.x == 0u) {
      const double inv = ok ? 1.0 / ((double)v.h * v.w) : __builtin_nan("");
      out[kMsLevels + l] = ra * inv, out[2 * kMsLevels + l] = rb * inv;
    }
  }
}
