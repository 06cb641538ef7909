// msssim_ragged.inc -- part of curl_kernels.hip (one translation unit; included after msssim.inc, whose tile constants it
// uses, and stream_ragged.inc, whose ragged_word it uses; not compiled alone).
// ------------------------------------------------------------------------------------------------
// the MS-SSIM statistics of a batch of byte images of different sizes (include/curl_hip_ragged_msssim.h)
// ------------------------------------------------------------------------------------------------
// Six launches for the whole batch, whatever B is:
//   level 0     the grid is the sum of the images' 32x32 tiles.  A workgroup finds its image as stream_ragged_kernel does
//               (stamp and hash, the scalar binary search over the running sums, the descriptor's extents against all three
//               arenas and the workspace, all before an address is formed), stages its tile plus the 5-pixel halo of a and b
//               as BYTES (zero outside the image and where the mask byte is 0: the neighbouring image in the arena never
//               reaches a halo) and, per channel, turns them into the float tile msssim_level_kernel stages -- the rest is
//               that kernel's arithmetic: the separable window over a, b, a^2, b^2, ab, the (co)variances with contraction
//               off, and the 16x16 piece of the level-1 planes.  No full-resolution float image is written.
//   levels 1-4  the same walk on the workspace's float planes, one launch per level, each writing the next but the last.
//   finish      B workgroups: each sums its image's pairs per level in a fixed order and writes the ten means.
// A workgroup writes ONE pair of float64 (sum of the SSIM map, sum of the contrast-structure map over its tile's three
// channels): zeros when its descriptor fails a check, so the finish never reads a word nobody wrote; a stale or foreign
// plan writes nothing at all.  No atomics, no memset; every sum in a fixed order.
constexpr unsigned kMsStamp = 0x4D535231u, kMsOp = 5u;
constexpr unsigned kMsHeaderWords = 32, kMsDescWords = 64, kMsLevelWord = 16, kMsLevelWords = 8;
constexpr int kMsLevels = 5;
enum {  // header words
  MH_STAMP = 0, MH_B, MH_OP, MH_HAS_MASK, MH_LAUNCHES, MH_GRID0 = 5, MH_RGB_BYTES = 12, MH_MASK_BYTES = 14, MH_WS_BYTES = 16,
  MH_HASH = 18, MH_PARTIAL_OFF = 20, MH_PAIR0 = 22
};
enum { MD_INDEX = 0, MD_H, MD_W, MD_RGB_OFF = 4, MD_MASK_OFF = 6 };                  // descriptor words
enum { ML_H = 0, ML_W, ML_TILES_X, ML_TILES, ML_FIRST, ML_PAIR, ML_PLANES = 6 };   // words of a descriptor's level
static_assert(kMsLevelWord + kMsLevels * kMsLevelWords <= kMsDescWords, "five levels fit a descriptor");

// (the kernels take the fields one by one, as stream_ragged_kernel does: scalars and pointers only beside the SsimArgs that
// carries the window -- its g, radius and level are what is read of it)
struct MsRaggedArgs {
  const int* plan;       // the device copy of the plan
  const uint8_t* a;      // the three arenas (level 0 only; mask: NULL = every pixel)
  const uint8_t* b;
  const uint8_t* mask;
  unsigned char* ws;     // the workspace: float planes of levels 1..4 in [0, planes_bytes)
  double* partial;       // THIS level's first pair
  unsigned long long a_bytes, b_bytes, mask_bytes, planes_bytes;
  unsigned long long hash;  // the HOST plan's
  unsigned stamp, B;
};

struct MsLevel {
  unsigned h, w, tiles_x, tiles, first;
  unsigned long long planes;
};
__device__ __forceinline__ MsLevel ms_level(const int* d, unsigned l) {
  const unsigned o = kMsLevelWord + l * kMsLevelWords;
  return MsLevel{ragged_word(d, o + ML_H), ragged_word(d, o + ML_W), ragged_word(d, o + ML_TILES_X), ragged_word(d, o + ML_TILES),
                 ragged_word(d, o + ML_FIRST), ragged_word64(d, o + ML_PLANES)};
}
// the workgroup's image at a level: the last descriptor whose first workgroup is <= wg (scalar throughout)
__device__ __forceinline__ const int* ms_find(const int* plan, unsigned B, unsigned level, unsigned wg) {
  const int* tab = plan + kMsHeaderWords;
  const unsigned word = kMsLevelWord + level * kMsLevelWords + ML_FIRST;
  unsigned lo = 0, hi = B;
  while (hi - lo > 1u) {
    const unsigned mid = (lo + hi) >> 1;
    if (ragged_word(tab, mid * kMsDescWords + word) <= wg) lo = mid;
    else hi = mid;
  }
  return tab + lo * kMsDescWords;
}
// a level's size and tiling hang together, and `chunk` is one of its tiles
__device__ __forceinline__ bool ms_level_ok(const MsLevel& v, unsigned chunk) {
  return v.h >= 1u && v.w >= 1u && (unsigned long long)v.h * v.w <= (1ull << 30) && v.tiles_x == (v.w + SSIM_TILE - 1u) / SSIM_TILE &&
         v.tiles == v.tiles_x * ((v.h + SSIM_TILE - 1u) / SSIM_TILE) && chunk < v.tiles;
}
// a level's six float planes lie inside the workspace's plane region
__device__ __forceinline__ bool ms_planes_ok(const MsLevel& v, unsigned long long planes_bytes) {
  return v.planes % 4u == 0u && v.planes <= planes_bytes && 24ull * v.h * v.w <= planes_bytes - v.planes;
}
__device__ __forceinline__ bool ms_halves(const MsLevel& v, const MsLevel& n) { return n.h == v.h / 2u && n.w == v.w / 2u && n.h >= 1u && n.w >= 1u; }

typedef float MsIn[SSIM_IN][SSIM_IN + 1];
typedef float MsRow[5][SSIM_IN][SSIM_TILE + 1];

// msssim_level_kernel's two passes on a staged tile of one plane: adds the tile's SSIM and contrast-structure values to
// the thread's sums.  The caller has a barrier behind the staging; one more is taken here between the passes.
__device__ __forceinline__ void ms_ssim_plane(const MsIn& sa, const MsIn& sb, MsRow& sh, const SsimArgs& p, int ty0, int tx0, int H,
                                              int W, double& sum_s, double& sum_c) {
  const int r = p.radius, off = SSIM_R - r;
  for (int i = threadIdx.x; i < SSIM_IN * SSIM_TILE; i += 256) {  // horizontal pass, all five quantities
    int ly = i / SSIM_TILE, cx = i - ly * SSIM_TILE;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f;
    for (int k = 0; k <= 2 * r; ++k) {
      float w = p.g[k], va = sa[ly][cx + off + k], vb = sb[ly][cx + off + k];
      s1 = fmaf(w, va, s1), s2 = fmaf(w, vb, s2);
      s3 = fmaf(w, va * va, s3), s4 = fmaf(w, vb * vb, s4), s5 = fmaf(w, va * vb, s5);
    }
    sh[0][ly][cx] = s1, sh[1][ly][cx] = s2, sh[2][ly][cx] = s3, sh[3][ly][cx] = s4, sh[4][ly][cx] = s5;
  }
  __syncthreads();
  const int tx = threadIdx.x & 31, tyb = threadIdx.x >> 5;
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
  for (int j = 0; j < SSIM_TILE / 8; ++j) {
    const int oy = tyb + 8 * j, y = ty0 + oy, x = tx0 + tx;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
    for (int k = 0; k <= 2 * r; ++k) {
      float w = p.g[k];
      const int ly = oy + off + k;
      m1 = fmaf(w, sh[0][ly][tx], m1), m2 = fmaf(w, sh[1][ly][tx], m2);
      e11 = fmaf(w, sh[2][ly][tx], e11), e22 = fmaf(w, sh[3][ly][tx], e22), e12 = fmaf(w, sh[4][ly][tx], e12);
    }
    if (y < H && x < W) {
      // metric.py:139-163, as msssim_level_kernel forms it
      float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
      float A1 = 2.0f * m12 + C1, B1 = m11 + m22 + C1;
      float s11, s22, s12;
      {
        // blur minus the ROUNDED product of the means (metric.py:143-145): contracted into an fma, a variance that is 0 comes
        // out as the rounding residue of the product, against C2 = 9e-4 (msssim.inc says what that cost)
#pragma clang fp contract(off)
        s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
      }
      float A2 = 2.0f * s12 + C2, B2 = s11 + s22 + C2;
      float rB1 = 1.0f / B1, rB2 = 1.0f / B2;
      float T = A2 * rB2, S = A1 * rB1 * T;
      sum_s += (double)S, sum_c += (double)T;
    }
  }
}

// the tile's 16x16 piece of the next level: F.avg_pool2d(x, (2, 2)), floor sizes (metric.py:191-192)
__device__ __forceinline__ void ms_pool_store(const MsIn& sa, const MsIn& sb, float* a_next, float* b_next, int ty0, int tx0, int Hn, int Wn) {
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const int y = ty0 / 2 + py, x = tx0 / 2 + px;
  if (y < Hn && x < Wn) {
    const int ly = SSIM_R + 2 * py, lx = SSIM_R + 2 * px;
    const size_t o = (size_t)y * Wn + x;
    a_next[o] = ((sa[ly][lx] + sa[ly][lx + 1]) + (sa[ly + 1][lx] + sa[ly + 1][lx + 1])) * 0.25f;
    b_next[o] = ((sb[ly][lx] + sb[ly][lx + 1]) + (sb[ly + 1][lx] + sb[ly + 1][lx + 1])) * 0.25f;
  }
}

// the workgroup's pair: the wave's sums by xor shuffles, the four waves' through LDS, in a fixed order
__device__ __forceinline__ void ms_write_pair(double s, double c, double (&sred)[4][2], double* pair) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64), c += __shfl_xor(c, off, 64);
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) sred[wave][0] = s, sred[wave][1] = c;
  __syncthreads();
  if (threadIdx.x == 0u) pair[0] = (sred[0][0] + sred[1][0]) + (sred[2][0] + sred[3][0]), pair[1] = (sred[0][1] + sred[1][1]) + (sred[2][1] + sred[3][1]);
}

// level 0, from the bytes.  Launched with 256 lanes on the plan's level-0 grid.
__global__ __launch_bounds__(256) void msssim_ragged_bytes_kernel(SsimArgs win, const int* plan, const uint8_t* a_arena, const uint8_t* b_arena,
                                                                  const uint8_t* mask_arena, unsigned char* workspace, double* partial,
                                                                  unsigned long long a_bytes, unsigned long long b_bytes,
                                                                  unsigned long long mask_bytes, unsigned long long planes_bytes,
                                                                  unsigned long long hash, unsigned stamp, unsigned B) {
  const MsRaggedArgs p{plan, a_arena, b_arena, mask_arena, workspace, partial, a_bytes, b_bytes, mask_bytes, planes_bytes, hash, stamp, B};
  __shared__ unsigned char s8[2][3][SSIM_IN][SSIM_IN + 2];  // a / b, channel, the tile + halo; masked-out and outside pixels 0
  __shared__ MsIn sa, sb;
  __shared__ MsRow sh;
  __shared__ double sred[4][2];
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
  bool ok = ms_level_ok(v, chunk) && ms_halves(v, n) && ms_planes_ok(n, p.planes_bytes);
  ok = ok && rgb_off <= p.a_bytes && px * 3u <= p.a_bytes - rgb_off && rgb_off <= p.b_bytes && px * 3u <= p.b_bytes - rgb_off;
  ok = ok && (!p.mask || (mask_off <= p.mask_bytes && px <= p.mask_bytes - mask_off));

  double sum_s = 0.0, sum_c = 0.0;
  if (ok) {
    const int H = (int)v.h, W = (int)v.w, tx0 = (int)(chunk % v.tiles_x) * SSIM_TILE, ty0 = (int)(chunk / v.tiles_x) * SSIM_TILE;
    const uint8_t* pa = p.a + rgb_off;
    const uint8_t* pb = p.b + rgb_off;
    const uint8_t* pm = p.mask ? p.mask + mask_off : nullptr;
    // 4. the tile + halo as bytes: 6 per pixel, 0 outside the image (conv2d's padding) and where the mask byte is 0
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
    float* next = reinterpret_cast<float*>(p.ws + n.planes);  // a's three planes [3][h/2][w/2], then b's
    const size_t npx = (size_t)n.h * n.w;
    for (int c = 0; c < 3; ++c) {
      // 5. the channel's float tile: byte / 255 correctly rounded (to_tensor's quotient; a multiply by 1/255 is another number)
      for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += 256) {
        const int ly = i / SSIM_IN, lx = i - ly * SSIM_IN;
        sa[ly][lx] = u8_to_unit((float)s8[0][c][ly][lx]), sb[ly][lx] = u8_to_unit((float)s8[1][c][ly][lx]);
      }
      __syncthreads();
      ms_ssim_plane(sa, sb, sh, win, ty0, tx0, H, W, sum_s, sum_c);
      ms_pool_store(sa, sb, next + c * npx, next + (3 + c) * npx, ty0, tx0, (int)n.h, (int)n.w);
      __syncthreads();  // sa / sb / sh are free again
    }
  }
  ms_write_pair(sum_s, sum_c, sred, p.partial + 2 * (size_t)wg);  // (every thread is here: `ok` is workgroup-uniform)
}

// levels 1..4 (win.level), on the workspace's float planes: msssim_level_kernel<false> with the plan walk.  Launched with 256
// lanes on the plan's grid of that level.
__global__ __launch_bounds__(256) void msssim_ragged_level_kernel(SsimArgs win, const int* plan, unsigned char* workspace, double* partial,
                                                                  unsigned long long planes_bytes, unsigned long long hash, unsigned stamp,
                                                                  unsigned B) {
  const MsRaggedArgs p{plan, nullptr, nullptr, nullptr, workspace, partial, 0ull, 0ull, 0ull, planes_bytes, hash, stamp, B};
  __shared__ MsIn sa, sb;
  __shared__ MsRow sh;
  __shared__ double sred[4][2];
  if (ragged_word(p.plan, MH_STAMP) != p.stamp || ragged_word64(p.plan, MH_HASH) != p.hash) return;

  const unsigned wg = blockIdx.x, level = (unsigned)win.level;
  const bool has_next = level + 1u < (unsigned)kMsLevels;
  const int* d = ms_find(p.plan, p.B, level, wg);
  const MsLevel v = ms_level(d, level), n = ms_level(d, has_next ? level + 1u : level);
  const unsigned chunk = wg - v.first;
  bool ok = level >= 1u && level < (unsigned)kMsLevels && ms_level_ok(v, chunk) && ms_planes_ok(v, p.planes_bytes);
  ok = ok && (!has_next || (ms_halves(v, n) && ms_planes_ok(n, p.planes_bytes)));

  double sum_s = 0.0, sum_c = 0.0;
  if (ok) {
    const int H = (int)v.h, W = (int)v.w, tx0 = (int)(chunk % v.tiles_x) * SSIM_TILE, ty0 = (int)(chunk / v.tiles_x) * SSIM_TILE;
    const float* cur = reinterpret_cast<const float*>(p.ws + v.planes);
    float* next = reinterpret_cast<float*>(p.ws + n.planes);
    const size_t cpx = (size_t)v.h * v.w, npx = (size_t)n.h * n.w;
    for (int c = 0; c < 3; ++c) {
      const float* pa = cur + c * cpx;
      const float* pb = cur + (3 + c) * cpx;
      for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += 256) {  // tile + halo, zero outside the image (conv2d padding)
        const int ly = i / SSIM_IN, lx = i - ly * SSIM_IN, y = ty0 + ly - SSIM_R, x = tx0 + lx - SSIM_R;
        const bool in = (y >= 0) & (y < H) & (x >= 0) & (x < W);
        sa[ly][lx] = in ? pa[(size_t)y * W + x] : 0.0f;
        sb[ly][lx] = in ? pb[(size_t)y * W + x] : 0.0f;
      }
      __syncthreads();
      ms_ssim_plane(sa, sb, sh, win, ty0, tx0, H, W, sum_s, sum_c);
      if (has_next) ms_pool_store(sa, sb, next + c * npx, next + (3 + c) * npx, ty0, tx0, (int)n.h, (int)n.w);
      __syncthreads();
    }
  }
  ms_write_pair(sum_s, sum_c, sred, p.partial + 2 * (size_t)wg);
}

// the finish.  Workgroup j takes descriptor j: per level the fixed-order float64 sum of its tiles' pairs -> the two means over
// the level's 3*h*w values.  partial: the first pair of level 0; stats: [B][2][5]; pairs is the HOST plan's count of pairs: a
// level's pairs [pair, pair + tiles) lie inside it or the level's means are NaN and nothing is read.  Launched with 256 lanes.
__global__ __launch_bounds__(256) void msssim_ragged_finish_kernel(const int* plan, const double* partial, double* stats,
                                                                   unsigned long long hash, unsigned stamp, unsigned B, unsigned pairs) {
  __shared__ double s0[256], s1[256];
  if (ragged_word(plan, MH_STAMP) != stamp || ragged_word64(plan, MH_HASH) != hash) return;
  const int* d = plan + kMsHeaderWords + blockIdx.x * kMsDescWords;
  const unsigned index = ragged_word(d, MD_INDEX);
  if (index >= B) return;
#pragma unroll
  for (int l = 0; l < kMsLevels; ++l) {
    const MsLevel v = ms_level(d, (unsigned)l);
    const unsigned pair = ragged_word(d, kMsLevelWord + (unsigned)l * kMsLevelWords + ML_PAIR);
    const bool ok = v.h >= 1u && v.w >= 1u && (unsigned long long)v.h * v.w <= (1ull << 30) && pair <= pairs && v.tiles <= pairs - pair;
    double a = 0.0, b = 0.0;
    if (ok) {
      const double* q = partial + 2 * (size_t)pair;
      for (unsigned t = threadIdx.x; t < v.tiles; t += 256u) a += q[2 * (size_t)t], b += q[2 * (size_t)t + 1];
    }
    s0[threadIdx.x] = a, s1[threadIdx.x] = b;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) s0[threadIdx.x] += s0[threadIdx.x + off], s1[threadIdx.x] += s1[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0u) {
      const double inv = ok ? 1.0 / (3.0 * v.h * v.w) : __builtin_nan("");
      stats[((size_t)index * 2) * kMsLevels + l] = s0[0] * inv;
      stats[((size_t)index * 2 + 1) * kMsLevels + l] = s1[0] * inv;
    }
    __syncthreads();  // s0 / s1 are free again
  }
}
