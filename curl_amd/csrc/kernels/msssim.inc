// msssim.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// MS-SSIM statistics  (metric.py:120-208: compute_ssim per pyramid level, avg_pool2d between levels)
// ------------------------------------------------------------------------------------------------
// The reference runs five grouped conv2d per level (blur of a, b, a*a, b*b, a*b with a ws x ws Gaussian, zero
// padding), forms the SSIM / contrast-structure maps and averages them per image, then halves both images.  Here a
// block owns a 32x32 tile of one plane: the tile and its halo go to LDS once, the window is applied separably
// (it is an outer product, metric.py:99-101) -- a horizontal pass into LDS, a vertical pass into registers -- for
// all five quantities together, the two maps are reduced per block (fixed-order float64 second pass, no atomics),
// and the same block writes its 16x16 piece of the next level.  Backward mode writes, instead of the sums, the
// three per-pixel derivative maps dL/d(mu1), dL/d(E[a^2]), dL/d(E[ab]); msssim_grad_kernel blurs them (the
// transpose of a symmetric zero-padded blur is the same blur) and adds the avg_pool2d gradient from the level below.
#define SSIM_TILE 32
#define SSIM_R 5                           // largest supported radius: window_size <= 11
#define SSIM_IN (SSIM_TILE + 2 * SSIM_R)   // 42
struct SsimArgs {
  const float* a;       // [N][H][W] this level, N = B*C planes
  const float* b;
  float* a_next;        // [N][H/2][W/2] or NULL (last level / backward)
  float* b_next;
  float* partial;       // forward: [N][tiles][2] (sum ssim_map, sum cs_map)
  const float* g_ssim;  // backward: [B][levels] dL/d(mean ssim), dL/d(mean cs)
  const float* g_cs;
  float* d_mu;          // backward: [N][H][W] x 3
  float* d_e11;
  float* d_e12;
  int H, W, C, level, levels, radius;
  unsigned tiles_x, tiles;
  float g[2 * SSIM_R + 1];  // 1-D window, g[0..2*radius]
};

template <bool BACKWARD>
__global__ __launch_bounds__(256) void msssim_level_kernel(SsimArgs p) {
  __shared__ float sa[SSIM_IN][SSIM_IN + 1], sb[SSIM_IN][SSIM_IN + 1];
  __shared__ float sh[5][SSIM_IN][SSIM_TILE + 1];
  __shared__ float sred[2][4];
  const int n = blockIdx.y, tile = blockIdx.x, tx0 = (tile % p.tiles_x) * SSIM_TILE, ty0 = (tile / p.tiles_x) * SSIM_TILE;
  const int H = p.H, W = p.W, r = p.radius, off = SSIM_R - r;
  const float* pa = p.a + (size_t)n * H * W;
  const float* pb = p.b + (size_t)n * H * W;
  for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += 256) {  // tile + halo, zero outside the image (conv2d padding)
    int ly = i / SSIM_IN, lx = i - ly * SSIM_IN, y = ty0 + ly - SSIM_R, x = tx0 + lx - SSIM_R;
    bool in = (y >= 0) & (y < H) & (x >= 0) & (x < W);
    sa[ly][lx] = in ? pa[(size_t)y * W + x] : 0.0f;
    sb[ly][lx] = in ? pb[(size_t)y * W + x] : 0.0f;
  }
  __syncthreads();
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
  float sum_s = 0.0f, sum_c = 0.0f, ws = 0.0f, wc = 0.0f;
  if (BACKWARD) {
    const int b = n / p.C;
    const float inv = 1.0f / ((float)p.C * (float)H * (float)W);  // the maps are averaged over dim (1,2,3)
    ws = p.g_ssim[b * p.levels + p.level] * inv;
    wc = p.g_cs[b * p.levels + p.level] * inv;
  }
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
      // metric.py:139-163
      float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
      float A1 = 2.0f * m12 + C1, B1 = m11 + m22 + C1;
      // The (co)variances as the reference forms them (metric.py:143-145): blur minus the ROUNDED product of the means.
      // Contracted into fma(-m1, m1, e11) -- exact product against a rounded blur -- a variance that is 0 (flat regions; any
      // region under window 1, where the blur of a^2 IS round(a * a)) came out as the rounding residue of the product, up to
      // 3e-8 against C2 = 9e-4: the per-level means were 1.2e-5 off on a 2x2 plane, where the oracle's float32 is 7e-8 off.
      float s11, s22, s12;
      {
#pragma clang fp contract(off)
        s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
      }
      float A2 = 2.0f * s12 + C2, B2 = s11 + s22 + C2;
      float rB1 = 1.0f / B1, rB2 = 1.0f / B2;
      float T = A2 * rB2, S = A1 * rB1 * T;
      if (!BACKWARD) {
        sum_s += S, sum_c += T;
      } else {
        // d/d(mu1), d/d(E[a^2]), d/d(E[ab]) of  ws * S + wc * T   (sigma1^2 = E11 - mu1^2, sigma12 = E12 - mu1 mu2)
        float dS_dm1 = (2.0f * m2 * (A2 - A1)) * rB1 * rB2 - S * 2.0f * m1 * (rB1 - rB2);
        float dT_dm1 = (2.0f * m1 * T - 2.0f * m2) * rB2;
        size_t o = (size_t)n * H * W + (size_t)y * W + x;
        p.d_mu[o] = ws * dS_dm1 + wc * dT_dm1;
        p.d_e11[o] = -(ws * S + wc * T) * rB2;
        p.d_e12[o] = 2.0f * (ws * A1 * rB1 + wc) * rB2;
      }
    }
  }
  if (!BACKWARD) {
    // the next pyramid level: F.avg_pool2d(x, (2, 2)), floor sizes (metric.py:191-192)
    if (p.a_next) {
      const int Hn = H / 2, Wn = W / 2, py = threadIdx.x >> 4, px = threadIdx.x & 15;
      const int y = ty0 / 2 + py, x = tx0 / 2 + px;
      if (y < Hn && x < Wn) {
        const int ly = SSIM_R + 2 * py, lx = SSIM_R + 2 * px;
        size_t o = (size_t)n * Hn * Wn + (size_t)y * Wn + x;
        p.a_next[o] = ((sa[ly][lx] + sa[ly][lx + 1]) + (sa[ly + 1][lx] + sa[ly + 1][lx + 1])) * 0.25f;
        p.b_next[o] = ((sb[ly][lx] + sb[ly][lx + 1]) + (sb[ly + 1][lx] + sb[ly + 1][lx + 1])) * 0.25f;
      }
    }
    float v[1][2] = {{sum_s, sum_c}};
    wave_sum_lane63(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) sred[0][wave] = v[0][0], sred[1][wave] = v[0][1];
    __syncthreads();
    if (threadIdx.x < 2)
      p.partial[((size_t)n * p.tiles + tile) * 2 + threadIdx.x] =
          (sred[threadIdx.x][0] + sred[threadIdx.x][1]) + (sred[threadIdx.x][2] + sred[threadIdx.x][3]);
  }
}

// per image and level: fixed-order float64 sum of the tile partials of its C planes -> mean ssim, mean cs
__global__ __launch_bounds__(256) void msssim_means_kernel(const float* partial, float* ssims, float* mcs, unsigned per_image,
                                                           double inv_count, int level, int levels) {
  __shared__ double s0[256], s1[256];
  const float* p = partial + (size_t)blockIdx.x * per_image * 2;
  double a = 0.0, b = 0.0;
  for (unsigned i = threadIdx.x; i < per_image; i += 256) a += (double)p[2 * i], b += (double)p[2 * i + 1];
  s0[threadIdx.x] = a, s1[threadIdx.x] = b;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s0[threadIdx.x] += s0[threadIdx.x + off], s1[threadIdx.x] += s1[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ssims[blockIdx.x * levels + level] = (float)(s0[0] * inv_count);
    mcs[blockIdx.x * levels + level] = (float)(s1[0] * inv_count);
  }
}

// grad_a(level) = blur(d_mu) + 2 a blur(d_e11) + b blur(d_e12) + avg_pool2d^T(grad_a(level + 1))
struct SsimGradArgs {
  const float* a;
  const float* b;
  const float* d_mu;
  const float* d_e11;
  const float* d_e12;
  const float* g_below;  // [N][H/2][W/2] gradient of the next (coarser) level, or NULL
  float* g_out;          // [N][H][W]
  int H, W, radius;
  unsigned tiles_x;
  float g[2 * SSIM_R + 1];
};
__global__ __launch_bounds__(256) void msssim_grad_kernel(SsimGradArgs p) {
  __shared__ float sm[3][SSIM_IN][SSIM_IN + 1];
  __shared__ float sh[3][SSIM_IN][SSIM_TILE + 1];
  const int n = blockIdx.y, tile = blockIdx.x, tx0 = (tile % p.tiles_x) * SSIM_TILE, ty0 = (tile / p.tiles_x) * SSIM_TILE;
  const int H = p.H, W = p.W, r = p.radius, off = SSIM_R - r;
  const size_t plane = (size_t)n * H * W;
  for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += 256) {
    int ly = i / SSIM_IN, lx = i - ly * SSIM_IN, y = ty0 + ly - SSIM_R, x = tx0 + lx - SSIM_R;
    bool in = (y >= 0) & (y < H) & (x >= 0) & (x < W);
    size_t o = plane + (size_t)y * W + x;
    sm[0][ly][lx] = in ? p.d_mu[o] : 0.0f;
    sm[1][ly][lx] = in ? p.d_e11[o] : 0.0f;
    sm[2][ly][lx] = in ? p.d_e12[o] : 0.0f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_IN * SSIM_TILE; i += 256) {
    int ly = i / SSIM_TILE, cx = i - ly * SSIM_TILE;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int k = 0; k <= 2 * r; ++k) {
      float w = p.g[k];
      s0 = fmaf(w, sm[0][ly][cx + off + k], s0), s1 = fmaf(w, sm[1][ly][cx + off + k], s1);
      s2 = fmaf(w, sm[2][ly][cx + off + k], s2);
    }
    sh[0][ly][cx] = s0, sh[1][ly][cx] = s1, sh[2][ly][cx] = s2;
  }
  __syncthreads();
  const int tx = threadIdx.x & 31, tyb = threadIdx.x >> 5;
#pragma unroll
  for (int j = 0; j < SSIM_TILE / 8; ++j) {
    const int oy = tyb + 8 * j, y = ty0 + oy, x = tx0 + tx;
    if (y >= H || x >= W) continue;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    for (int k = 0; k <= 2 * r; ++k) {
      float w = p.g[k];
      const int ly = oy + off + k;
      b0 = fmaf(w, sh[0][ly][tx], b0), b1 = fmaf(w, sh[1][ly][tx], b1), b2 = fmaf(w, sh[2][ly][tx], b2);
    }
    size_t o = plane + (size_t)y * W + x;
    float gval = b0 + 2.0f * p.a[o] * b1 + p.b[o] * b2;
    if (p.g_below) {
      const int Hn = H / 2, Wn = W / 2;
      if ((y >> 1) < Hn && (x >> 1) < Wn) gval += 0.25f * p.g_below[(size_t)n * Hn * Wn + (size_t)(y >> 1) * Wn + (x >> 1)];
    }
    p.g_out[o] = gval;
  }
}
