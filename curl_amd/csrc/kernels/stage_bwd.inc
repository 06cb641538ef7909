// stage_bwd.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// backward of the stand-alone curve ops, converters and fused stages (curl_adjust_*_bwd_f32, curl_*2*_bwd_f32,
// curl_lab_stage_bwd_f32, curl_hsv_stage_bwd_f32)
// ------------------------------------------------------------------------------------------------
// The same two-pass shape as the layer's backward (layer_bwd.inc), for ONE knot segment of 3 or 4 curves: a per-pixel
// kernel recomputes the stage's forward tape in registers (curl_math_bwd.h: adjust3_bwd, adjust_hsv_bwd, lab_stage_bwd,
// hsv_stage_bwd), writes the image gradient and reduces its curves' sums P, Q to one row of block partials (no float
// atomics); a per-image kernel sums the rows in a fixed order in float64 and applies the chain rule to the raw knots.
// The tile -- addressing, the mask protocol, the guarded store of grad_img, the block's row of partials -- is the one
// layer_bwd_kernel uses (bwd_tile.inc).  The pullbacks and the second-pass kernels stay separate: knots_bwd_kernel is tuned
// for the layer's ten curves (1024 threads, knot_bwd5, its loads asked for early) and is benchmarked.
#define STAGE_ADJ3 0  // adjust_rgb / adjust_lab: OpAdjust3 in the forward
#define STAGE_AHSV 1  // adjust_hsv
#define STAGE_LAB 2   // rgb2lab -> adjust3 -> *mask -> lab2rgb
#define STAGE_HSV 3   // rgb2hsv -> adjust_hsv -> *mask -> hsv2rgb
template <int OP>
struct StageCurves {
  static constexpr int kN = (OP == STAGE_AHSV || OP == STAGE_HSV) ? 4 : 3;
};
#define STAGE_NACC_MAX 8  // P[4], Q[4]

template <int OP, bool BINARY, bool GIN>
__device__ __forceinline__ Px stage_pixel_bwd(Px in, float m, const Affine* k, Px g, float* P, float* Q) {
  if constexpr (OP == STAGE_ADJ3) return adjust3_bwd(in, k, g, P, Q);
  else if constexpr (OP == STAGE_AHSV) return adjust_hsv_bwd(in, k, g, P, Q);
  else if constexpr (OP == STAGE_LAB) return lab_stage_bwd<BINARY, GIN>(in, m, k, g, P, Q);
  else return hsv_stage_bwd<BINARY, GIN>(in, m, k, g, P, Q);
}

// One tile per block (bwd_tile.inc).  GIN: d loss / d img is wanted.
template <int OP, int VEC, int MK, bool GIN>
__global__ __launch_bounds__(256) void stage_bwd_kernel(BwdArgs a) {
  typedef typename Pack<VEC>::T T;
  constexpr int NC = StageCurves<OP>::kN, NACC = 2 * NC;
  __shared__ float sPart[4][NACC];
  const unsigned img = blockIdx.y;
  const unsigned chunk = blockIdx.x;
  const unsigned bid = img * a.blocks_per_image + chunk;
  const float* row = a.coef + (size_t)img * a.coef_stride;
  Affine k[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) k[c] = load_affine(row, c);
  BwdTile<VEC, MK, GIN> tile;
  tile.load(a.in, a.gout, a.mask, img, chunk, a.n, a.mask_first);
  float acc[NACC];
#pragma unroll
  for (int c = 0; c < NACC; ++c) acc[c] = 0.0f;
  T y0, y1, y2;
  float dep = 0.0f;
  if (GIN && tile.dead) y0 = T(0.0f), y1 = T(0.0f), y2 = T(0.0f);
  if (!tile.dead)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float m = tile.m(e);
      Px pin = tile.pin(e), gin = tile.gin(e);
      // lanes past the end contribute nothing: their incoming gradient is 0 (the stand-alone curves have no mask to carry it)
      if (!tile.valid()) gin = Px{0.0f, 0.0f, 0.0f}, m = 0.0f;
      // one pixel after the other (bwd_tile.inc, at BwdTile::m)
      asm volatile("" : "+v"(pin.c0), "+v"(pin.c1), "+v"(pin.c2), "+v"(gin.c0), "+v"(gin.c1), "+v"(gin.c2) : "v"(dep));
      // P: each pixel's terms from zero, then one plain add behind a barrier.  `P += g_pre * x` (curve_self_pull,
      // curve_cross_pull) is the compiler's to contract, and it chose per instantiation: with four pixels per lane the GIN
      // and !GIN kernels of the four-curve operators fused different ones of these, and need_grad_img=False moved the knot
      // gradient's last bits (tests/test_gpu_pixel_jacobians.py).  From zero both forms are the rounded product; Q's fmaf is
      // explicit and the same everywhere.  This rests on every pullback adding exactly ONE term per pixel to each P[c]
      // (curve_self_pull and curve_cross_pull, each called once per curve): a second `+=` into the same P[c] within a pixel
      // would be contractable again.
      float pp[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) pp[c] = 0.0f;
      Px gi = stage_pixel_bwd<OP, MK != CURL_MASK_F32, GIN>(pin, m, k, gin, pp, acc + NC);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        asm("" : "+v"(pp[c]));
        acc[c] += pp[c];
      }
      dep = gi.c0;
      if constexpr (GIN) {
        set_lane(y0, e, gi.c0);
        set_lane(y1, e, gi.c1);
        set_lane(y2, e, gi.c2);
      }
    }
  if constexpr (GIN) tile.store(a.gin, row, a.stamp, y0, y1, y2);
  block_row_sum(acc, sPart, a.partial, bid);
}

struct StageKnotsArgs {
  const float* ws;       // prep output (exp'd knots at WS_KNOTS)
  const float* partial;  // [B][blocks_per_image][2 * nc]
  const float* greg;     // nullable [B]
  float* graw;           // [B, KP_TOTAL(K, nc)]
  int K;                 // packed (KP_*)
  unsigned ws_stride, blocks_per_image;
};

// One workgroup per image: fixed-order float64 reduction of the block partials (thread t < kLive walks the floats t,
// t + kLive, ...: always value t % NACC; then the phase sums of a value in phase order -- bit-reproducible), then one thread
// per knot: the chain rule (P, Q, d reg) -> raw knot (curl_math_bwd.h knot_bwd).  torch.chunk's shorter last curve: KP_LAST.
#define STAGE_KNOTS_THREADS 256
template <int NC>
__global__ __launch_bounds__(STAGE_KNOTS_THREADS) void stage_knots_bwd_kernel(StageKnotsArgs a) {
  constexpr int NACC = 2 * NC, kPhases = STAGE_KNOTS_THREADS / NACC, kLive = kPhases * NACC;
  __shared__ double sAcc[kLive];
  __shared__ double sPQ[NACC];
  const unsigned b = blockIdx.x;
  const float* part = a.partial + (size_t)b * a.blocks_per_image * NACC;
  const float* row = a.ws + (size_t)b * a.ws_stride;
  if (threadIdx.x < kLive) sAcc[threadIdx.x] = walk_sum8(part, threadIdx.x, kLive, (size_t)a.blocks_per_image * NACC);
  __syncthreads();
  if (threadIdx.x < NACC) {
    double r = sAcc[threadIdx.x];
    for (int m = 1; m < kPhases; ++m) r += sAcc[threadIdx.x + m * NACC];
    sPQ[threadIdx.x] = r;
  }
  __syncthreads();
  const int K0 = KP_K(a.K), n_all = KP_TOTAL(a.K, NC);
  const double g_reg = a.greg ? (double)a.greg[b] : 0.0;
  const bool row_ok = reinterpret_cast<const unsigned*>(row)[WS_STAMP] == ws_stamp((unsigned)n_all, a.ws_stride);
  for (int i = threadIdx.x; i < n_all; i += STAGE_KNOTS_THREADS) {
    const int local = min(i / K0, NC - 1), kk = i - local * K0;
    const int K = local == NC - 1 ? KP_LAST(a.K) : K0;
    const float g = knot_bwd(row + WS_KNOTS + (i - kk), K, sPQ[local], sPQ[NC + local], g_reg, kk);
    a.graw[(size_t)b * n_all + i] = row_ok ? g : __builtin_nanf("");
  }
}

// Converter backward: a pure pointwise stream (6 planes in, 3 out: 36 B/px), the stand-alone pullbacks of curl_math_bwd.h.
#define CONV_RGB2LAB 0
#define CONV_LAB2RGB 1
#define CONV_RGB2HSV 2
#define CONV_HSV2RGB 3
struct ConvBwdArgs {
  const float* in;
  const float* gout;
  float* gin;
  unsigned n;  // VEC-groups per plane
};
template <int CONV>
__device__ __forceinline__ Px conv_pixel_bwd(Px p, Px g) {
  if constexpr (CONV == CONV_RGB2LAB) return rgb2lab_bwd(p, g);
  else if constexpr (CONV == CONV_LAB2RGB) return lab2rgb_bwd(p, g);
  else if constexpr (CONV == CONV_RGB2HSV) return rgb2hsv_bwd(p, g);
  else return hsv2rgb_bwd(p, g);  // the general form: a stand-alone hsv2rgb's input can be anything
}
template <int CONV, int VEC>
__global__ __launch_bounds__(256) void convert_bwd_kernel(ConvBwdArgs a) {
  typedef typename Pack<VEC>::T T;
  constexpr bool kNT = VEC == 4;
  const unsigned img = blockIdx.y;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  const size_t plane = (size_t)a.n;
  const T* p0 = reinterpret_cast<const T*>(a.in) + (size_t)img * 3 * plane;
  const T* g0 = reinterpret_cast<const T*>(a.gout) + (size_t)img * 3 * plane;
  T* q0 = reinterpret_cast<T*>(a.gin) + (size_t)img * 3 * plane;
  const T x0 = ld<kNT>(at(p0, i)), x1 = ld<kNT>(at(p0 + plane, i)), x2 = ld<kNT>(at(p0 + 2 * plane, i));
  const T w0 = ld<kNT>(at(g0, i)), w1 = ld<kNT>(at(g0 + plane, i)), w2 = ld<kNT>(at(g0 + 2 * plane, i));
  T y0, y1, y2;
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const Px gi = conv_pixel_bwd<CONV>(Px{lane(x0, e), lane(x1, e), lane(x2, e)}, Px{lane(w0, e), lane(w1, e), lane(w2, e)});
    set_lane(y0, e, gi.c0);
    set_lane(y1, e, gi.c1);
    set_lane(y2, e, gi.c2);
  }
  st<kNT>(at(q0, i), y0);
  st<kNT>(at(q0 + plane, i), y1);
  st<kNT>(at(q0 + 2 * plane, i), y2);
}
