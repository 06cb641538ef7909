// layer_bwd.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// backward of the fused layer
// ------------------------------------------------------------------------------------------------
#define BWD_NACC 20  // P[10], Q[10]

// One tile per block (bwd_tile.inc).  Per-pixel reverse mode (curl_math_bwd.h) recomputes the forward
// chain in registers; the 20 per-image curve sums are reduced wave -> LDS -> one row of `partial` per block
// (no float atomics: the second pass sums the rows in a fixed order in float64, so results are reproducible).
constexpr int kBwdWaves = 1;  // waves per SIMD the register allocation is held to (1: unconstrained -- 154 VGPRs, three waves)
// GIN: d loss / d img is wanted (a.gin non-NULL).  Without it -- the training step's case -- the kernel also skips
// RGB2LAB's pullback and its three stores (25 instead of 37 B/px).
template <int VEC, int MK, bool GIN = true>
__global__ __launch_bounds__(256, kBwdWaves) void layer_bwd_kernel(BwdArgs a) {
  typedef typename Pack<VEC>::T T;
  __shared__ float sPart[4][BWD_NACC];
  const unsigned img = blockIdx.y;
  const unsigned chunk = blockIdx.x;
  const unsigned bid = img * a.blocks_per_image + chunk;
  const LayerCoef k = OpLayer::load(a.coef + (size_t)img * a.coef_stride, StreamArgs{});
  BwdTile<VEC, MK, GIN> tile;
  tile.load(a.in, a.gout, a.mask, img, chunk, a.n, a.mask_first);
  float acc[BWD_NACC];
#pragma unroll
  for (int c = 0; c < BWD_NACC; ++c) acc[c] = 0.0f;
  T y0, y1, y2;
  float dep = 0.0f;
  if (GIN && tile.dead) y0 = T(0.0f), y1 = T(0.0f), y2 = T(0.0f);
  if (!tile.dead)
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    float m = tile.m(e);
    Px pin = tile.pin(e), gin = tile.gin(e);
    if (!tile.valid()) m = 0.0f;  // lanes past the end contribute nothing (m multiplies every path to P, Q)
    // one pixel after the other (bwd_tile.inc, at BwdTile::m)
    asm volatile("" : "+v"(pin.c0), "+v"(pin.c1), "+v"(pin.c2), "+v"(gin.c0), "+v"(gin.c1), "+v"(gin.c2) : "v"(dep));
    // bool / uint8 / no mask: m is exactly 0 or 1 (the binary specialisation); the curve sums go straight into `acc`
    Px gi = curl_layer_bwd<MK != CURL_MASK_F32, GIN>(pin, m, k, gin, acc, acc + 10);
    dep = gi.c0;  // (GIN = false: the gradient entering RGB2LAB's pullback -- the end of this pixel's chain just the same)
    if constexpr (GIN) {
      set_lane(y0, e, gi.c0);
      set_lane(y1, e, gi.c1);
      set_lane(y2, e, gi.c2);
    }
  }
  if constexpr (GIN) {
    if (a.gin) tile.store(a.gin, a.coef + (size_t)img * a.coef_stride, a.stamp, y0, y1, y2);
  }
  block_row_sum(acc, sPart, a.partial, bid);
}

struct KnotsBwdArgs {
  const float* ws;       // prep output (exp'd knots at WS_KNOTS)
  const float* partial;  // [B][blocks_per_image][row]: BWD_NACC floats per row, n_knots for the PWL layer
  const float* greg;     // nullable [B]
  float* graw[3];        // gradients shaped like rawL, rawR, rawH
  int K[3];
  unsigned ws_stride, blocks_per_image;
};

// One workgroup per image: fixed-order float64 reduction of the block partials, then the chain rule
// (P, Q, d reg) -> raw knots of each of the 10 curves (curl_math_bwd.h: knots_bwd).
// (Round 4 tried this pass FOLDED into the last workgroup of each image to finish -- a ticket counter in the workspace row,
// agent-scope stores / loads of the partial rows -- to save the launch at the training crop batch: 27.5 us against 25.1 for
// the two launches, the last workgroup's L2-bypassing reads cost more than the kernel boundary; with __threadfence()
// instead, 295 us.  tools/experiments/patches/r04_bwd_fold.patch, profiles/r04/small_batch_*.log.)
#define KNOTS_BWD_THREADS 1024
__global__ __launch_bounds__(KNOTS_BWD_THREADS) void knots_bwd_kernel(KnotsBwdArgs a) {
  // One walk over the image's [blocks][20] partials: thread t < 1020 adds the floats t, t + 1020, ... (1020 = 51 x 20: always
  // value t % 20, consecutive lanes read consecutive floats), then the 51 phase sums of a value are added in phase order --
  // a fixed order in float64, bit-reproducible.  The walk is a chain of dependent load + add steps, hence the wide block.
  constexpr int kPhases = KNOTS_BWD_THREADS / BWD_NACC, kLive = kPhases * BWD_NACC;
  __shared__ double sAcc[kLive];
  __shared__ double sPQ[BWD_NACC];
  const unsigned b = blockIdx.x;
  const float* part = a.partial + (size_t)b * a.blocks_per_image * BWD_NACC;
  // ---- everything the chain rule at the end needs from memory is asked for HERE (round 5): the row's stamp, d loss / d reg,
  // the five knots around this thread's own.  Asked for behind the reductions, each was a memory latency of its own at the end
  // of a kernel that is little else (greg, then the stamp, then the knots: three waits in a row in the ISA).
  // (the per-segment arguments as opaque scalars: `a.K[s]`, `a.graw[s]` with a per-lane s are otherwise compiled into indexed
  // VECTOR loads from the kernel-argument segment -- one more latency; curl_kernels.hip PREP_SEGS)
  int K0s = a.K[0], K1s = a.K[1], K2s = a.K[2];
  float *g0 = a.graw[0], *g1 = a.graw[1], *g2 = a.graw[2];
  asm volatile("" : "+s"(K0s), "+s"(K1s), "+s"(K2s), "+s"(g0), "+s"(g1), "+s"(g2));
  typedef float __attribute__((address_space(1))) * gptr;
  const int n0 = KP_TOTAL(K0s, 3), n1 = n0 + KP_TOTAL(K1s, 3), n_all = n1 + KP_TOTAL(K2s, 4);
  const float* row = a.ws + (size_t)b * a.ws_stride;
  const unsigned row_stamp = reinterpret_cast<const unsigned*>(row)[WS_STAMP];
  // (one unconditional load; the value is used only if greg is there)
  const float greg_f = *(const float __attribute__((address_space(1)))*)(a.greg ? a.greg + b : row);
  // thread t's (curve, knot): t < n_all  (a macro over plain locals: as a struct out of a lambda the seven ints went to scratch)
#define KNOT_OF(i, P)                                                                       \
  const int P##s = (i) < n0 ? 0 : ((i) < n1 ? 1 : 2);                                       \
  const int P##Ks = P##s == 0 ? K0s : (P##s == 1 ? K1s : K2s);                              \
  const int P##nc = P##s == 2 ? 4 : 3, P##K0 = KP_K(P##Ks);                                 \
  const int P##in_seg = (i) - (P##s == 0 ? 0 : (P##s == 1 ? n0 : n1));                      \
  const int P##local = min(P##in_seg / P##K0, P##nc - 1), P##kk = P##in_seg - P##local * P##K0; \
  const int P##K = P##local == P##nc - 1 ? KP_LAST(P##Ks) : P##K0; /* torch.chunk: the last curve may be shorter */ \
  const int P##c = (P##s == 0 ? 0 : (P##s == 1 ? 3 : 6)) + P##local
  const int i_first = (int)threadIdx.x;
  const int i_mine = min(i_first, n_all - 1);
  KNOT_OF(i_mine, my_);
  float c5[5];
  {
    const float* C = row + WS_KNOTS + (i_mine - my_kk);  // knots are stored segment after segment
#pragma unroll
    for (int d = 0; d < 5; ++d) c5[d] = C[min(max(my_kk - 2 + d, 0), my_K - 1)];
  }
  if (threadIdx.x < kLive) {
    // eight loads in flight per thread, eight partial sums, added in a fixed order (walk_sum8)
    sAcc[threadIdx.x] = walk_sum8(part, threadIdx.x, kLive, (size_t)a.blocks_per_image * BWD_NACC);
  }
  __syncthreads();
  if (threadIdx.x < BWD_NACC) {
    double r = sAcc[threadIdx.x];
#pragma unroll
    for (int m = 1; m < kPhases; ++m) r += sAcc[threadIdx.x + m * BWD_NACC];
    sPQ[threadIdx.x] = r;
  }
  __syncthreads();
  // one thread per (curve, knot), from the values asked for at the top
  const double g_reg = a.greg ? (double)greg_f : 0.0;
  // the workspace row must be the one a prep pass filled for THIS call's knot counts (CURL_F_WS_READY trusts the caller with
  // the values; a row of another shape, or one never filled, is answered with NaN gradients instead of plausible numbers)
  const bool row_ok = row_stamp == ws_stamp((unsigned)n_all, a.ws_stride);
  if (i_first < n_all) {
    const float g = knot_bwd5(c5, my_K, sPQ[my_c], sPQ[10 + my_c], g_reg, my_kk);
    ((gptr)(my_s == 0 ? g0 : (my_s == 1 ? g1 : g2)))[(size_t)b * KP_TOTAL(my_Ks, my_nc) + my_in_seg] = row_ok ? g : __builtin_nanf("");
  }
  for (int i = i_first + KNOTS_BWD_THREADS; i < n_all; i += KNOTS_BWD_THREADS) {  // more than 1 024 knots per image: K > 102
    KNOT_OF(i, m_);
    const float* C = row + WS_KNOTS + (i - m_kk);
    const float g = knot_bwd(C, m_K, sPQ[m_c], sPQ[10 + m_c], g_reg, m_kk);
    ((gptr)(m_s == 0 ? g0 : (m_s == 1 ? g1 : g2)))[(size_t)b * KP_TOTAL(m_Ks, m_nc) + m_in_seg] = row_ok ? g : __builtin_nanf("");
  }
#undef KNOT_OF
}
