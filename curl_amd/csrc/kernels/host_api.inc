// host_api.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int check_img(const void* in, const void* out, int B, int H, int W) {
  if (!in || !out) return fail(CURL_E_NULL, "image pointer is NULL");
  if (B <= 0 || H <= 0 || W <= 0) return fail(CURL_E_SHAPE, "B, H, W must be positive");
  if ((uint64_t)H * (uint64_t)W > (1ull << 30)) return fail(CURL_E_SHAPE, "H*W exceeds 2^30 pixels");
  if (B > 65535) return fail(CURL_E_SHAPE, "B exceeds 65535 images per call");
  return 0;
}
// the SPATIAL order-4 polynomial tables (126 coefficients) are copied into LDS as 8-byte pairs (9 x 126 floats per image:
// every image's table starts on an 8-byte boundary when the first one does).  Every other width (35, and orders 1-3: 4, 10,
// 20, 6, 21, 56) is read as scalars: a float's own 4-byte alignment is all they need.
static int check_coeffs_aligned(const float* coeffs, int num_coeffs) {
  if (num_coeffs == PolyEval<5>::kCoeffs && (uintptr_t)coeffs % 8) return fail(CURL_E_SHAPE, "coeffs must be 8-byte aligned (num_coeffs = 126)");
  if ((uintptr_t)coeffs % 4) return fail(CURL_E_SHAPE, "coeffs must be 4-byte aligned");
  return 0;
}
static int check_flags(unsigned flags, unsigned allowed) {
  const unsigned tune = CURL_F_TUNE_UNROLL_MASK | CURL_F_TUNE_BLOCK_MASK | CURL_F_TUNE_XCD_MASK | CURL_F_TUNE_OCC_MASK | CURL_F_TUNE_PREP_MASK | CURL_F_MASK_FIRST | CURL_F_TUNE_NO_NT | CURL_F_DIAG_NO_MEM;
  if (flags & ~(allowed | tune)) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point");
  if ((flags & CURL_F_EXACT_ORDER) && (flags & CURL_F_PWL))
    return fail(CURL_E_FLAGS, "CURL_F_EXACT_ORDER and CURL_F_PWL are exclusive");
  if (((flags & CURL_F_TUNE_PREP_MASK) >> CURL_F_TUNE_PREP_SHIFT) > 2)
    return fail(CURL_E_FLAGS, "curve-collapse placement must be 0 (library's choice), 1 (separate launch) or 2 (in the kernel)");
  return 0;
}
// the last HIP error as an entry point's return value (`where` names the kernels in curl_last_error)
static int hip_done(const char* where) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e, where) : 0;
}

// every pointer on a grid of `bytes` (NULL is on every grid)
template <class... P>
static bool on_grid(unsigned bytes, const P*... p) {
  return ((uintptr_t)0 | ... | (uintptr_t)p) % bytes == 0;
}
// THE float4-or-scalar verdict.  float4 access to image planes: plane size a multiple of 4 pixels, every image base on a grid
// of base_align bytes -- 16 for float planes, 4 for the byte edges' interleaved images (dword accesses) --, float masks on the
// 16-byte grid, uint8 masks on the 4-byte one (a mask pointer that mask_kind does not name is nobody's business)
template <class... P>
static bool planes_vec4(size_t HW, const void* mask, int mask_kind, unsigned base_align, const P*... bases) {
  return HW % 4 == 0 && on_grid(base_align, bases...) && (mask_kind != CURL_MASK_F32 || on_grid(16, mask)) &&
         (mask_kind != CURL_MASK_U8 || on_grid(4, mask));
}
// What a pointwise kernel outside the stream_kernel skeleton is launched with: one lane per float4 group (or pixel), 256-thread
// blocks, grid (blocks per image, image)
struct Pointwise {
  bool aligned;
  unsigned n, bpi;  // groups per plane, blocks per image
  dim3 grid;
  bool too_large() const { return (uint64_t)bpi * (uint64_t)grid.y > 0x7fffffffull; }  // (asked by the entries with partial rows per block)
};
static Pointwise pointwise(size_t HW, int B, bool aligned) {
  Pointwise p;
  p.aligned = aligned;
  p.n = (unsigned)(HW / (aligned ? 4 : 1));
  p.bpi = (p.n + 255u) / 256u;
  p.grid = dim3(p.bpi, (unsigned)B);
  return p;
}
// f(VEC, MK) with std::integral_constants for the vector width (4 or 1) and the mask kind, over (aligned, mask_kind); MASKS
// names the mask kinds the kernel family is instantiated for, so that no other instantiation comes into being
enum MaskKinds { kMasksAll, kMasksNone, kMasksU8F32 };
template <int I>
using int_c = std::integral_constant<int, I>;
template <MaskKinds MASKS, class F>
static void dispatch_vec_mask(bool aligned, int mask_kind, F&& f) {
  const auto with_vec = [&](auto vec) {
    if constexpr (MASKS == kMasksNone) {
      f(vec, int_c<CURL_MASK_NONE>());
    } else {
      if (mask_kind == CURL_MASK_U8) f(vec, int_c<CURL_MASK_U8>());
      else if (MASKS == kMasksU8F32 || mask_kind == CURL_MASK_F32) f(vec, int_c<CURL_MASK_F32>());
      else if constexpr (MASKS == kMasksAll) f(vec, int_c<CURL_MASK_NONE>());
    }
  };
  if (aligned) with_vec(int_c<4>());
  else with_vec(int_c<1>());
}

constexpr unsigned kXcdDefault = 1;  // library default of the workgroup -> tile mapping: 1 = plain, 2 = XCD-contiguous
struct Geometry {
  int xcd = 0;   // XCD-contiguous mapping requested
  int vec;       // 4 or 1
  int unroll;    // 1, 2 or 4
  unsigned n;    // plane length in vec units
  unsigned blocks_per_image, n_blocks, n_images;
  int nt;  // non-temporal loads and stores (float4 kernels)
  unsigned threads = 256;      // block size (row-tiled ops: follows the row width)
  unsigned units = 0, segs = 0;  // row-tiled ops: vec groups per row, blocks per row
  unsigned lds_cap = 0;  // unused dynamic LDS bytes per workgroup that hold the CU to k resident workgroups
};
// Row tiles: a block covers (part of) ONE image row.  Block size = the multiple of 64 lanes (<= 256) that wastes the fewest
// lanes on the last block of a row, larger preferred: 1500 px = 375 float4 groups -> 2 blocks of 192 lanes (2.3 % idle)
// rather than 256 + 119.
struct RowBlocks {
  unsigned threads, segs;
};
static RowBlocks row_blocks(unsigned units) {
  unsigned best_t = 64, best_waste = ~0u;
  for (unsigned t = 64; t <= 256; t += 64) {
    unsigned segs = (units + t - 1) / t, waste = segs * t - units;
    if (waste <= best_waste) best_waste = waste, best_t = t;
  }
  return RowBlocks{best_t, (units + best_t - 1) / best_t};
}
// Row-tiled ops (Op::kRowTiles): the grid of a geometry whose vector width and tuning are decided
static int make_row_geometry(Geometry& g, int B, int H, int W) {
  if (g.vec == 4 && W % 4 != 0) g.vec = 1;  // rows must start on a float4 boundary
  g.units = (unsigned)(W / g.vec);
  const RowBlocks rb = row_blocks(g.units);
  g.threads = rb.threads;
  g.segs = rb.segs;
  g.n = (unsigned)((size_t)H * W / g.vec);
  uint64_t per_image = (uint64_t)g.segs * (uint64_t)H;
  if (per_image * (uint64_t)B > 0x7fffffffull || per_image > 0x7fffffffull) return fail(CURL_E_SHAPE, "grid too large");
  g.blocks_per_image = (unsigned)per_image;
  g.n_blocks = (unsigned)(per_image * (uint64_t)B);
  return 0;
}

// Library defaults chosen from the sweep in DESIGN.md (profiles/).

// Unused dynamic LDS per 256-thread workgroup that lets exactly k = 2..7 of them share a CU.  LDS is handed out in 128
// granules of 1 280 bytes per CU (measured: tools/ubench/occ.hip's spin kernel, profiles/r03/exp27i_residency.log -- 32 768
// bytes, 25.6 granules, fit four times, not five, whatever hipOccupancyMaxActiveBlocksPerMultiprocessor says): floor(128 / k)
// granules fit k times and not k + 1; k = 2 takes 43 (64 would pass the 64 KB a launch may ask for without an attribute).
// static_bytes: the kernel's own static LDS, which counts toward the same granules -- subtracted, so that k means k.
static unsigned lds_for_resident(unsigned k, unsigned static_bytes = 0) {
  const unsigned total = (k == 2 ? 43u : 128u / k) * 1280u;
  return total > static_bytes ? total - static_bytes : 0u;
}
template <auto Kernel>
static unsigned static_lds() {  // hipFuncGetAttributes once per kernel instantiation
  static const unsigned v = [] {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(Kernel)) == hipSuccess ? (unsigned)a.sharedSizeBytes : 0u;
  }();
  return v;
}
// Op::kResident applies to launches of at least this many 1024-pixel tiles (below, every CU's share fits in one or two
// rounds of workgroups anyway and fewer resident ones would only serialise them)
constexpr unsigned kResidentMinTiles = 5632u;  // 22 per CU: 4 images of 1500x1000 (profiles/r03/exp27f_occ_batch.log)
// The same for the pointwise kernels outside the stream_kernel skeleton (256-thread blocks of 1024 pixels each).  TRUE resident
// workgroups per CU (round 3's logs print the nominal count of a reservation that ignored the kernels' static LDS: masked PSNR's
// "4" was 3 -- 32 B of static LDS took a 33rd granule): byte egress 4 (-5.9 %; 2 / 3 / 5 / 6: +0.1 / +0.4 / -1.6 / -1.4 %), byte
// ingress 4 (-14.4 %; 2: +10.1, 3: -6.2, 5: -10.6 %), masked PSNR 3 (-1.1 ... -4.0 % over three cards; a narrow optimum but a
// steady one); the CURLLoss terms are VALU-bound and lose at any cap (profiles/r03/exp27g, exp27j_occupancy_aux_kernels.log).
constexpr unsigned kResPsnr = 3, kResEgress = 4, kResIngress = 4, kResLoss = 0, kResLossBwd = 0;
static unsigned aux_lds(unsigned k_resident, const dim3& grid, bool float4_path, unsigned static_bytes) {
  return (k_resident > 1 && float4_path && (uint64_t)grid.x * grid.y >= kResidentMinTiles) ? lds_for_resident(k_resident, static_bytes) : 0u;
}

// a launch's workgroups at one group per lane (256 lanes; 1024-pixel tiles on the float4 path): what the self-prep and residency rules count
static uint64_t tiles_of(size_t groups, int B) { return (uint64_t)((groups + 255u) / 256u) * (uint64_t)B; }

// The caller's tuning fields, parsed and validated: what of the launch's shape the flags ask for.  unroll = 0: no request
// (ignore_unroll: ops built for one tile shape do not look at the field at all).
struct Tuning {  // (as declared: nothing asked)
  int unroll = 0;
  unsigned threads = 256;  // block size
  bool xcd = kXcdDefault == 2, nt = true;
  bool shape_asked = false;  // a tile-shape or occupancy field is set (unroll, block size, occupancy)
  unsigned lds_cap = 0;  // CURL_F_TUNE_OCC: k workgroups per CU (= k waves per SIMD at 256 threads), by an LDS reservation nobody uses
};
static int parse_tuning(Tuning& t, unsigned flags, bool ignore_unroll = false) {
  t.unroll = ignore_unroll ? 0 : (int)((flags & CURL_F_TUNE_UNROLL_MASK) >> CURL_F_TUNE_UNROLL_SHIFT);
  if (t.unroll != 0 && t.unroll != 1 && t.unroll != 2 && t.unroll != 4) return fail(CURL_E_FLAGS, "tuning unroll must be 1, 2 or 4");
  const unsigned bsel = (flags & CURL_F_TUNE_BLOCK_MASK) >> CURL_F_TUNE_BLOCK_SHIFT;
  if (bsel > 2) return fail(CURL_E_FLAGS, "tuning block size must be 0 (256), 1 (128) or 2 (64 threads)");
  t.threads = 256u >> bsel;
  const unsigned xsel = (flags & CURL_F_TUNE_XCD_MASK) >> CURL_F_TUNE_XCD_SHIFT;
  if (xsel > 2) return fail(CURL_E_FLAGS, "tuning tile mapping must be 0 (default), 1 (plain) or 2 (XCD-contiguous)");
  t.xcd = (xsel ? xsel : kXcdDefault) == 2;
  t.nt = !(flags & CURL_F_TUNE_NO_NT);
  const unsigned occ = (flags & CURL_F_TUNE_OCC_MASK) >> CURL_F_TUNE_OCC_SHIFT;
  t.lds_cap = occ > 1 ? lds_for_resident(occ) : 0u;  // occ == 1: "no cap" said explicitly (the operators' defaults off)
  t.shape_asked = t.unroll || bsel || occ;
  return 0;
}
// The grid arithmetic, last: `unroll` groups of `vec` floats per lane are decided, so is the LDS reservation
static int make_geometry(Geometry& g, const Tuning& t, int vec, int unroll, unsigned lds_cap, size_t HW, int B) {
  g.vec = vec;
  g.unroll = unroll;
  g.n = (unsigned)(HW / vec);
  g.threads = t.threads;
  const unsigned per_chunk = g.threads * (unsigned)unroll;
  g.blocks_per_image = (g.n + per_chunk - 1) / per_chunk;
  const uint64_t nb = (uint64_t)g.blocks_per_image * (uint64_t)B;
  if (nb > 0x7fffffffull) return fail(CURL_E_SHAPE, "grid too large");
  g.n_blocks = (unsigned)nb;
  g.n_images = (unsigned)B;
  g.nt = t.nt;
  g.xcd = t.xcd;
  g.lds_cap = lds_cap;
  return 0;
}

template <class Op, int VEC, int MK, bool NT>
static void launch_u(const Geometry& g, const StreamArgs& a, hipStream_t s) {
  dim3 grid(a.xcd_per ? 8u * a.xcd_per : g.blocks_per_image, g.n_images), block(g.threads);
  if constexpr (Op::kSingleTileShape) {
    // very large ops (polynomial layers) are built for one tile shape only
    hipLaunchKernelGGL((stream_kernel<Op, VEC, 1, MK, NT>), grid, block, g.lds_cap, s, a);
  } else {
    switch (g.unroll) {
      case 1:
        if constexpr (Op::kMask && MK == CURL_MASK_U8 && VEC == 4 && NT && Op::kLdsFloats == 0) {
          if (a.mask_first == 1) {  // CURL_F_MASK_FIRST / Op::kMaskFirst: the foreground-mask variant of the kernel
            hipLaunchKernelGGL((stream_kernel<Op, VEC, 1, MK, NT, FMT_F32CHW, true>), grid, block, g.lds_cap, s, a);
            break;
          }
        }
        hipLaunchKernelGGL((stream_kernel<Op, VEC, 1, MK, NT>), grid, block, g.lds_cap, s, a);
        break;
      case 2:
        hipLaunchKernelGGL((stream_kernel<Op, VEC, 2, MK, NT>), grid, block, g.lds_cap, s, a);
        break;
      default:
        hipLaunchKernelGGL((stream_kernel<Op, VEC, 4, MK, NT>), grid, block, g.lds_cap, s, a);
        break;
    }
  }
}

static int launch_prep(const PrepArgs& p, int B, hipStream_t s) {
  hipLaunchKernelGGL(knots_prep_kernel, dim3(B), dim3(256), 0, s, p);
  return hip_done("knots_prep_kernel");
}

// rows [row0, row0 + rows) of images that are H_full rows high; H_full == 0: whole images
struct Slab {
  int H_full = 0, row0 = 0;
};

// The in-kernel form of the curve collapse (stream_selfprep_kernel) is taken while the launch's workgroups (1024 pixels each
// on the float4 path, 256 on the scalar one) number at most this many: the whole grid is resident at once (256 CUs x 8 workgroups), so the ~4 us prologue every workgroup pays
// runs beside its neighbours' instead of queueing behind them.  One 1500x1000 frame: 1 465 tiles (14.6 us against 15.2 per
// call), the training crop batch 32 x 256x256: 2 048 (14.6 against 15.4); two frames, 2 930 tiles, already lose (21.8 against
// 19.3): tools/small_batch.py, profiles/r04/small_batch_*.log.
constexpr unsigned kSelfPrepMaxTiles = 2048u;

// prep: the call's curve collapse, not yet launched (NULL: the op needs none, or the workspace is ready) -- launch_stream
// decides between a launch of its own and the in-kernel form (CURL_F_TUNE_PREP).  Every decision is taken once, in this
// order, and every check is through before the first launch: the float4-or-scalar verdict (pointers, sizes and the slab
// only), the caller's tuning fields, the groups per lane and the LDS reservation, the grid.
template <class Op>
static int launch_stream(const float* in, float* out, const void* mask, int mask_kind, const float* coef,
                         unsigned coef_stride, int B, int H, int W, unsigned flags, hipStream_t s, const char* name,
                         int op_flag = 0, Slab slab = Slab(), const PrepArgs* prep = nullptr) {
  // a slab's plane stride and first-row offset must be float4 multiples too for the vector kernels (else scalar)
  const size_t HW = (size_t)H * W, plane_px = slab.H_full ? (size_t)slab.H_full * W : HW, off_px = (size_t)slab.row0 * W;
  const int vec = planes_vec4(HW, mask, mask_kind, 16, in, out) && (plane_px | off_px) % 4 == 0 ? 4 : 1;
  Tuning t;
  if (int rc = parse_tuning(t, flags, Op::kSingleTileShape)) return rc;
  const bool no_mem = flags & CURL_F_DIAG_NO_MEM, mask_first = !no_mem && (Op::kMaskFirst || (flags & CURL_F_MASK_FIRST));
  // the launch's workgroups at one group per lane: 1024-pixel ones on the float4 path, 256-pixel ones on the scalar path (H*W
  // or a pointer off the float4 grid -- 32 crops of 255x255 are 8 160 workgroups, not 2 048: no longer resident at once, each
  // paying the prologue; ADVICE r4)
  const uint64_t tiles = tiles_of(HW / vec, B);
  int unroll = t.unroll ? t.unroll : Op::kUnroll;
  unsigned lds_cap = t.lds_cap;
  bool self_prep = false;
  if constexpr (Op::kSelfPrep) {
    const unsigned psel = (flags & CURL_F_TUNE_PREP_MASK) >> CURL_F_TUNE_PREP_SHIFT;
    const bool as_is = !t.shape_asked && !(flags & (CURL_F_TUNE_XCD_MASK | CURL_F_TUNE_NO_NT | CURL_F_MASK_FIRST)) && !no_mem;
    if (prep && tiles > 0x7fffffffull) return fail(CURL_E_SHAPE, "grid too large");  // (the in-kernel form's grid, whichever form runs)
    self_prep = prep && as_is && !Op::kMaskFirst && (psel == 2 || (psel == 0 && tiles <= kSelfPrepMaxTiles));
    if (self_prep) unroll = 1;  // one group per lane
  }
  if constexpr (Op::kResident > 0) {
    // large float4 launches with no tile-shape / occupancy request of the caller's: one group per lane, Op::kResident
    // workgroups per CU (ops.inc OpDefaults::kResident)
    if (!t.shape_asked && !self_prep && vec == 4 && tiles >= kResidentMinTiles) unroll = 1, lds_cap = lds_for_resident(Op::kResident);
  }
  // the mask-first kernel variant exists at one group per lane: a caller who asks for it gets that tile shape (ops whose
  // default is two groups -- the HSV stage below kResidentMinTiles -- would otherwise ignore the flag silently; ADVICE r3)
  if constexpr (Op::kMask && !Op::kSingleTileShape)
    if (mask_first && mask_kind == CURL_MASK_U8 && vec == 4 && !t.unroll) unroll = 1;
  if constexpr (Op::kLdsFloats > 0 || Op::kRowTiles) lds_cap = 0;  // ops with LDS tables of their own: no reservation on top
  Geometry g;
  if (int rc = make_geometry(g, t, vec, unroll, lds_cap, HW, B)) return rc;
  if constexpr (Op::kRowTiles)
    if (int rc = make_row_geometry(g, B, H, W)) return rc;
  if (plane_px % g.vec || off_px % g.vec) return fail(CURL_E_SHAPE, "internal: slab not aligned to the vector width");
  if (prep && !self_prep)
    if (int rc = launch_prep(*prep, B, s)) return rc;
  StreamArgs a;
  a.in = in;
  a.out = out;
  a.mask = mask;
  a.coef = coef;
  a.coef_stride = coef_stride;
  a.n = g.n;
  a.blocks_per_image = g.blocks_per_image;
  a.n_blocks = g.n_blocks;
  a.no_mem = no_mem;
  a.W = (unsigned)W;
  a.H = (unsigned)(slab.H_full ? slab.H_full : H);
  a.op_flag = op_flag;
  a.mask_first = mask_first;
  a.white = nullptr;
  a.units = g.units, a.segs = g.segs;
  a.plane = (unsigned)(plane_px / g.vec), a.off = (unsigned)(off_px / g.vec), a.row0 = (unsigned)slab.row0;
  a.xcd_per = (g.xcd && !Op::kRowTiles && g.blocks_per_image >= 64u) ? (g.blocks_per_image + 7u) / 8u : 0u;
  dispatch_vec_mask<Op::kMask ? kMasksAll : kMasksNone>(g.vec == 4, mask_kind, [&](auto V, auto M) {
    constexpr bool kNT = V == 4;  // the scalar correctness path: plain accesses
    if constexpr (Op::kSelfPrep) {
      if (self_prep) {
        hipLaunchKernelGGL((stream_selfprep_kernel<Op, V, M, kNT>), dim3(g.blocks_per_image, g.n_images), dim3(256), 0, s, a, *prep);
        return;
      }
    }
    if (kNT && !g.nt) launch_u<Op, V, M, false>(g, a, s);
    else launch_u<Op, V, M, kNT>(g, a, s);
  });
  return hip_done(name);
}

// FMT_U8HWC launch: interleaved bytes in and out, optional white-background mask; one tile shape per op, no tuning
template <class Op>
static int launch_stream_u8(const uint8_t* in, uint8_t* out, const void* mask, int mask_kind, const uint8_t* white,
                            const float* coef, unsigned coef_stride, int B, int H, int W, hipStream_t s,
                            const char* name, const PrepArgs* prep = nullptr) {
  constexpr int U = Op::kSingleTileShape ? 1 : Op::kUnroll;
  const size_t HW = (size_t)H * W;
  Geometry g;
  if (int rc = make_geometry(g, Tuning(), planes_vec4(HW, mask, mask_kind, 4, in, out, white) ? 4 : 1, U, 0, HW, B)) return rc;
  if constexpr (Op::kRowTiles)
    if (int rc = make_row_geometry(g, B, H, W)) return rc;
  if (prep)  // (always a launch of its own: the byte edge has no in-kernel collapse)
    if (int rc = launch_prep(*prep, B, s)) return rc;
  StreamArgs a{};
  a.in = reinterpret_cast<const float*>(in);
  a.out = reinterpret_cast<float*>(out);
  a.mask = mask;
  a.white = white;
  a.coef = coef;
  a.coef_stride = coef_stride;
  a.n = g.n;
  a.blocks_per_image = g.blocks_per_image;
  a.n_blocks = g.n_blocks;
  a.no_mem = 0;
  a.W = (unsigned)W;
  a.H = (unsigned)H;
  a.op_flag = 0;
  a.units = g.units, a.segs = g.segs;
  a.plane = a.n, a.off = 0, a.row0 = 0;
  const dim3 grid(g.blocks_per_image, g.n_images), block(g.threads);
  dispatch_vec_mask<Op::kMask ? kMasksAll : kMasksNone>(g.vec == 4, mask_kind, [&](auto V, auto M) {
    hipLaunchKernelGGL((stream_kernel<Op, V, U, M, V == 4, FMT_U8HWC>), grid, block, 0, s, a);
  });
  return hip_done(name);
}

static int check_mask(const void* mask, int mask_kind) {
  if (mask_kind != CURL_MASK_NONE && mask_kind != CURL_MASK_U8 && mask_kind != CURL_MASK_F32)
    return fail(CURL_E_MASK, "mask_kind must be 0 (none), 1 (u8) or 2 (f32)");
  if (mask_kind != CURL_MASK_NONE && !mask) return fail(CURL_E_MASK, "mask_kind set but mask pointer is NULL");
  return 0;
}
static int check_K(int Kp, bool uneven_ok = false) {
  const int K = KP_K(Kp), last = KP_LAST(Kp);
  if (Kp < 0 || K < 2 || K > CURL_MAX_KNOTS) return fail(CURL_E_KNOTS, "knots per curve must be in [2, CURL_MAX_KNOTS]");
  if (last < 2 || last > K) return fail(CURL_E_KNOTS, "CURL_K_UNEVEN: the last curve must hold between 2 and K knots");
  if (KP_UNEVEN(Kp) && !uneven_ok)
    return fail(CURL_E_KNOTS, "CURL_K_UNEVEN is supported by the affine (default) form only, not with CURL_F_EXACT_ORDER / CURL_F_PWL or apply_curve");
  return 0;
}
static int check_ws(const void* ws, size_t bytes, int B, int n_knots) {
  if (!ws) return fail(CURL_E_WORKSPACE, "workspace is NULL");
  if (!on_grid(16, ws)) return fail(CURL_E_WORKSPACE, "workspace must be 16-byte aligned");
  if (bytes < curl_workspace_bytes(B, n_knots)) return fail(CURL_E_WORKSPACE, "workspace too small");
  return 0;
}
// The knot set-up of a call: knots checked, workspace checked, and what the curve collapse is launched with.  One segment of
// n curves (adjust_*, the stages: 3 or 4) or the fused layer's three (L and R of 3 curves, H of 4).
struct KnotSetup {
  float* ws;
  unsigned stride;
  int n_knots;
  PrepArgs prep;
};
static int knot_setup(KnotSetup& k, int segs, const float* const (&raw)[3], const int (&ncurves)[3], const int (&K)[3], bool uneven_ok,
                      void* workspace, size_t workspace_bytes, int B, float* reg) {
  k.n_knots = 0;
  for (int i = 0; i < segs; ++i) {
    if (int rc = check_K(K[i], uneven_ok)) return rc;
    k.n_knots += KP_TOTAL(K[i], ncurves[i]);
  }
  if (int rc = check_ws(workspace, workspace_bytes, B, k.n_knots)) return rc;
  k.ws = (float*)workspace;
  k.stride = ws_stride(k.n_knots);
  for (int i = 0; i < 3; ++i) k.prep.raw[i] = i < segs ? raw[i] : nullptr, k.prep.ncurves[i] = i < segs ? ncurves[i] : 0, k.prep.K[i] = i < segs ? K[i] : 0;
  k.prep.ws = k.ws;
  k.prep.reg_out = reg;
  k.prep.stride = k.stride;
  return 0;
}
static int segment_knots(KnotSetup& k, const float* raw, int n_curves, int K, bool uneven_ok, void* workspace, size_t workspace_bytes,
                         int B, float* reg) {
  return knot_setup(k, 1, {raw, nullptr, nullptr}, {n_curves, 0, 0}, {K, 0, 0}, uneven_ok, workspace, workspace_bytes, B, reg);
}
static int layer_knots(KnotSetup& k, const float* rawL, const float* rawR, const float* rawH, int Kl, int Kr, int Kh, bool uneven_ok,
                       void* workspace, size_t workspace_bytes, int B, float* reg) {
  if (!rawL || !rawR || !rawH) return fail(CURL_E_NULL, "rawL/rawR/rawH must all be non-NULL");
  return knot_setup(k, 3, {rawL, rawR, rawH}, {3, 3, 4}, {Kl, Kr, Kh}, uneven_ok, workspace, workspace_bytes, B, reg);
}
static int layer_n_knots(int Kl, int Kr, int Kh) { return KP_TOTAL(Kl, 3) + KP_TOTAL(Kr, 3) + KP_TOTAL(Kh, 4); }
// scratch buffers: present, large enough, and on the 16-byte grid where the kernels read them as float4 / double2
static int check_scratch(const void* scratch, size_t bytes, size_t need, bool wants_16_byte_alignment, const char* msg) {
  if (!scratch || (wants_16_byte_alignment && !on_grid(16, scratch)) || bytes < need) return fail(CURL_E_WORKSPACE, msg);
  return 0;
}
// The counts, the (variables, order) pairs and which of them is which come from kPolyPairs (poly_pairs.h) everywhere below.
static int check_num_coeffs(int num_coeffs, const char* msg) { return is_poly_count(num_coeffs, 4) ? 0 : fail(CURL_E_KNOTS, msg); }
static int check_num_variables(int num_variables) {
  return is_poly_pair(num_variables, 4) ? 0 : fail(CURL_E_SHAPE, "num_variables must be 5 or 3 (degree 4)");
}
// The polynomial order of a forward call.  The eight coefficient counts C(V + D, D), V = 3 | 5, D = 1..4, are all different, so
// a count names its order and its variable count; the entries still want the order said (curl_hip_poly.h packs it into the
// high half of num_coeffs, as CURL_K_UNEVEN packs a knot count) because a plain count other than 126 | 35 has always been
// CURL_E_KNOTS.  A high half of 0 is order 4.  -> the count, checked against the order; 0 after fail().
static int unpack_num_coeffs(int packed, int& count, int& order) {
  count = packed & 0xffff, order = (packed >> 16) & 0xffff;
  if (order == 0) {
    order = 4;
    return check_num_coeffs(packed, "num_coeffs must be 126 (degree 4, 5 variables) or 35 (degree 4, 3 variables)");
  }
  if (!is_poly_count(count, order))
    return fail(CURL_E_KNOTS, "num_coeffs with a polynomial order in its high half: the order must be 1..4 and the count 6 | 21 | 56 | 126 (5 variables) or 4 | 10 | 20 | 35 (3 variables) for orders 1..4");
  return 0;
}
// The same for curl_poly_layer_f32's num_variables: the variable count in the low half, the degree in the high half.
static int unpack_num_variables(int packed, int& V, int& degree) {
  V = packed & 0xffff, degree = (packed >> 16) & 0xffff;
  if (degree == 0) {
    degree = 4;
    return check_num_variables(packed);
  }
  if (!is_poly_pair(V, degree))
    return fail(CURL_E_SHAPE, "num_variables with a polynomial degree in its high half: 5 or 3 variables, degree 1..4");
  return 0;
}
// f(V, D) with both as compile-time constants, for a count unpack_num_coeffs accepted (-1: no pair has that count)
template <class F, size_t... I>
static int dispatch_order(int count, F&& f, std::index_sequence<I...>) {
  int rc = -1;
  (void)((count == poly_count(kPolyPairs[I].V, kPolyPairs[I].D) && (rc = f(int_c<kPolyPairs[I].V>(), int_c<kPolyPairs[I].D>()), true)) || ...);
  return rc;
}
template <class F>
static int dispatch_order(int count, F&& f) {
  return dispatch_order(count, f, std::make_index_sequence<sizeof(kPolyPairs) / sizeof(kPolyPairs[0])>());
}
// The forward kernel of a pair: the row fold for the spatial order 4, OpTriSpace<V> at order 4, the order's own op below it;
// `where` names it in curl_last_error
template <int V, int D>
struct TriSpaceOp {
  static constexpr bool kRows = V == 5 && D == 4;
  typedef std::conditional_t<kRows, OpTriSpaceRows, std::conditional_t<D == 4, OpTriSpace<V>, OpTriSpaceOrder<V, D>>> Op;
  static constexpr unsigned kCoefStride = 9 * PolyEval<V, D>::kCoeffs;  // floats per image
  static constexpr const char* where(bool u8) { return kRows ? (u8 ? "trispace_rows_u8hwc" : "trispace_rows") : (u8 ? "trispace_u8hwc" : "trispace"); }
};

// chain_kernel's launch in two steps, so that a caller's own launches (the knot prep, apply_curve's regulariser) come after
// every check: the plan (verdict, tuning fields, groups per lane and LDS reservation, grid), then the launch
static int plan_chain(Geometry& g, const float* in, const float* out, int mode, int B, int H, int W, unsigned flags) {
  const size_t HW = (size_t)H * W;
  const int vec = planes_vec4(HW, nullptr, CURL_MASK_NONE, 16, in, out) ? 4 : 1;
  Tuning t;
  if (int rc = parse_tuning(t, flags & ~CURL_F_TUNE_BLOCK_MASK)) return rc;  // 256-thread kernel
  int unroll = t.unroll ? t.unroll : 2;
  unsigned lds_cap = t.lds_cap;
  // the affine form is a light streaming op (its block prologue -- knots to LDS, a barrier -- wants more waves than the
  // skeleton's ops: 5 workgroups per CU -- what round 3's nominal "7" was with the static tables counted --, one group per lane: 195.0 -> 186.9 us; profiles/r03/exp27j_occ_sweep_true_residency.log)
  if (mode == 0 && !t.shape_asked && vec == 4 && tiles_of(HW / 4, B) >= kResidentMinTiles)
    unroll = 1, lds_cap = lds_for_resident(5, static_lds<chain_kernel<4, 1>>());  // with the kernel's own 8 KB of static tables: five fit
  return make_geometry(g, t, vec, unroll, lds_cap, HW, B);
}
static int launch_chain(const Geometry& g, const float* in, float* out, const float* knots, unsigned knot_stride, int n_steps,
                        int K, const int* knot_off, const int* cin, const int* cout, int mode, hipStream_t s) {
  ChainArgs a;
  a.in = in;
  a.out = out;
  a.knots = knots;
  a.knot_stride = knot_stride;
  a.n_steps = n_steps;
  a.K = K;
  for (int i = 0; i < CHAIN_MAX; ++i) {
    a.knot_off[i] = i < n_steps ? knot_off[i] : 0;
    a.cin[i] = i < n_steps ? cin[i] : 0;
    a.cout[i] = i < n_steps ? cout[i] : 0;
  }
  a.n = g.n;
  a.blocks_per_image = g.blocks_per_image;
  a.n_blocks = g.n_blocks;
  a.mode = mode;
  const dim3 grid(g.blocks_per_image, g.n_images), block(g.threads);
  dispatch_vec_mask<kMasksNone>(g.vec == 4, CURL_MASK_NONE, [&](auto V, auto) {
    switch (g.unroll) {
      case 1:
        hipLaunchKernelGGL((chain_kernel<V, 1>), grid, block, g.lds_cap, s, a);
        break;
      case 2:
        hipLaunchKernelGGL((chain_kernel<V, 2>), grid, block, g.lds_cap, s, a);
        break;
      default:
        hipLaunchKernelGGL((chain_kernel<V, 4>), grid, block, g.lds_cap, s, a);
        break;
    }
  });
  return hip_done("chain_kernel");
}

static int chain_mode(unsigned flags) { return (flags & CURL_F_EXACT_ORDER) ? 1 : (flags & CURL_F_PWL) ? 2 : 0; }

// pixels per thread of the accumulation pass: enough to amortise the 3*T-value block reduction (>= 16), few enough
static unsigned tri_ppt(int B, size_t HW) {
  size_t p = HW * 9 * (size_t)B / (256u * 2048u);
  return (unsigned)(p < 16 ? 16 : (p > 64 ? 64 : p));
}
static unsigned tri_tiles(int B, size_t HW) {
  size_t per = 256u * (size_t)tri_ppt(B, HW);
  return (unsigned)((HW + per - 1) / per);
}

// Geometry of the spatial form's accumulation pass (trispace_coef_grad_strip_kernel): a block covers cw columns x 256/cw
// row phases; cw = the one of 64 / 128 / 256 that wastes the fewest lanes past the last column (ties: the widest), rows
// per thread enough to amortise the block reduction (3 x 126 values x 6 DPP steps) yet leave >= 2048 blocks' worth of work.
constexpr unsigned kTriStripStepsMax = 64;
constexpr bool kTriBwdStrips = true;
struct StripGeo {
  unsigned cw_log2, steps, n_cb, n_rt;
  unsigned tiles() const { return n_cb * n_rt; }
};
static StripGeo strip_geo(int B, int H, int W) {
  StripGeo g{8, 16, 1, 1};
  unsigned best = ~0u;
  for (unsigned l = 6; l <= 8; ++l) {
    unsigned cw = 1u << l, covered = ((unsigned)W + cw - 1) / cw * cw;
    if (covered <= best) best = covered, g.cw_log2 = l;
  }
  const unsigned cw = 1u << g.cw_log2, rp = 256u / cw;
  g.n_cb = ((unsigned)W + cw - 1) / cw;
  size_t steps = (size_t)H * g.n_cb * 3 * 2 * (size_t)B / (rp * 2048u);  // rows per thread that leave 2048 blocks
  g.steps = (unsigned)(steps < 16 ? 16 : (steps > kTriStripStepsMax ? kTriStripStepsMax : steps));
  g.n_rt = ((unsigned)H + g.steps * rp - 1) / (g.steps * rp);
  return g;
}

// the tiles of the tri-space backward's accumulation pass (one row of partials each)
static size_t tri_bwd_tiles(int B, int H, int W, int num_coeffs) {
  return (num_coeffs == PolyEval<5>::kCoeffs && kTriBwdStrips) ? strip_geo(B, H, W).tiles() : tri_tiles(B, (size_t)H * W);
}

template <int V>
static void launch_trispace_bwd(const float* img, const float* coeffs, const float* gout, float* gcoef, float* pxbuf,
                                float* partial, int B, int H, int W, int residual_only, hipStream_t s) {
  constexpr int NC = PolyEval<V>::kCoeffs;
  unsigned HW = (unsigned)((size_t)H * W), ppt = tri_ppt(B, HW), tiles = (unsigned)tri_bwd_tiles(B, H, W, NC);
  // (not planes_vec4's rule: pass 1 takes TRI_BWD_N = 2 pixels per lane, as 8-byte pairs)
  int vec_ok = (HW % TRI_BWD_N == 0) && on_grid(4 * TRI_BWD_N, img, gout, pxbuf);
  unsigned threads = (HW + TRI_BWD_N - 1) / TRI_BWD_N;
  if constexpr (V == 5) {
    // row tiles (see row_blocks): block = the multiple of 64 lanes that wastes the fewest at the row end
    int row_vec_ok = vec_ok && (W % TRI_BWD_N == 0);
    const unsigned units = ((unsigned)W + TRI_BWD_N - 1) / TRI_BWD_N;
    const RowBlocks rb = row_blocks(units);
    hipLaunchKernelGGL(trispace_bwd_px_rows_kernel, dim3(rb.segs * (unsigned)H, (unsigned)B), dim3(rb.threads), 0, s, img, coeffs, gout,
                       pxbuf, HW, (unsigned)W, (unsigned)H, units, rb.segs, residual_only, row_vec_ok);
  } else {
    hipLaunchKernelGGL(trispace_bwd_px_kernel<V>, dim3((threads + 255u) / 256u, (unsigned)B), dim3(256), 0, s, img, coeffs,
                       gout, pxbuf, HW, (unsigned)W, (float)W, (float)H, residual_only, vec_ok);
  }
  if constexpr (V == 5 && kTriBwdStrips) {
    const StripGeo g = strip_geo(B, H, W);
    CoefGradStripArgs a{pxbuf, partial, HW, (unsigned)W, (unsigned)H, g.cw_log2, g.steps, g.n_cb, g.n_rt, (unsigned)B * 3u * tiles,
                        (float)W, (float)H};
    hipLaunchKernelGGL(trispace_coef_grad_strip_kernel, dim3((a.items + 7u) / 8u * 8u * kPolyFoldXChunks), dim3(256), 0, s, a);
  } else {
    CoefGradArgs a{pxbuf, partial, HW, (unsigned)W, tiles, ppt, (unsigned)B * 3u * tiles, 256u / (unsigned)W, 256u % (unsigned)W,
                   (float)W, (float)H};
    hipLaunchKernelGGL(trispace_coef_grad_kernel<V>, dim3((a.items + 7u) / 8u * 8u * PolyEval<V>::kChunks), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(trispace_coef_final_kernel, dim3((9 * NC + COEF_FINAL_OUTS - 1) / COEF_FINAL_OUTS, (unsigned)B), dim3(256),
                     0, s, partial, gcoef, tiles, 9 * NC);
}

// The stand-alone polynomial layer's coefficient gradient: a tile = 1024 * steps pixels (256 lanes x steps groups of 4),
// steps = B * H * W / 2^20 held to [4, 16] -- enough pixels per lane to amortise the block reduction, enough tiles to fill
// the device on a training-sized batch.  The same for the float4 and the scalar instantiation (the scratch size must not
// depend on the pointers' alignment).
static unsigned poly_bwd_steps(int B, size_t HW) {
  const size_t p = HW * (size_t)B >> 20;
  return (unsigned)(p < 4 ? 4 : (p > 16 ? 16 : p));
}
static size_t poly_bwd_tiles(int B, size_t HW) {
  const size_t per = 1024u * (size_t)poly_bwd_steps(B, HW);
  return (HW + per - 1) / per;
}
template <int V>
static void launch_poly_layer_bwd(const float* img, const float* coeffs, const float* gout, float* gimg, float* gcoef,
                                  float* partial, int B, size_t HW, hipStream_t s) {
  constexpr int NC = PolyEval<V>::kCoeffs;
  if (gcoef) {
    const unsigned tiles = (unsigned)poly_bwd_tiles(B, HW);
    PolyLayerGradArgs a{img, gout, partial, (unsigned)HW, (unsigned)((HW + 3) / 4), tiles, poly_bwd_steps(B, HW), (unsigned)B * tiles};
    const dim3 grid((a.items + 7u) / 8u * 8u * PolyEval<V>::kChunks), block(256);
    dispatch_vec_mask<kMasksNone>(planes_vec4(HW, nullptr, CURL_MASK_NONE, 16, img, gout), CURL_MASK_NONE, [&](auto VEC, auto) {
      hipLaunchKernelGGL((poly_layer_coef_grad_kernel<V, VEC>), grid, block, 0, s, a);
    });
    hipLaunchKernelGGL(trispace_coef_final_kernel, dim3((3 * NC + COEF_FINAL_OUTS - 1) / COEF_FINAL_OUTS, (unsigned)B), dim3(256),
                       0, s, partial, gcoef, tiles, 3 * NC);
  }
  if (gimg) {
    const Pointwise p = pointwise(HW, B, planes_vec4(HW, nullptr, CURL_MASK_NONE, 16, img, gout, gimg));
    dispatch_vec_mask<kMasksNone>(p.aligned, CURL_MASK_NONE, [&](auto VEC, auto) {
      hipLaunchKernelGGL((poly_layer_img_grad_kernel<V, VEC>), p.grid, dim3(256), 0, s, img, coeffs, gout, gimg, p.n);
    });
  }
}

// What the backward entry points share once their own knot arguments and the workspace are checked (knot_setup): the
// remaining argument checks, before any HIP call, then the knot prep -- unless CURL_F_WS_READY: the workspace is the one the
// forward filled for THESE knots (the autograd nodes keep it), and the prep launch and its kernel boundary go (a fifth of a
// training-crop-batch backward).
// Then what the three per-pixel backward kernels are launched with: the tile's arguments (bwd_tile.inc), one 256-thread
// block per tile and image (p), and whether the float4 kernels apply.
static int bwd_setup(BwdArgs& a, Pointwise& p, const float* img, const float* grad_out, float* grad_img, const void* mask,
                     int mask_kind, unsigned flags, const KnotSetup& k, void* scratch, size_t scratch_bytes, int B, int H, int W,
                     hipStream_t s, size_t scratch_need = 0,
                     const char* scratch_msg = "scratch missing, misaligned or smaller than curl_layer_bwd_scratch_bytes") {
  if (int rc = check_img(img, grad_out, B, H, W)) return rc;
  if (int rc = check_mask(mask, mask_kind)) return rc;
  if (int rc = check_flags(flags, CURL_F_WS_READY)) return rc;  // (+ CURL_F_MASK_FIRST, CURL_F_TUNE_PREP: allowed everywhere)
  if (!scratch_need) scratch_need = curl_layer_bwd_scratch_bytes(B, H, W);
  if (int rc = check_scratch(scratch, scratch_bytes, scratch_need, true, scratch_msg)) return rc;
  const size_t HW = (size_t)H * W;
  p = pointwise(HW, B, planes_vec4(HW, mask, mask_kind, 16, img, grad_out, grad_img));
  if (p.too_large()) return fail(CURL_E_SHAPE, "grid too large");
  a.in = img;
  a.gout = grad_out;
  a.gin = grad_img;
  a.mask = mask_kind ? mask : nullptr;
  a.coef = k.ws;
  a.partial = (float*)scratch;
  a.coef_stride = k.stride;
  a.n = p.n;
  a.blocks_per_image = p.bpi;
  a.n_blocks = p.bpi * (unsigned)B;
  a.mask_first = (flags & CURL_F_MASK_FIRST) ? 1 : 0;
  a.stamp = ws_stamp((unsigned)k.n_knots, k.stride);
  return (flags & CURL_F_WS_READY) ? 0 : launch_prep(k.prep, B, s);
}
// The second pass of the two layer forms (knots_bwd_kernel, layer_pwl_knots_bwd_kernel) takes the same arguments.
static KnotsBwdArgs knots_bwd_args(const KnotSetup& k, const void* scratch, const float* grad_reg, float* grad_rawL, float* grad_rawR,
                                   float* grad_rawH, int Kl, int Kr, int Kh, unsigned blocks_per_image) {
  KnotsBwdArgs kb;
  kb.ws = k.ws;
  kb.partial = (const float*)scratch;
  kb.greg = grad_reg;
  kb.graw[0] = grad_rawL, kb.graw[1] = grad_rawR, kb.graw[2] = grad_rawH;
  kb.K[0] = Kl, kb.K[1] = Kr, kb.K[2] = Kh;
  kb.ws_stride = k.stride;
  kb.blocks_per_image = blocks_per_image;
  return kb;
}

// The backward of one knot segment of 3 (adjust_rgb / adjust_lab, the Lab stage) or 4 curves (adjust_hsv, the HSV stage):
// arguments checked before any HIP call, the knot prep unless CURL_F_WS_READY, stage_bwd_kernel, stage_knots_bwd_kernel.
template <int OP>
static int stage_bwd_common(const float* img, const void* mask, int mask_kind, const float* raw, const float* grad_out,
                            const float* grad_reg, float* grad_img, float* grad_raw, void* workspace, size_t workspace_bytes,
                            void* scratch, size_t scratch_bytes, int B, int H, int W, int K, unsigned flags,
                            curl_stream_t stream, const char* name) {
  constexpr int NC = StageCurves<OP>::kN;
  g_err[0] = 0;
  if (!raw) return fail(CURL_E_NULL, "raw knot pointer is NULL");
  if (!grad_raw) return fail(CURL_E_NULL, "grad_raw is NULL");
  KnotSetup k;
  if (int rc = segment_knots(k, raw, NC, K, true, workspace, workspace_bytes, B, nullptr)) return rc;
  if (flags & CURL_F_PWL) return fail(CURL_E_FLAGS, "CURL_F_PWL has no backward");
  hipStream_t s = (hipStream_t)stream;
  BwdArgs a;
  Pointwise p;
  if (int rc = bwd_setup(a, p, img, grad_out, grad_img, mask, mask_kind, flags, k, scratch, scratch_bytes, B, H, W, s)) return rc;
  // (the adjust_* entries have no mask argument: only their CURL_MASK_NONE kernels exist)
  dispatch_vec_mask<(OP == STAGE_LAB || OP == STAGE_HSV) ? kMasksAll : kMasksNone>(p.aligned, mask_kind, [&](auto V, auto M) {
    if (a.gin) hipLaunchKernelGGL((stage_bwd_kernel<OP, V, M, true>), p.grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((stage_bwd_kernel<OP, V, M, false>), p.grid, dim3(256), 0, s, a);
  });
  if (int rc = hip_done(name)) return rc;
  StageKnotsArgs kb;
  kb.ws = k.ws;
  kb.partial = (const float*)scratch;
  kb.greg = grad_reg;
  kb.graw = grad_raw;
  kb.K = K;
  kb.ws_stride = k.stride;
  kb.blocks_per_image = a.blocks_per_image;
  hipLaunchKernelGGL(stage_knots_bwd_kernel<NC>, dim3((unsigned)B), dim3(STAGE_KNOTS_THREADS), 0, s, kb);
  return hip_done("stage_knots_bwd_kernel");
}

template <int CONV>
static int convert_bwd_common(const float* in, const float* grad_out, float* grad_in, int B, int H, int W, unsigned flags,
                              curl_stream_t stream, const char* name) {
  g_err[0] = 0;
  if (int rc = check_img(in, grad_out, B, H, W)) return rc;
  if (!grad_in) return fail(CURL_E_NULL, "grad_in is NULL");
  if (int rc = check_flags(flags, 0)) return rc;
  const size_t HW = (size_t)H * W;
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, nullptr, CURL_MASK_NONE, 16, in, grad_out, grad_in));
  ConvBwdArgs a{in, grad_out, grad_in, p.n};
  dispatch_vec_mask<kMasksNone>(p.aligned, CURL_MASK_NONE, [&](auto V, auto) {
    hipLaunchKernelGGL((convert_bwd_kernel<CONV, V>), p.grid, dim3(256), 0, (hipStream_t)stream, a);
  });
  return hip_done(name);
}

// the byte egress, with the white background where `mask` is given: float planes in (16-byte grid), interleaved bytes out (4)
template <MaskKinds MASKS>
static int launch_egress(const float* in, const void* mask, int mask_kind, uint8_t* out, int B, int H, int W, curl_stream_t stream,
                         const char* name) {
  const size_t HW = (size_t)H * W;
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, mask, mask_kind, 16, in) && on_grid(4, out));
  dispatch_vec_mask<MASKS>(p.aligned, mask_kind, [&](auto V, auto M) {
    hipLaunchKernelGGL((f32chw_to_u8hwc_kernel<V, M>), p.grid, dim3(256), aux_lds(kResEgress, p.grid, V == 4, static_lds<f32chw_to_u8hwc_kernel<V, M>>()),
                       (hipStream_t)stream, in, mask, out, p.n);
  });
  return hip_done(name);
}

extern "C" {

// 0.1.5: round 4 (CURL_F_TUNE_PREP: curves collapsed inside the streaming kernel for small launches; stamped workspace rows)
// 0.1.6: same entry points; curl_layer_bwd_f32 with grad_img = NULL runs its own kernel; gradients at black pixels, at
//        prediction == target (CURLLoss) and the PSNR of equal images under a float mask follow the reference (DESIGN.md 3e.8-9)
// 0.1.9: backward entry points of the stand-alone curve ops, converters and fused stages (curl_*_bwd_f32)
// 0.1.10: curl_layer_pwl_bwd_f32, the fused layer's backward with the paper's piecewise-linear curves (CURL_F_PWL)
// 0.1.11: curl_poly_layer_bwd_f32, the stand-alone polynomial layers' backward (image and coefficient gradients)
// 0.1.13: polynomial orders 1-3: the curl_trispace_fwd_* entries take the order in the high half of num_coeffs and
//         curl_poly_layer_f32 the degree in the high half of num_variables (include/curl_hip_poly.h)
// 0.1.16: the ragged byte entries: a batch of images of different sizes in one launch per class (include/curl_hip_ragged.h)
// 0.1.18: the ragged byte entries, foreground-aware: dead wavefronts store white unread (include/curl_hip_ragged_fg.h)
// 0.1.19: the exact score of a ragged byte batch: per-image integer SSE and pixel count (include/curl_hip_ragged_score.h)
// 0.1.20: the MS-SSIM statistics of a ragged byte batch: six launches from the bytes (include/curl_hip_ragged_msssim.h)
// 0.1.21: the CURLLoss statistics of a ragged byte batch: six launches from the bytes (include/curl_hip_ragged_loss.h)
int curl_version(void) { return 121; }

const char* curl_last_error(void) { return g_err; }

size_t curl_workspace_bytes(int B, int n_knots) {
  if (B <= 0 || n_knots < 0) return 0;
  return (size_t)B * ws_stride(n_knots) * sizeof(float);
}

int curl_apply_curve_f32(const float* img, const float* C, float* out, float* reg, int B, int H, int W, int K,
                         int channel_in, int channel_out, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!C) return fail(CURL_E_NULL, "C is NULL");
  if (int rc = check_K(K)) return rc;
  if (channel_in < 0 || channel_in > 2 || channel_out < 0 || channel_out > 2)
    return fail(CURL_E_SHAPE, "channel_in/channel_out must be 0, 1 or 2");
  if (int rc = check_flags(flags, CURL_F_EXACT_ORDER | CURL_F_PWL)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Geometry g;
  if (int rc = plan_chain(g, img, out, chain_mode(flags), B, H, W, flags)) return rc;
  if (reg) {
    hipLaunchKernelGGL(curve_reg_kernel, dim3((B + 63) / 64), dim3(64), 0, s, C, reg, B, K);
    if (int rc = hip_done("curve_reg_kernel")) return rc;
  }
  int off[1] = {0}, ci[1] = {channel_in}, co[1] = {channel_out};
  return launch_chain(g, img, out, C, (unsigned)K, 1, K, off, ci, co, chain_mode(flags), s);
}

static int adjust_common(const float* img, const float* raw, float* out, float* reg, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, int K, unsigned flags, curl_stream_t stream,
                         int n_curves) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!raw) return fail(CURL_E_NULL, "raw knot pointer is NULL");
  if (int rc = check_flags(flags, CURL_F_EXACT_ORDER | CURL_F_PWL)) return rc;
  KnotSetup k;
  if (int rc = segment_knots(k, raw, n_curves, K, chain_mode(flags) == 0, workspace, workspace_bytes, B, reg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int mode = chain_mode(flags);
  if (mode == 0) {
    if (n_curves == 3)
      return launch_stream<OpAdjust3>(img, out, nullptr, 0, k.ws, k.stride, B, H, W, flags, s, "adjust3", 0, Slab(), &k.prep);
    return launch_stream<OpAdjustHsv>(img, out, nullptr, 0, k.ws, k.stride, B, H, W, flags, s, "adjust_hsv", 0, Slab(), &k.prep);
  }
  Geometry g;
  if (int rc = plan_chain(g, img, out, mode, B, H, W, flags)) return rc;
  if (int rc = launch_prep(k.prep, B, s)) return rc;
  int off[4], ci[4], co[4];
  for (int c = 0; c < n_curves; ++c) off[c] = WS_KNOTS + c * K;
  if (n_curves == 3) {
    for (int c = 0; c < 3; ++c) ci[c] = co[c] = c;  // curves.py:113-126,160-173
  } else {
    ci[0] = 0, co[0] = 0;  // curves.py:61-62
    ci[1] = 0, co[1] = 1;  // curves.py:67-68
    ci[2] = 1, co[2] = 1;  // curves.py:73-74
    ci[3] = 2, co[3] = 2;  // curves.py:79-80
  }
  return launch_chain(g, img, out, k.ws, k.stride, n_curves, K, off, ci, co, mode, s);
}

int curl_adjust_rgb_f32(const float* img, const float* raw, float* out, float* reg, void* workspace,
                        size_t workspace_bytes, int B, int H, int W, int K, unsigned flags, curl_stream_t stream) {
  return adjust_common(img, raw, out, reg, workspace, workspace_bytes, B, H, W, K, flags, stream, 3);
}
int curl_adjust_lab_f32(const float* img, const float* raw, float* out, float* reg, void* workspace,
                        size_t workspace_bytes, int B, int H, int W, int K, unsigned flags, curl_stream_t stream) {
  return adjust_common(img, raw, out, reg, workspace, workspace_bytes, B, H, W, K, flags, stream, 3);
}
int curl_adjust_hsv_f32(const float* img, const float* raw, float* out, float* reg, void* workspace,
                        size_t workspace_bytes, int B, int H, int W, int K, unsigned flags, curl_stream_t stream) {
  return adjust_common(img, raw, out, reg, workspace, workspace_bytes, B, H, W, K, flags, stream, 4);
}

#define CONVERTER_ENTRY(FN, OP)                                                                              \
  int FN(const float* in, float* out, int B, int H, int W, unsigned flags, curl_stream_t stream) {           \
    g_err[0] = 0;                                                                                            \
    if (int rc = check_img(in, out, B, H, W)) return rc;                                                     \
    if (int rc = check_flags(flags, 0)) return rc;                                                           \
    return launch_stream<OP>(in, out, nullptr, 0, nullptr, 0, B, H, W, flags, (hipStream_t)stream, #FN);     \
  }
CONVERTER_ENTRY(curl_rgb2lab_f32, OpRgb2Lab)
CONVERTER_ENTRY(curl_lab2rgb_f32, OpLab2Rgb)
CONVERTER_ENTRY(curl_rgb2hsv_f32, OpRgb2Hsv)
CONVERTER_ENTRY(curl_hsv2rgb_f32, OpHsv2Rgb)

int curl_lab_stage_f32(const float* img, const void* mask, int mask_kind, const float* rawL, float* out, float* reg,
                       void* workspace, size_t workspace_bytes, int B, int H, int W, int Kl, unsigned flags,
                       curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!rawL) return fail(CURL_E_NULL, "rawL is NULL");
  if (int rc = check_mask(mask, mask_kind)) return rc;
  if (int rc = check_flags(flags, CURL_F_PWL | CURL_F_EXACT_ORDER)) return rc;
  KnotSetup k;
  if (int rc = segment_knots(k, rawL, 3, Kl, chain_mode(flags) == 0, workspace, workspace_bytes, B, reg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (flags & CURL_F_PWL)  // the paper's clamped piecewise-linear curves, knots in LDS
    return launch_stream<OpLabStageTab<0>>(img, out, mask_kind ? mask : nullptr, mask_kind, k.ws, k.stride, B, H, W,
                                           flags & ~CURL_F_PWL, s, "lab_stage_pwl", Kl, Slab(), &k.prep);
  if (flags & CURL_F_EXACT_ORDER)  // validation mode: every curve as the reference's term-by-term float32 sum
    return launch_stream<OpLabStageTab<1>>(img, out, mask_kind ? mask : nullptr, mask_kind, k.ws, k.stride, B, H, W,
                                           flags & ~CURL_F_EXACT_ORDER, s, "lab_stage_exact", Kl, Slab(), &k.prep);
  return launch_stream<OpLabStage>(img, out, mask_kind ? mask : nullptr, mask_kind, k.ws, k.stride, B, H, W, flags, s,
                                   "lab_stage", 0, Slab(), &k.prep);
}

int curl_hsv_stage_f32(const float* img, const void* mask, int mask_kind, const float* rawH, float* out, float* reg,
                       void* workspace, size_t workspace_bytes, int B, int H, int W, int Kh, unsigned flags,
                       curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!rawH) return fail(CURL_E_NULL, "rawH is NULL");
  if (int rc = check_mask(mask, mask_kind)) return rc;
  if (int rc = check_flags(flags, 0)) return rc;
  KnotSetup k;
  if (int rc = segment_knots(k, rawH, 4, Kh, true, workspace, workspace_bytes, B, reg)) return rc;
  return launch_stream<OpHsvStage>(img, out, mask_kind ? mask : nullptr, mask_kind, k.ws, k.stride, B, H, W, flags,
                                   (hipStream_t)stream, "hsv_stage", 0, Slab(), &k.prep);
}

// the two *_slab_* entries: rows [row0, row0 + rows) of images H rows high, checked before the rows stand in for H
static int slab_of(Slab& slab, int H, int W, int row0, int rows) {
  if (H <= 0) return fail(CURL_E_SHAPE, "B, H, W must be positive");
  if (row0 < 0 || rows <= 0 || (int64_t)row0 + rows > H) return fail(CURL_E_SHAPE, "row slab [row0, row0 + rows) must lie inside [0, H)");
  if ((uint64_t)H * (uint64_t)(W > 0 ? W : 0) > (1ull << 30)) return fail(CURL_E_SHAPE, "H*W exceeds 2^30 pixels");
  slab.H_full = H, slab.row0 = row0;
  return 0;
}

static int layer_fwd_impl(const float* img, const void* mask, int mask_kind, const float* rawL, const float* rawR,
                          const float* rawH, float* out, float* reg, void* workspace, size_t workspace_bytes, int B, int H,
                          int W, int Kl, int Kr, int Kh, unsigned flags, curl_stream_t stream, Slab slab) {
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (int rc = check_mask(mask, mask_kind)) return rc;
  // (CURL_F_DIAG_SKIP_PREP: accepted by these two entries only -- it makes the kernel read a workspace the caller vouches for)
  if (int rc = check_flags(flags, CURL_F_PWL | CURL_F_EXACT_ORDER | CURL_F_DIAG_SKIP_PREP)) return rc;
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, chain_mode(flags) == 0, workspace, workspace_bytes, B, reg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const PrepArgs* prep = (flags & CURL_F_DIAG_SKIP_PREP) ? nullptr : &k.prep;
  flags &= ~CURL_F_DIAG_SKIP_PREP;
  if (flags & CURL_F_PWL)  // the paper's clamped piecewise-linear curves, all ten of them from LDS
    return launch_stream<OpLayerTab<0>>(img, out, mask_kind ? mask : nullptr, mask_kind, k.ws, k.stride, B, H, W,
                                        flags & ~CURL_F_PWL, s, "curl_layer_pwl", Kl | (Kr << 10) | (Kh << 20), slab, prep);
  if (flags & CURL_F_EXACT_ORDER)  // validation mode (SURVEY.md 7.2): curves.py:31-32 term by term, reference stage order
    return launch_stream<OpLayerTab<1>>(img, out, mask_kind ? mask : nullptr, mask_kind, k.ws, k.stride, B, H, W,
                                        flags & ~CURL_F_EXACT_ORDER, s, "curl_layer_exact", Kl | (Kr << 10) | (Kh << 20), slab, prep);
  return launch_stream<OpLayer>(img, out, mask_kind ? mask : nullptr, mask_kind, k.ws, k.stride, B, H, W, flags, s,
                                "curl_layer", 0, slab, prep);
}

int curl_layer_fwd_f32(const float* img, const void* mask, int mask_kind, const float* rawL, const float* rawR,
                       const float* rawH, float* out, float* reg, void* workspace, size_t workspace_bytes, int B, int H,
                       int W, int Kl, int Kr, int Kh, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  return layer_fwd_impl(img, mask, mask_kind, rawL, rawR, rawH, out, reg, workspace, workspace_bytes, B, H, W, Kl, Kr, Kh,
                        flags, stream, Slab());
}

int curl_layer_fwd_slab_f32(const float* img, const void* mask, int mask_kind, const float* rawL, const float* rawR,
                            const float* rawH, float* out, float* reg, void* workspace, size_t workspace_bytes, int B, int H,
                            int W, int row0, int rows, int Kl, int Kr, int Kh, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  Slab slab;
  if (int rc = slab_of(slab, H, W, row0, rows)) return rc;
  return layer_fwd_impl(img, mask, mask_kind, rawL, rawR, rawH, out, reg, workspace, workspace_bytes, B, rows, W, Kl, Kr,
                        Kh, flags, stream, slab);
}

int curl_layer_fwd_u8hwc(const uint8_t* img, const void* mask, int mask_kind, const float* rawL, const float* rawR,
                         const float* rawH, const uint8_t* white_mask, uint8_t* out, float* reg, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, int Kl, int Kr, int Kh, unsigned flags,
                         curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (int rc = check_mask(mask, mask_kind)) return rc;
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point");
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, true, workspace, workspace_bytes, B, reg)) return rc;
  return launch_stream_u8<OpLayer>(img, out, mask_kind ? mask : nullptr, mask_kind, white_mask, k.ws, k.stride, B, H, W,
                                   (hipStream_t)stream, "curl_layer_u8hwc", &k.prep);
}

size_t curl_layer_bwd_scratch_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  size_t HW = (size_t)H * W;
  size_t blocks = (HW + 255) / 256;  // upper bound: the scalar path, one pixel per lane
  return (size_t)B * blocks * BWD_NACC * sizeof(float);
}

int curl_layer_bwd_f32(const float* img, const void* mask, int mask_kind, const float* rawL, const float* rawR,
                       const float* rawH, const float* grad_out, const float* grad_reg, float* grad_img,
                       float* grad_rawL, float* grad_rawR, float* grad_rawH, void* workspace, size_t workspace_bytes,
                       void* scratch, size_t scratch_bytes, int B, int H, int W, int Kl, int Kr, int Kh, unsigned flags,
                       curl_stream_t stream) {
  g_err[0] = 0;
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, true, workspace, workspace_bytes, B, nullptr)) return rc;
  if (!grad_rawL || !grad_rawR || !grad_rawH) return fail(CURL_E_NULL, "grad_rawL/R/H must all be non-NULL");
  hipStream_t s = (hipStream_t)stream;
  BwdArgs a;
  Pointwise p;
  if (int rc = bwd_setup(a, p, img, grad_out, grad_img, mask, mask_kind, flags, k, scratch, scratch_bytes, B, H, W, s)) return rc;
  dispatch_vec_mask<kMasksAll>(p.aligned, mask_kind, [&](auto V, auto M) {
    if (a.gin) hipLaunchKernelGGL((layer_bwd_kernel<V, M, true>), p.grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((layer_bwd_kernel<V, M, false>), p.grid, dim3(256), 0, s, a);
  });
  if (int rc = hip_done("layer_bwd_kernel")) return rc;
  const KnotsBwdArgs kb = knots_bwd_args(k, scratch, grad_reg, grad_rawL, grad_rawR, grad_rawH, Kl, Kr, Kh, a.blocks_per_image);
  hipLaunchKernelGGL(knots_bwd_kernel, dim3(B), dim3(KNOTS_BWD_THREADS), 0, s, kb);
  return hip_done("knots_bwd_kernel");
}

size_t curl_layer_pwl_bwd_scratch_bytes(int B, int H, int W, int Kl, int Kr, int Kh) {
  if (B <= 0 || H <= 0 || W <= 0 || Kl < 2 || Kr < 2 || Kh < 2 || Kl > CURL_MAX_KNOTS || Kr > CURL_MAX_KNOTS || Kh > CURL_MAX_KNOTS)
    return 0;
  size_t HW = (size_t)H * W;
  size_t blocks = (HW + 255) / 256;  // upper bound: the scalar path, one pixel per lane
  return (size_t)B * blocks * (size_t)layer_n_knots(Kl, Kr, Kh) * sizeof(float);
}

// The fused layer's backward with the paper's curves: curl_layer_bwd_f32's arguments and checks, one row of n_knots block
// partials per workgroup (layer_pwl_bwd_kernel), then one workgroup per curve and image (layer_pwl_knots_bwd_kernel).
int curl_layer_pwl_bwd_f32(const float* img, const void* mask, int mask_kind, const float* rawL, const float* rawR,
                           const float* rawH, const float* grad_out, const float* grad_reg, float* grad_img,
                           float* grad_rawL, float* grad_rawR, float* grad_rawH, void* workspace, size_t workspace_bytes,
                           void* scratch, size_t scratch_bytes, int B, int H, int W, int Kl, int Kr, int Kh, unsigned flags,
                           curl_stream_t stream) {
  g_err[0] = 0;
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, false, workspace, workspace_bytes, B, nullptr)) return rc;
  if (!grad_rawL || !grad_rawR || !grad_rawH) return fail(CURL_E_NULL, "grad_rawL/R/H must all be non-NULL");
  if (flags & ~(CURL_F_WS_READY | CURL_F_MASK_FIRST)) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point");
  hipStream_t s = (hipStream_t)stream;
  const size_t need = (B > 0 && H > 0 && W > 0) ? curl_layer_pwl_bwd_scratch_bytes(B, H, W, Kl, Kr, Kh) : 0;
  PwlBwdArgs a;
  Pointwise p;
  if (int rc = bwd_setup(a, p, img, grad_out, grad_img, mask, mask_kind, flags, k, scratch, scratch_bytes, B, H, W, s, need,
                         "scratch missing, misaligned or smaller than curl_layer_pwl_bwd_scratch_bytes"))
    return rc;
  a.kl = Kl, a.kr = Kr, a.kh = Kh;
  const size_t lds = pwl_bwd_lds_bytes(Kl, Kr, Kh);
  dispatch_vec_mask<kMasksAll>(p.aligned, mask_kind, [&](auto V, auto M) {
    if (a.gin) hipLaunchKernelGGL((layer_pwl_bwd_kernel<V, M, true>), p.grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((layer_pwl_bwd_kernel<V, M, false>), p.grid, dim3(256), lds, s, a);
  });
  if (int rc = hip_done("layer_pwl_bwd_kernel")) return rc;
  const KnotsBwdArgs kb = knots_bwd_args(k, scratch, grad_reg, grad_rawL, grad_rawR, grad_rawH, Kl, Kr, Kh, a.blocks_per_image);
  hipLaunchKernelGGL(layer_pwl_knots_bwd_kernel, dim3(MAX_CURVES, (unsigned)B), dim3(PWL_KNOTS_THREADS), 0, s, kb);
  return hip_done("layer_pwl_knots_bwd_kernel");
}

int curl_adjust_rgb_bwd_f32(const float* img, const float* raw, const float* grad_out, const float* grad_reg,
                            float* grad_img, float* grad_raw, void* workspace, size_t workspace_bytes, void* scratch,
                            size_t scratch_bytes, int B, int H, int W, int K, unsigned flags, curl_stream_t stream) {
  return stage_bwd_common<STAGE_ADJ3>(img, nullptr, CURL_MASK_NONE, raw, grad_out, grad_reg, grad_img, grad_raw, workspace,
                                      workspace_bytes, scratch, scratch_bytes, B, H, W, K, flags & ~CURL_F_MASK_FIRST, stream,
                                      "adjust_rgb_bwd");
}
int curl_adjust_lab_bwd_f32(const float* img, const float* raw, const float* grad_out, const float* grad_reg,
                            float* grad_img, float* grad_raw, void* workspace, size_t workspace_bytes, void* scratch,
                            size_t scratch_bytes, int B, int H, int W, int K, unsigned flags, curl_stream_t stream) {
  return stage_bwd_common<STAGE_ADJ3>(img, nullptr, CURL_MASK_NONE, raw, grad_out, grad_reg, grad_img, grad_raw, workspace,
                                      workspace_bytes, scratch, scratch_bytes, B, H, W, K, flags & ~CURL_F_MASK_FIRST, stream,
                                      "adjust_lab_bwd");
}
int curl_adjust_hsv_bwd_f32(const float* img, const float* raw, const float* grad_out, const float* grad_reg,
                            float* grad_img, float* grad_raw, void* workspace, size_t workspace_bytes, void* scratch,
                            size_t scratch_bytes, int B, int H, int W, int K, unsigned flags, curl_stream_t stream) {
  return stage_bwd_common<STAGE_AHSV>(img, nullptr, CURL_MASK_NONE, raw, grad_out, grad_reg, grad_img, grad_raw, workspace,
                                      workspace_bytes, scratch, scratch_bytes, B, H, W, K, flags & ~CURL_F_MASK_FIRST, stream,
                                      "adjust_hsv_bwd");
}
int curl_rgb2lab_bwd_f32(const float* in, const float* grad_out, float* grad_in, int B, int H, int W, unsigned flags,
                         curl_stream_t stream) {
  return convert_bwd_common<CONV_RGB2LAB>(in, grad_out, grad_in, B, H, W, flags, stream, "rgb2lab_bwd");
}
int curl_lab2rgb_bwd_f32(const float* in, const float* grad_out, float* grad_in, int B, int H, int W, unsigned flags,
                         curl_stream_t stream) {
  return convert_bwd_common<CONV_LAB2RGB>(in, grad_out, grad_in, B, H, W, flags, stream, "lab2rgb_bwd");
}
int curl_rgb2hsv_bwd_f32(const float* in, const float* grad_out, float* grad_in, int B, int H, int W, unsigned flags,
                         curl_stream_t stream) {
  return convert_bwd_common<CONV_RGB2HSV>(in, grad_out, grad_in, B, H, W, flags, stream, "rgb2hsv_bwd");
}
int curl_hsv2rgb_bwd_f32(const float* in, const float* grad_out, float* grad_in, int B, int H, int W, unsigned flags,
                         curl_stream_t stream) {
  return convert_bwd_common<CONV_HSV2RGB>(in, grad_out, grad_in, B, H, W, flags, stream, "hsv2rgb_bwd");
}
int curl_lab_stage_bwd_f32(const float* img, const void* mask, int mask_kind, const float* rawL, const float* grad_out,
                           const float* grad_reg, float* grad_img, float* grad_rawL, void* workspace, size_t workspace_bytes,
                           void* scratch, size_t scratch_bytes, int B, int H, int W, int Kl, unsigned flags,
                           curl_stream_t stream) {
  return stage_bwd_common<STAGE_LAB>(img, mask, mask_kind, rawL, grad_out, grad_reg, grad_img, grad_rawL, workspace,
                                     workspace_bytes, scratch, scratch_bytes, B, H, W, Kl, flags, stream, "lab_stage_bwd");
}
int curl_hsv_stage_bwd_f32(const float* img, const void* mask, int mask_kind, const float* rawH, const float* grad_out,
                           const float* grad_reg, float* grad_img, float* grad_rawH, void* workspace, size_t workspace_bytes,
                           void* scratch, size_t scratch_bytes, int B, int H, int W, int Kh, unsigned flags,
                           curl_stream_t stream) {
  return stage_bwd_common<STAGE_HSV>(img, mask, mask_kind, rawH, grad_out, grad_reg, grad_img, grad_rawH, workspace,
                                     workspace_bytes, scratch, scratch_bytes, B, H, W, Kh, flags, stream, "hsv_stage_bwd");
}

static int trispace_fwd_impl(const float* img, const float* coeffs, float* out, int B, int H, int W, int num_coeffs,
                             unsigned flags, curl_stream_t stream, Slab slab) {
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!coeffs) return fail(CURL_E_NULL, "coeffs is NULL");
  int order;
  if (int rc = unpack_num_coeffs(num_coeffs, num_coeffs, order)) return rc;
  if (int rc = check_flags(flags, CURL_F_RESIDUAL_ONLY)) return rc;
  if (int rc = check_coeffs_aligned(coeffs, num_coeffs)) return rc;
  int ro = (flags & CURL_F_RESIDUAL_ONLY) ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_order(num_coeffs, [&](auto V, auto D) {
    typedef TriSpaceOp<V, D> T;
    return launch_stream<typename T::Op>(img, out, nullptr, 0, coeffs, T::kCoefStride, B, H, W, flags, s, T::where(false), ro, slab);
  });
}

int curl_trispace_fwd_f32(const float* img, const float* coeffs, float* out, int B, int H, int W, int num_coeffs,
                          unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  return trispace_fwd_impl(img, coeffs, out, B, H, W, num_coeffs, flags, stream, Slab());
}

int curl_trispace_fwd_slab_f32(const float* img, const float* coeffs, float* out, int B, int H, int W, int row0, int rows,
                               int num_coeffs, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  Slab slab;
  if (int rc = slab_of(slab, H, W, row0, rows)) return rc;
  return trispace_fwd_impl(img, coeffs, out, B, rows, W, num_coeffs, flags, stream, slab);
}

int curl_trispace_fwd_u8hwc(const uint8_t* img, const float* coeffs, const uint8_t* white_mask, uint8_t* out, int B, int H,
                            int W, int num_coeffs, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!coeffs) return fail(CURL_E_NULL, "coeffs is NULL");
  int order;
  if (int rc = unpack_num_coeffs(num_coeffs, num_coeffs, order)) return rc;
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (the byte output is an image)");
  if (int rc = check_coeffs_aligned(coeffs, num_coeffs)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_order(num_coeffs, [&](auto V, auto D) {
    typedef TriSpaceOp<V, D> T;
    return launch_stream_u8<typename T::Op>(img, out, nullptr, 0, white_mask, coeffs, T::kCoefStride, B, H, W, s, T::where(true));
  });
}

int curl_poly_layer_f32(const float* img, const float* coeffs, float* out, int B, int H, int W, int num_variables,
                        curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!coeffs) return fail(CURL_E_NULL, "coeffs is NULL");
  int degree;  // (the packed form of include/curl_hip_poly.h)
  if (int rc = unpack_num_variables(num_variables, num_variables, degree)) return rc;
  const size_t HW = (size_t)H * W;
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, nullptr, CURL_MASK_NONE, 16, img, out));
  dispatch_vec_mask<kMasksNone>(p.aligned, CURL_MASK_NONE, [&](auto VEC, auto) {
    dispatch_order(poly_count(num_variables, degree), [&](auto V, auto D) {
      void (*kernel)(const float*, const float*, float*, unsigned);
      if constexpr (D == 4) kernel = poly_layer_kernel<V, VEC>;
      else kernel = poly_layer_order_kernel<V, VEC, D>;
      hipLaunchKernelGGL(kernel, p.grid, dim3(256), 0, (hipStream_t)stream, img, coeffs, out, p.n);
      return 0;
    });
  });
  return hip_done("poly_layer_kernel");
}

int curl_u8hwc_to_f32chw(const uint8_t* in, float* out, int B, int H, int W, int Cin, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(in, out, B, H, W)) return rc;
  if (Cin != 3 && Cin != 4) return fail(CURL_E_SHAPE, "Cin must be 3 (RGB) or 4 (RGBA)");
  const size_t HW = (size_t)H * W;
  // (four RGBA pixels are one 16-byte load, four RGB pixels three dwords)
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, nullptr, CURL_MASK_NONE, 16, out) && on_grid(Cin == 4 ? 16 : 4, in));
  if (p.aligned) hipLaunchKernelGGL(u8hwc_to_f32chw_kernel<4>, p.grid, dim3(256), aux_lds(kResIngress, p.grid, true, static_lds<u8hwc_to_f32chw_kernel<4>>()), (hipStream_t)stream, in, out, p.n, Cin);
  else hipLaunchKernelGGL(u8hwc_to_f32chw_kernel<1>, p.grid, dim3(256), 0, (hipStream_t)stream, in, out, p.n, Cin);
  return hip_done("u8hwc_to_f32chw");
}

int curl_f32chw_to_u8hwc(const float* in, uint8_t* out, int B, int H, int W, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(in, out, B, H, W)) return rc;
  return launch_egress<kMasksNone>(in, nullptr, CURL_MASK_NONE, out, B, H, W, stream, "f32chw_to_u8hwc");
}

int curl_compose_white_u8hwc(const float* in, const void* mask, int mask_kind, uint8_t* out, int B, int H, int W,
                             curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(in, out, B, H, W)) return rc;
  if (mask_kind != CURL_MASK_U8 && mask_kind != CURL_MASK_F32) return fail(CURL_E_MASK, "mask_kind must be 1 (u8) or 2 (f32)");
  if (!mask) return fail(CURL_E_MASK, "mask is NULL");
  return launch_egress<kMasksU8F32>(in, mask, mask_kind, out, B, H, W, stream, "compose_white_u8hwc");
}

size_t curl_psnr_scratch_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  size_t blocks = ((size_t)H * W + 255) / 256;
  return (size_t)B * blocks * 2 * sizeof(float);
}

int curl_psnr_f32(const float* a, const float* b, const void* mask, int mask_kind, float* psnr, void* scratch,
                  size_t scratch_bytes, int B, int H, int W, float max_intensity, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(a, b, B, H, W)) return rc;
  if (!psnr) return fail(CURL_E_NULL, "psnr output is NULL");
  if (int rc = check_mask(mask, mask_kind)) return rc;
  if (int rc = check_scratch(scratch, scratch_bytes, curl_psnr_scratch_bytes(B, H, W), false, "scratch missing or smaller than curl_psnr_scratch_bytes"))
    return rc;
  const size_t HW = (size_t)H * W;
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, mask, mask_kind, 16, a, b));  // p.bpi <= the blocks the scratch is sized for
  hipStream_t s = (hipStream_t)stream;
  dispatch_vec_mask<kMasksAll>(p.aligned, mask_kind, [&](auto V, auto M) {
    hipLaunchKernelGGL((psnr_partial_kernel<V, M>), p.grid, dim3(256), aux_lds(kResPsnr, p.grid, V == 4, static_lds<psnr_partial_kernel<V, M>>()), s,
                       a, b, mask, (float*)scratch, p.n, p.bpi);
  });
  hipLaunchKernelGGL(psnr_final_kernel, dim3((unsigned)B), dim3(256), 0, s, (const float*)scratch, psnr, p.bpi,
                     max_intensity);
  return hip_done("psnr kernels");
}

#define MSSSIM_LEVELS 5
static unsigned ssim_tiles_x(int W) { return (unsigned)((W + SSIM_TILE - 1) / SSIM_TILE); }
static unsigned ssim_tiles(int H, int W) { return ssim_tiles_x(W) * (unsigned)((H + SSIM_TILE - 1) / SSIM_TILE); }
struct SsimPlan {
  size_t level_off[MSSSIM_LEVELS];  // float offsets of levels 1.. inside one pyramid buffer (level 0 = caller's tensor)
  size_t pyr, maps, partial, total;
};
static SsimPlan ssim_plan(int B, int C, int H, int W) {
  SsimPlan p{};
  size_t N = (size_t)B * C, acc = 0;
  for (int l = 1; l < MSSSIM_LEVELS; ++l) {
    p.level_off[l] = acc;
    acc += N * (size_t)(H >> l) * (size_t)(W >> l);
  }
  p.pyr = acc;                              // one pyramid (levels 1..4); three of them: a, b, gradient
  p.maps = N * (size_t)H * W;               // one per-pixel map at level-0 size; three of them
  p.partial = N * ssim_tiles(H, W) * 2;
  p.total = 3 * p.pyr + 3 * p.maps + p.partial;
  return p;
}
size_t curl_msssim_scratch_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return ssim_plan(B, C, H, W).total * sizeof(float);
}
static int ssim_check(const void* a, const void* b, int B, int C, int H, int W, int ws, const void* scratch, size_t bytes) {
  if (!a || !b) return fail(CURL_E_NULL, "image pointer is NULL");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CURL_E_SHAPE, "B, C, H, W must be positive");
  if ((H >> MSSSIM_LEVELS) < 1 || (W >> MSSSIM_LEVELS) < 1)  // metric.py:185-192 pools once more after the fifth level
    return fail(CURL_E_SHAPE, "MS-SSIM needs H, W >= 32 (five pyramid levels, each followed by a 2x2 pooling)");
  if ((uint64_t)H * (uint64_t)W > (1ull << 30) || (uint64_t)B * C > 65535) return fail(CURL_E_SHAPE, "image too large");
  if (ws < 1 || ws > 2 * SSIM_R + 1 || (ws & 1) == 0) return fail(CURL_E_KNOTS, "window_size must be odd and <= 11");
  return check_scratch(scratch, bytes, curl_msssim_scratch_bytes(B, C, H, W), true,
                       "scratch missing, misaligned or smaller than curl_msssim_scratch_bytes");
}
static void ssim_window(int ws, float* g) {  // metric.py:104-118: exp(-(x - ws//2)^2 / (2 sigma^2)), sigma 1.5, normalised
  float sum = 0.0f;
  for (int x = 0; x < ws; ++x) {
    g[x] = (float)exp(-(double)((x - ws / 2) * (x - ws / 2)) / (2.0 * 1.5 * 1.5));
    sum += g[x];
  }
  for (int x = 0; x < ws; ++x) g[x] /= sum;
}
// runs the forward level kernels: pyramids of a and b into scratch, per-level means into ssims/mcs when asked
static void ssim_forward_levels(const float* a, const float* b, float* ssims, float* mcs, float* scr, const SsimPlan& pl,
                                int B, int C, int H, int W, int ws, int last_level, hipStream_t s) {
  float* pyr_a = scr;
  float* pyr_b = scr + pl.pyr;
  float* partial = scr + 3 * pl.pyr + 3 * pl.maps;
  const float *la = a, *lb = b;
  for (int l = 0; l <= last_level; ++l) {
    int h = H >> l, w = W >> l;
    SsimArgs k{};
    k.a = la, k.b = lb;
    bool has_next = l + 1 < MSSSIM_LEVELS;
    k.a_next = has_next ? pyr_a + pl.level_off[l + 1] : nullptr;
    k.b_next = has_next ? pyr_b + pl.level_off[l + 1] : nullptr;
    k.partial = partial;
    k.H = h, k.W = w, k.C = C, k.level = l, k.levels = MSSSIM_LEVELS, k.radius = ws / 2;
    k.tiles_x = ssim_tiles_x(w), k.tiles = ssim_tiles(h, w);
    ssim_window(ws, k.g);
    hipLaunchKernelGGL(msssim_level_kernel<false>, dim3(k.tiles, (unsigned)(B * C)), dim3(256), 0, s, k);
    if (ssims)
      hipLaunchKernelGGL(msssim_means_kernel, dim3((unsigned)B), dim3(256), 0, s, (const float*)partial, ssims, mcs,
                         (unsigned)C * k.tiles, 1.0 / ((double)C * h * w), l, MSSSIM_LEVELS);
    la = k.a_next, lb = k.b_next;
  }
}

int curl_msssim_fwd_f32(const float* a, const float* b, float* ssims, float* mcs, void* scratch, size_t scratch_bytes,
                        int B, int C, int H, int W, int window_size, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = ssim_check(a, b, B, C, H, W, window_size, scratch, scratch_bytes)) return rc;
  if (!ssims || !mcs) return fail(CURL_E_NULL, "ssims / mcs output is NULL");
  SsimPlan pl = ssim_plan(B, C, H, W);
  ssim_forward_levels(a, b, ssims, mcs, (float*)scratch, pl, B, C, H, W, window_size, MSSSIM_LEVELS - 1, (hipStream_t)stream);
  return hip_done("msssim forward kernels");
}

int curl_msssim_bwd_f32(const float* a, const float* b, const float* g_ssims, const float* g_mcs, float* grad_a,
                        void* scratch, size_t scratch_bytes, int B, int C, int H, int W, int window_size,
                        curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = ssim_check(a, b, B, C, H, W, window_size, scratch, scratch_bytes)) return rc;
  if (!g_ssims || !g_mcs || !grad_a) return fail(CURL_E_NULL, "g_ssims / g_mcs / grad_a is NULL");
  SsimPlan pl = ssim_plan(B, C, H, W);
  hipStream_t s = (hipStream_t)stream;
  float* scr = (float*)scratch;
  // the pyramids again (stateless between the two calls): levels 1..4 of a and b
  ssim_forward_levels(a, b, nullptr, nullptr, scr, pl, B, C, H, W, window_size, MSSSIM_LEVELS - 2, s);
  if (int rc = hip_done("msssim pyramid kernels")) return rc;
  float* pyr_a = scr;
  float* pyr_b = scr + pl.pyr;
  float* pyr_g = scr + 2 * pl.pyr;
  float* maps = scr + 3 * pl.pyr;
  for (int l = MSSSIM_LEVELS - 1; l >= 0; --l) {  // coarsest first: each level adds the pooled gradient from below
    int h = H >> l, w = W >> l;
    const float* la = l ? pyr_a + pl.level_off[l] : a;
    const float* lb = l ? pyr_b + pl.level_off[l] : b;
    SsimArgs k{};
    k.a = la, k.b = lb;
    k.g_ssim = g_ssims, k.g_cs = g_mcs;
    k.d_mu = maps, k.d_e11 = maps + pl.maps, k.d_e12 = maps + 2 * pl.maps;
    k.H = h, k.W = w, k.C = C, k.level = l, k.levels = MSSSIM_LEVELS, k.radius = window_size / 2;
    k.tiles_x = ssim_tiles_x(w), k.tiles = ssim_tiles(h, w);
    ssim_window(window_size, k.g);
    hipLaunchKernelGGL(msssim_level_kernel<true>, dim3(k.tiles, (unsigned)(B * C)), dim3(256), 0, s, k);
    SsimGradArgs q{};
    q.a = la, q.b = lb, q.d_mu = k.d_mu, q.d_e11 = k.d_e11, q.d_e12 = k.d_e12;
    q.g_below = (l + 1 < MSSSIM_LEVELS) ? pyr_g + pl.level_off[l + 1] : nullptr;
    q.g_out = l ? pyr_g + pl.level_off[l] : grad_a;
    q.H = h, q.W = w, q.radius = k.radius, q.tiles_x = k.tiles_x;
    ssim_window(window_size, q.g);
    hipLaunchKernelGGL(msssim_grad_kernel, dim3(k.tiles, (unsigned)(B * C)), dim3(256), 0, s, q);
  }
  return hip_done("msssim backward kernels");
}

size_t curl_loss_terms_scratch_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (((size_t)H * W + 255) / 256) * LOSS_NSUM * sizeof(float);
}

int curl_loss_terms_f32(const float* pred, const float* target, const void* mask, int mask_kind, double* sums,
                        float* L_pred, float* L_target, void* scratch, size_t scratch_bytes, int B, int H, int W,
                        curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(pred, target, B, H, W)) return rc;
  if (!sums) return fail(CURL_E_NULL, "sums is NULL");
  if (int rc = check_mask(mask, mask_kind)) return rc;
  if (int rc = check_scratch(scratch, scratch_bytes, curl_loss_terms_scratch_bytes(B, H, W), false,
                             "scratch missing or smaller than curl_loss_terms_scratch_bytes"))
    return rc;
  const size_t HW = (size_t)H * W;
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, mask, mask_kind, 16, pred, target, L_pred, L_target));  // p.bpi <= the blocks the scratch is sized for
  hipStream_t s = (hipStream_t)stream;
  dispatch_vec_mask<kMasksAll>(p.aligned, mask_kind, [&](auto V, auto M) {
    hipLaunchKernelGGL((loss_terms_kernel<V, M>), p.grid, dim3(256), aux_lds(kResLoss, p.grid, V == 4, 0), s, pred, target, mask, (float*)scratch,
                       L_pred, L_target, p.n, p.bpi);
  });
  hipLaunchKernelGGL(loss_terms_final_kernel, dim3((unsigned)B), dim3(LOSS_FINAL_THREADS), 0, s, (const float*)scratch, sums, p.bpi);
  return hip_done("loss_terms kernels");
}

int curl_layer_loss_fwd_f32(const float* img, const void* mask, int mask_kind, const float* rawL, const float* rawR,
                            const float* rawH, const float* target, float* out, float* reg, double* sums, float* L_pred,
                            float* L_target, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                            int B, int H, int W, int Kl, int Kr, int Kh, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!target || !sums) return fail(CURL_E_NULL, "target / sums is NULL");
  if (int rc = check_mask(mask, mask_kind)) return rc;
  if (int rc = check_flags(flags, 0)) return rc;
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, true, workspace, workspace_bytes, B, reg)) return rc;
  if (int rc = check_scratch(scratch, scratch_bytes, curl_loss_terms_scratch_bytes(B, H, W), false,
                             "scratch missing or smaller than curl_loss_terms_scratch_bytes"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t HW = (size_t)H * W;
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, mask, mask_kind, 16, img, target, out, L_pred, L_target));  // p.bpi <= the blocks the scratch is sized for
  if (p.too_large()) return fail(CURL_E_SHAPE, "grid too large");
  // small launches collapse their curves inside the kernel (one launch less: launch_stream's rule and CURL_F_TUNE_PREP)
  const unsigned psel = (flags & CURL_F_TUNE_PREP_MASK) >> CURL_F_TUNE_PREP_SHIFT;
  const bool self_prep = psel == 2 || (psel == 0 && (uint64_t)p.bpi * (uint64_t)B <= kSelfPrepMaxTiles);
  if (!self_prep)
    if (int rc = launch_prep(k.prep, B, s)) return rc;
  LayerLossArgs a;
  a.img = img, a.tgt = target, a.mask = mask_kind ? mask : nullptr, a.coef = k.ws, a.out = out, a.partial = (float*)scratch;
  a.Lp = L_pred, a.Lt = L_target, a.coef_stride = k.stride, a.n = p.n, a.blocks_per_image = p.bpi;
  dispatch_vec_mask<kMasksAll>(p.aligned, mask_kind, [&](auto V, auto M) {
    if (self_prep) hipLaunchKernelGGL((layer_loss_kernel<V, M, true>), p.grid, dim3(256), 0, s, a, k.prep);
    else hipLaunchKernelGGL((layer_loss_kernel<V, M, false>), p.grid, dim3(256), 0, s, a, k.prep);
  });
  hipLaunchKernelGGL(loss_terms_final_kernel, dim3((unsigned)B), dim3(LOSS_FINAL_THREADS), 0, s, (const float*)scratch, sums, p.bpi);
  return hip_done("layer_loss kernels");
}

// `weights` is a DEVICE pointer: the host cannot look at it.  Supported: any finite float32 for the three L1 weights (0, 2, 3) --
// x = 0 (masked out, pred == target) gives exactly 0 for all of them; w sign(x) is exact for |w| <= 2^101 (|w| <= 2^78 when x
// is denormal), sign-correct beyond; |x| = |pred m - target m| < 2^27.  curl_math_loss.h signw_of, include/curl_hip.h.
int curl_loss_terms_bwd_f32(const float* pred, const float* target, const void* mask, int mask_kind,
                            const float* weights, const float* grad_L_pred, float* grad_pred, int B, int H, int W,
                            curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(pred, target, B, H, W)) return rc;
  if (!weights || !grad_pred) return fail(CURL_E_NULL, "weights / grad_pred is NULL");
  if (int rc = check_mask(mask, mask_kind)) return rc;
  const size_t HW = (size_t)H * W;
  const Pointwise p = pointwise(HW, B, planes_vec4(HW, mask, mask_kind, 16, pred, target, grad_L_pred, grad_pred));
  dispatch_vec_mask<kMasksAll>(p.aligned, mask_kind, [&](auto V, auto M) {
    hipLaunchKernelGGL((loss_terms_bwd_kernel<V, M>), p.grid, dim3(256), aux_lds(kResLossBwd, p.grid, V == 4, 0), (hipStream_t)stream, pred, target,
                       mask, weights, grad_L_pred, grad_pred, p.n);
  });
  return hip_done("loss_terms_bwd_kernel");
}

size_t curl_trispace_bwd_scratch_bytes(int B, int H, int W, int num_coeffs) {
  if (B <= 0 || H <= 0 || W <= 0 || !is_poly_count(num_coeffs, 4)) return 0;
  size_t HW = (size_t)H * W;
  return ((size_t)B * 18 * HW + (size_t)B * tri_bwd_tiles(B, H, W, num_coeffs) * 9 * num_coeffs) * sizeof(float);
}

int curl_trispace_bwd_f32(const float* img, const float* coeffs, const float* grad_out, float* grad_coeffs, void* scratch,
                          size_t scratch_bytes, int B, int H, int W, int num_coeffs, unsigned flags,
                          curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, grad_out, B, H, W)) return rc;
  if (!coeffs || !grad_coeffs) return fail(CURL_E_NULL, "coeffs / grad_coeffs is NULL");
  if (int rc = check_num_coeffs(num_coeffs, "num_coeffs must be 126 or 35")) return rc;
  if (int rc = check_flags(flags, CURL_F_RESIDUAL_ONLY)) return rc;
  if (int rc = check_coeffs_aligned(coeffs, num_coeffs)) return rc;
  if (int rc = check_scratch(scratch, scratch_bytes, curl_trispace_bwd_scratch_bytes(B, H, W, num_coeffs), true,
                             "scratch missing, misaligned or smaller than curl_trispace_bwd_scratch_bytes"))
    return rc;
  size_t HW = (size_t)H * W;
  // the accumulation pass is a 1-D grid of (image, space, tile, chunk) blocks
  if ((uint64_t)B * 3u * tri_bwd_tiles(B, H, W, num_coeffs) * 3u + 64u > 0x7fffffffull) return fail(CURL_E_SHAPE, "grid too large");
  float* pxbuf = (float*)scratch;
  float* partial = pxbuf + (size_t)B * 18 * HW;
  int ro = (flags & CURL_F_RESIDUAL_ONLY) ? 1 : 0;
  if (num_coeffs == PolyEval<5>::kCoeffs) launch_trispace_bwd<5>(img, coeffs, grad_out, grad_coeffs, pxbuf, partial, B, H, W, ro, (hipStream_t)stream);
  else launch_trispace_bwd<3>(img, coeffs, grad_out, grad_coeffs, pxbuf, partial, B, H, W, ro, (hipStream_t)stream);
  return hip_done("trispace backward kernels");
}

size_t curl_poly_layer_bwd_scratch_bytes(int B, int H, int W, int num_variables) {
  if (B <= 0 || H <= 0 || W <= 0 || !is_poly_pair(num_variables, 4)) return 0;
  const size_t HW = (size_t)H * W;
  return (size_t)B * poly_bwd_tiles(B, HW) * 3 * poly_count(num_variables, 4) * sizeof(float);
}

int curl_poly_layer_bwd_f32(const float* img, const float* coeffs, const float* grad_out, float* grad_img, float* grad_coeffs,
                            void* scratch, size_t scratch_bytes, int B, int H, int W, int num_variables, unsigned flags,
                            curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, grad_out, B, H, W)) return rc;
  if (!coeffs) return fail(CURL_E_NULL, "coeffs is NULL");
  if (!grad_img && !grad_coeffs) return fail(CURL_E_NULL, "grad_img and grad_coeffs are both NULL: nothing to compute");
  if (int rc = check_num_variables(num_variables)) return rc;
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (flags must be 0)");
  const size_t HW = (size_t)H * W;
  if (grad_coeffs) {  // the tile partials; the image gradient alone needs no scratch
    if (int rc = check_scratch(scratch, scratch_bytes, curl_poly_layer_bwd_scratch_bytes(B, H, W, num_variables), true,
                               "scratch missing, misaligned or smaller than curl_poly_layer_bwd_scratch_bytes"))
      return rc;
    // a 1-D grid of (image, tile, chunk) blocks
    if ((uint64_t)B * poly_bwd_tiles(B, HW) * 3u + 64u > 0x7fffffffull) return fail(CURL_E_SHAPE, "grid too large");
  }
  if (num_variables == 5)
    launch_poly_layer_bwd<5>(img, coeffs, grad_out, grad_img, grad_coeffs, (float*)scratch, B, HW, (hipStream_t)stream);
  else
    launch_poly_layer_bwd<3>(img, coeffs, grad_out, grad_img, grad_coeffs, (float*)scratch, B, HW, (hipStream_t)stream);
  return hip_done("poly_layer backward kernels");
}

}  // extern "C"
