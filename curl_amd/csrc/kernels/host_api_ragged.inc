// host_api_ragged.inc -- part of curl_kernels.hip (one translation unit; included after host_api.inc, whose argument checks,
// knot set-up and error text it uses).  The entry points of include/curl_hip_ragged.h.
// ------------------------------------------------------------------------------------------------
// host side: the byte edge for a batch of images of different sizes
// ------------------------------------------------------------------------------------------------
constexpr uint64_t kRaggedAlign = 16;     // every per-image offset (the header says why)
constexpr int kRaggedMaxImages = 65535;

// the operator a plan is tiled for: its coefficient count (0: the curve layer); the spatial order-4 model is row-tiled
struct RaggedOp {
  int count;
  bool rows;
};
static int ragged_op(int num_coeffs_or_0, RaggedOp& op) {
  op = RaggedOp{0, false};
  if (num_coeffs_or_0 == 0) return 0;
  int count, order;
  if (int rc = unpack_num_coeffs(num_coeffs_or_0, count, order)) return rc;
  op = RaggedOp{count, count == PolyEval<5>::kCoeffs};
  return 0;
}
static size_t ragged_plan_words(int B) { return kRaggedHeaderWords + (size_t)B * kRaggedDescWords; }
template <class... A>  // fail() with a message that names one of the family's functions or arenas
static int ragged_failf(int code, const char* fmt, A... a) { return snprintf(g_err, sizeof(g_err), fmt, a...), code; }
static void put64(int* p, uint64_t v) { p[0] = (int)(uint32_t)v, p[1] = (int)(uint32_t)(v >> 32); }
static uint64_t get64(const int* p) { return (uint64_t)(uint32_t)p[0] | ((uint64_t)(uint32_t)p[1] << 32); }
static uint64_t ragged_hash_word(uint64_t h, uint32_t w) {  // FNV-1a, a byte at a time
  for (int k = 0; k < 4; ++k) h = (h ^ ((w >> (8 * k)) & 0xffu)) * 1099511628211ull;
  return h;
}
// The arenas' layout, the one rule of every plan over a ragged batch (this file's and the encoder view's, host_api_view.inc):
// the images in index order, each offset rounded up to kRaggedAlign.  place() gives image i its three offsets and moves on;
// afterwards img / mask / out are the arena sizes.  align() is the rounding, for whatever else a plan lays out by the rule.
struct RaggedArenas {
  uint64_t img = 0, mask = 0, out = 0;
  static uint64_t align(uint64_t v) { return (v + kRaggedAlign - 1) & ~(kRaggedAlign - 1); }
  int place(uint64_t px, int channels, bool has_mask, uint64_t& img_off, uint64_t& mask_off, uint64_t& out_off) {
    img = align(img), out = align(out), mask = align(mask);
    img_off = img, out_off = out, mask_off = has_mask ? mask : 0;
    img += px * (uint64_t)channels, out += px * 3u, mask += has_mask ? px : 0;
    if ((img | out | mask) >> 63) return fail(CURL_E_SHAPE, "ragged batch: an arena exceeds 2^63 bytes");
    return 0;
  }
};
static bool ragged_is_dword(const RaggedOp& op, int H, int W) { return op.rows ? W % 4 == 0 : ((uint64_t)H * (uint64_t)W) % 4 == 0; }

// Row tiles of a whole launch: the block size is one per launch.  row_blocks' rule for one image -- among 64 / 128 / 192 /
// 256 lanes the one that wastes the fewest, ties to the larger -- summed over many rows always ends at 64 (a row's waste at 64
// lanes is never more than at a multiple of 64, and over a batch the ties are gone), and a 64-lane workgroup folds a row's
// 630 coefficients for one wave: measured 15 % slower than the loop of single-image calls on 32 mixed photographs, while 256
// lanes everywhere lost 19 % on 8 x 1500x1000 to the idle waves of every row's last workgroup (profiles/ragged/).  What is
// minimised is therefore the launch's wave slots PLUS its row folds: per row, segs * t / 64 waves and segs folds, a fold
// weighing half a wave's arithmetic on the dword path (256 pixels per wave) and two waves' on the byte path (64 pixels per
// wave) -- the two measurements above give 0.4 ... 0.55.  For one image this picks what row_blocks picks at 341, 512 and
// 1500 pixels per row.  Ties go to the larger.
static unsigned ragged_row_threads(int B, const int* H, const int* W, const RaggedOp& op, bool dword) {
  unsigned best_t = 256;
  uint64_t best_cost = ~0ull;
  for (unsigned t = 64; t <= 256; t += 64) {
    uint64_t cost = 0;  // in half waves
    for (int i = 0; i < B; ++i) {
      if (ragged_is_dword(op, H[i], W[i]) != dword) continue;
      const uint64_t units = (uint64_t)W[i] / (dword ? 4u : 1u), segs = (units + t - 1) / t;
      cost += (2 * segs * (t / 64) + (dword ? 1u : 4u) * segs) * (uint64_t)H[i];
    }
    if (cost <= best_cost) best_cost = cost, best_t = t;
  }
  return best_t;
}

// What every plan builder of the family asks of its arguments before it reads a size, in this order (dims_null: the message
// for a NULL size array; words / bytes_fn: the plan's size rule and the query that gives it; op: an operator's place in it).
static int ragged_plan_buffer(bool have_dims, const char* dims_null, const void* host_buf, int B, size_t bytes, size_t (*words)(int),
                              const char* bytes_fn, RaggedOp* op = nullptr, int num_coeffs_or_0 = 0) {
  if (!have_dims) return fail(CURL_E_NULL, dims_null);
  if (!host_buf) return fail(CURL_E_NULL, "host_buf is NULL");
  if (B < 1) return fail(CURL_E_SHAPE, "ragged batch: B must be positive");
  if (B > kRaggedMaxImages) return fail(CURL_E_SHAPE, "B exceeds 65535 images per call");
  if (op)
    if (int rc = ragged_op(num_coeffs_or_0, *op)) return rc;
  if ((uintptr_t)host_buf % 8) return fail(CURL_E_WORKSPACE, "ragged batch: the plan buffer must be 8-byte aligned");
  if (bytes < words(B) * sizeof(int)) return ragged_failf(CURL_E_WORKSPACE, "ragged batch: the plan buffer is too small (%s)", bytes_fn);
  return 0;
}
// ... and of every image's size
static int ragged_image_size(int H, int W) {
  if (H <= 0 || W <= 0) return fail(CURL_E_SHAPE, "ragged batch: every H and W must be positive");
  if ((uint64_t)H * (uint64_t)W > (1ull << 30)) return fail(CURL_E_SHAPE, "ragged batch: an image's H*W exceeds 2^30 pixels");
  return 0;
}

static int ragged_build(int B, const int* H, const int* W, const int* C, bool has_mask, const RaggedOp& op, int* p) {
  int n_dword = 0;
  uint64_t hash = 1469598103934665603ull;
  hash = ragged_hash_word(ragged_hash_word(ragged_hash_word(hash, (uint32_t)op.count), has_mask), (uint32_t)B);
  for (int i = 0; i < B; ++i) {
    if (int rc = ragged_image_size(H[i], W[i])) return rc;
    if (C[i] != 3 && C[i] != 4) return fail(CURL_E_SHAPE, "ragged batch: channels must be 3 (RGB) or 4 (RGBA)");
    n_dword += ragged_is_dword(op, H[i], W[i]);
    hash = ragged_hash_word(ragged_hash_word(ragged_hash_word(hash, (uint32_t)H[i]), (uint32_t)W[i]), (uint32_t)C[i]);
  }
  const unsigned threads[2] = {op.rows ? ragged_row_threads(B, H, W, op, true) : 256u,
                               op.rows ? ragged_row_threads(B, H, W, op, false) : 256u};
  memset(p, 0, ragged_plan_words(B) * sizeof(int));
  uint64_t grid[2] = {0, 0};
  RaggedArenas arenas;
  int cursor[2] = {0, n_dword};
  for (int i = 0; i < B; ++i) {
    const int cls = ragged_is_dword(op, H[i], W[i]) ? 0 : 1;
    const unsigned vec = cls == 0 ? 4u : 1u;
    const uint64_t px = (uint64_t)H[i] * (uint64_t)W[i], n = px / vec;
    uint64_t units = 0, segs = 0, tiles = (n + 255u) / 256u;
    if (op.rows) units = (uint64_t)W[i] / vec, segs = (units + threads[cls] - 1) / threads[cls], tiles = segs * (uint64_t)H[i];
    int* d = p + kRaggedHeaderWords + (size_t)cursor[cls]++ * kRaggedDescWords;
    if (grid[cls] + tiles > 0x7fffffffull) return fail(CURL_E_SHAPE, "ragged batch: a launch's grid exceeds 2^31 - 1 workgroups");
    d[RD_FIRST] = (int)grid[cls], d[RD_INDEX] = i, d[RD_H] = H[i], d[RD_W] = W[i], d[RD_CHANNELS] = C[i], d[RD_N] = (int)n;
    d[RD_UNITS] = (int)units, d[RD_SEGS] = (int)segs, d[RD_TILES] = (int)tiles;
    grid[cls] += tiles;
    uint64_t off_img, off_mask, off_out;
    if (int rc = arenas.place(px, C[i], has_mask, off_img, off_mask, off_out)) return rc;
    put64(d + RD_IMG_OFF, off_img), put64(d + RD_OUT_OFF, off_out), put64(d + RD_MASK_OFF, off_mask);
  }
  p[RH_STAMP] = (int)kRaggedStamp, p[RH_B] = B, p[RH_OP] = op.count, p[RH_HAS_MASK] = has_mask;
  p[RH_LAUNCHES] = (n_dword > 0) + (n_dword < B), p[RH_N_DWORD] = n_dword, p[RH_N_BYTE] = B - n_dword;
  p[RH_THREADS_DWORD] = n_dword > 0 ? (int)threads[0] : 0, p[RH_GRID_DWORD] = (int)grid[0];
  p[RH_THREADS_BYTE] = n_dword < B ? (int)threads[1] : 0, p[RH_GRID_BYTE] = (int)grid[1];
  put64(p + RH_IMG_BYTES, arenas.img), put64(p + RH_MASK_BYTES, arenas.mask), put64(p + RH_OUT_BYTES, arenas.out), put64(p + RH_HASH, hash);
  return 0;
}

// A host plan is the caller's memory: what the entries read from it is checked for being a plan's
static int ragged_host_plan(const void* host_plan) {
  if (!host_plan) return fail(CURL_E_NULL, "host_plan is NULL");
  if ((uintptr_t)host_plan % 8) return fail(CURL_E_WORKSPACE, "ragged batch: the host plan must be 8-byte aligned");
  const int* p = static_cast<const int*>(host_plan);
  if ((unsigned)p[RH_STAMP] != kRaggedStamp || p[RH_B] < 1 || p[RH_B] > kRaggedMaxImages || p[RH_N_DWORD] < 0 || p[RH_N_BYTE] < 0 ||
      p[RH_N_DWORD] + p[RH_N_BYTE] != p[RH_B])
    return fail(CURL_E_WORKSPACE, "ragged batch: host_plan holds no plan (curl_ragged_plan)");
  for (int c = 0; c < 2; ++c) {
    const int count = p[RH_N_DWORD + c], threads = p[RH_THREADS_DWORD + 2 * c], grid = p[RH_GRID_DWORD + 2 * c];
    if (count > 0 && (threads < 64 || threads > 256 || threads % 64 || grid < count))
      return fail(CURL_E_WORKSPACE, "ragged batch: host_plan holds no plan (curl_ragged_plan)");
  }
  return 0;
}

// what a launch entry asks of the plan, in the header's order (its host copy, flags, operator, masks, device copy); no HIP call
static int check_ragged_plan(const void* host_plan, const void* plan_dev, size_t plan_bytes, int op_count, unsigned flags, bool masks) {
  if (!plan_dev) return fail(CURL_E_NULL, "plan_dev is NULL");
  if (int rc = ragged_host_plan(host_plan)) return rc;
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (flags must be 0)");
  const int* p = static_cast<const int*>(host_plan);
  if (p[RH_OP] != op_count) return fail(CURL_E_WORKSPACE, "ragged batch: the plan was made for another operator");
  if (masks && !p[RH_HAS_MASK]) return fail(CURL_E_WORKSPACE, "ragged batch: a mask arena with a plan that was made without masks");
  if ((uintptr_t)plan_dev % 8) return fail(CURL_E_WORKSPACE, "ragged batch: plan_dev must be 8-byte aligned");
  if (plan_bytes < ragged_plan_words(p[RH_B]) * sizeof(int)) return fail(CURL_E_WORKSPACE, "ragged batch: plan_dev is too small (curl_ragged_plan_bytes)");
  return 0;
}
// ... and of the three arenas of a forward entry, behind it: each as large as the (checked) plan's, on the dword grid -> r
static int check_ragged_arenas(RaggedArgs& r, const uint8_t* img, size_t img_bytes, const uint8_t* mask, size_t mask_bytes, uint8_t* out,
                               size_t out_bytes, const void* host_plan, const void* plan_dev) {
  const int* p = static_cast<const int*>(host_plan);
  if (img_bytes < get64(p + RH_IMG_BYTES)) return fail(CURL_E_WORKSPACE, "ragged batch: the image arena is smaller than the plan's");
  if (mask && mask_bytes < get64(p + RH_MASK_BYTES)) return fail(CURL_E_WORKSPACE, "ragged batch: the mask arena is smaller than the plan's");
  if (out_bytes < get64(p + RH_OUT_BYTES)) return fail(CURL_E_WORKSPACE, "ragged batch: the out arena is smaller than the plan's");
  if (!on_grid(4, img, mask, out)) return fail(CURL_E_SHAPE, "ragged batch: the arenas must be 4-byte aligned");
  r.plan = static_cast<const int*>(plan_dev);
  r.img = img, r.mask = mask, r.out = out;
  r.img_bytes = img_bytes, r.mask_bytes = mask ? mask_bytes : 0, r.out_bytes = out_bytes;
  r.hash = get64(p + RH_HASH), r.stamp = kRaggedStamp;
  return 0;
}
// every check that the forward entries share; fg: the foreground entries', which need the masks
static int check_ragged(RaggedArgs& r, const uint8_t* img, size_t img_bytes, const uint8_t* mask, size_t mask_bytes, uint8_t* out,
                        size_t out_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, int op_count, unsigned flags,
                        bool fg = false) {
  if (!img || !out) return fail(CURL_E_NULL, "arena pointer is NULL");
  if (fg && !mask) return fail(CURL_E_MASK, "mask_arena is NULL (the foreground entries need the masks)");
  if (int rc = check_ragged_plan(host_plan, plan_dev, plan_bytes, op_count, flags, mask != nullptr)) return rc;
  return check_ragged_arenas(r, img, img_bytes, mask, mask_bytes, out, out_bytes, host_plan, plan_dev);
}

// the two kernels of a forward entry (stream_ragged_kernel's or stream_ragged_fg_kernel's): the dword and the byte class's
typedef void (*StreamRaggedKernel)(StreamArgs, const int*, const uint8_t*, const uint8_t*, uint8_t*, unsigned long long, unsigned long long,
                                   unsigned long long, unsigned long long, unsigned, unsigned, unsigned);
// one launch per non-empty class (the curve collapse first); everything is checked by now
static int launch_stream_ragged(StreamRaggedKernel dword, StreamRaggedKernel byte, RaggedArgs r, const void* host_plan, const float* coef,
                                unsigned coef_stride, hipStream_t s, const char* name, const PrepArgs* prep = nullptr) {
  const int* p = static_cast<const int*>(host_plan);
  if (prep)
    if (int rc = launch_prep(*prep, p[RH_B], s)) return rc;
  StreamArgs a{};
  a.coef = coef;
  a.coef_stride = coef_stride;
  if (p[RH_N_DWORD] > 0) {
    r.table = kRaggedHeaderWords, r.count = (unsigned)p[RH_N_DWORD];
    hipLaunchKernelGGL(dword, dim3((unsigned)p[RH_GRID_DWORD]), dim3((unsigned)p[RH_THREADS_DWORD]), 0, s, a, r.plan, r.img, r.mask, r.out, r.img_bytes,
                       r.mask_bytes, r.out_bytes, r.hash, r.stamp, r.table, r.count);
  }
  if (p[RH_N_BYTE] > 0) {
    r.table = kRaggedHeaderWords + (unsigned)p[RH_N_DWORD] * kRaggedDescWords, r.count = (unsigned)p[RH_N_BYTE];
    hipLaunchKernelGGL(byte, dim3((unsigned)p[RH_GRID_BYTE]), dim3((unsigned)p[RH_THREADS_BYTE]), 0, s, a, r.plan, r.img, r.mask, r.out, r.img_bytes,
                       r.mask_bytes, r.out_bytes, r.hash, r.stamp, r.table, r.count);
  }
  return hip_done(name);
}

// the two forward entries and, with fg, their foreground twins (host_api_ragged_fg.inc): the masks required, the _fg_ kernels
static int trispace_fwd_ragged(const uint8_t* img_arena, size_t img_bytes, const float* coeffs, const uint8_t* mask_arena, size_t mask_bytes,
                               uint8_t* out_arena, size_t out_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes,
                               int num_coeffs, unsigned flags, curl_stream_t stream, bool fg) {
  g_err[0] = 0;
  if (!coeffs) return fail(CURL_E_NULL, "coeffs is NULL");
  if (!img_arena || !out_arena) return fail(CURL_E_NULL, "arena pointer is NULL");
  int order;
  if (int rc = unpack_num_coeffs(num_coeffs, num_coeffs, order)) return rc;
  RaggedArgs r{};
  if (int rc = check_ragged(r, img_arena, img_bytes, mask_arena, mask_bytes, out_arena, out_bytes, host_plan, plan_dev, plan_bytes,
                            num_coeffs, flags, fg))
    return rc;
  if (int rc = check_coeffs_aligned(coeffs, num_coeffs)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_order(num_coeffs, [&](auto V, auto D) {
    typedef TriSpaceOp<V, D> T;
    typedef typename T::Op Op;
    if (fg)
      return launch_stream_ragged(stream_ragged_fg_kernel<Op, 4, true>, stream_ragged_fg_kernel<Op, 1, false>, r, host_plan, coeffs,
                                  T::kCoefStride, s, T::kRows ? "trispace_rows_ragged_fg_u8hwc" : "trispace_ragged_fg_u8hwc");
    return launch_stream_ragged(stream_ragged_kernel<Op, 4, true>, stream_ragged_kernel<Op, 1, false>, r, host_plan, coeffs, T::kCoefStride,
                                s, T::kRows ? "trispace_rows_ragged_u8hwc" : "trispace_ragged_u8hwc");
  });
}

static int layer_fwd_ragged(const uint8_t* img_arena, size_t img_bytes, const float* rawL, const float* rawR, const float* rawH,
                            const uint8_t* mask_arena, size_t mask_bytes, uint8_t* out_arena, size_t out_bytes, float* reg, void* workspace,
                            size_t workspace_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, int Kl, int Kr, int Kh,
                            unsigned flags, curl_stream_t stream, bool fg) {
  g_err[0] = 0;
  RaggedArgs r{};
  if (int rc = check_ragged(r, img_arena, img_bytes, mask_arena, mask_bytes, out_arena, out_bytes, host_plan, plan_dev, plan_bytes, 0,
                            flags, fg))
    return rc;
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, true, workspace, workspace_bytes, static_cast<const int*>(host_plan)[RH_B], reg))
    return rc;
  if (fg)
    return launch_stream_ragged(stream_ragged_fg_kernel<OpLayer, 4, true>, stream_ragged_fg_kernel<OpLayer, 1, false>, r, host_plan, k.ws,
                                k.stride, (hipStream_t)stream, "curl_layer_ragged_fg_u8hwc", &k.prep);
  return launch_stream_ragged(stream_ragged_kernel<OpLayer, 4, true>, stream_ragged_kernel<OpLayer, 1, false>, r, host_plan, k.ws, k.stride,
                              (hipStream_t)stream, "curl_layer_ragged_u8hwc", &k.prep);
}

extern "C" {

size_t curl_ragged_plan_bytes(int B, int num_coeffs_or_0) {
  RaggedOp op;
  if (B < 1 || B > kRaggedMaxImages || ragged_op(num_coeffs_or_0, op)) return 0;
  return ragged_plan_words(B) * sizeof(int);
}

int curl_ragged_plan(int B, const int* H, const int* W, const int* channels, int has_mask, int num_coeffs_or_0, void* host_buf,
                     size_t bytes) {
  g_err[0] = 0;
  RaggedOp op;
  if (int rc = ragged_plan_buffer(H && W && channels, "H / W / channels is NULL", host_buf, B, bytes, ragged_plan_words,
                                  "curl_ragged_plan_bytes", &op, num_coeffs_or_0))
    return rc;
  return ragged_build(B, H, W, channels, has_mask != 0, op, static_cast<int*>(host_buf));
}

int curl_ragged_arena_bytes(const void* host_plan, size_t* img_bytes, size_t* mask_bytes, size_t* out_bytes) {
  g_err[0] = 0;
  if (!img_bytes || !mask_bytes || !out_bytes) return fail(CURL_E_NULL, "img_bytes / mask_bytes / out_bytes is NULL");
  if (int rc = ragged_host_plan(host_plan)) return rc;
  const int* p = static_cast<const int*>(host_plan);
  *img_bytes = (size_t)get64(p + RH_IMG_BYTES), *mask_bytes = (size_t)get64(p + RH_MASK_BYTES), *out_bytes = (size_t)get64(p + RH_OUT_BYTES);
  return 0;
}

int curl_trispace_fwd_ragged_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* coeffs, const uint8_t* mask_arena,
                                   size_t mask_bytes, uint8_t* out_arena, size_t out_bytes, const void* host_plan,
                                   const void* plan_dev, size_t plan_bytes, int num_coeffs, unsigned flags, curl_stream_t stream) {
  return trispace_fwd_ragged(img_arena, img_bytes, coeffs, mask_arena, mask_bytes, out_arena, out_bytes, host_plan, plan_dev, plan_bytes,
                             num_coeffs, flags, stream, false);
}

int curl_layer_fwd_ragged_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* rawL, const float* rawR,
                                const float* rawH, const uint8_t* mask_arena, size_t mask_bytes, uint8_t* out_arena,
                                size_t out_bytes, float* reg, void* workspace, size_t workspace_bytes, const void* host_plan,
                                const void* plan_dev, size_t plan_bytes, int Kl, int Kr, int Kh, unsigned flags,
                                curl_stream_t stream) {
  return layer_fwd_ragged(img_arena, img_bytes, rawL, rawR, rawH, mask_arena, mask_bytes, out_arena, out_bytes, reg, workspace,
                          workspace_bytes, host_plan, plan_dev, plan_bytes, Kl, Kr, Kh, flags, stream, false);
}

}  // extern "C"

