// host_api_ragged_msssim.inc -- part of curl_kernels.hip (one translation unit; included after host_api_ragged.inc, whose
// arena rule, hash and error text it uses, and host_api.inc, whose ssim_window it uses).  The entry points of
// include/curl_hip_ragged_msssim.h.
// ------------------------------------------------------------------------------------------------
// host side: the MS-SSIM statistics of a batch of byte images of different sizes
// ------------------------------------------------------------------------------------------------
static size_t ms_plan_words(int B) { return kMsHeaderWords + (size_t)B * kMsDescWords; }

// The two plans of this layout: the MS-SSIM statistics' and the CURLLoss statistics' (include/curl_hip_ragged_loss.h,
// host_api_ragged_loss.inc), which walks the same pyramid on one channel and adds the level-0 workgroups' term sums.
// A kind is everything in which the two families of entries differ on the host, their kernels apart.
struct MsPlanKind {
  unsigned stamp, op;
  unsigned planes;  // float planes per pyramid level: a's three and b's / prediction L and target L
  unsigned terms;   // float64 per level-0 workgroup behind the pairs (their byte offset: header word LH_TERMS_OFF, loss_ragged.inc)
  unsigned rows;    // rows of five float64 per image in the entry's stats
  const char* what;
  const char* a_name;  // what the messages call the two arenas
  const char* b_name;
  const char* plan_fn;  // ... and the functions they point the caller to
  const char* plan_bytes_fn;
  const char* workspace_fn;
};
static const MsPlanKind kMsPlan{kMsStamp, kMsOp, 6u, 0u, 2u, "ragged MS-SSIM", "a", "b", "curl_msssim_ragged_plan",
                                "curl_msssim_ragged_plan_bytes", "curl_msssim_ragged_workspace_bytes"};

static int ms_build(const MsPlanKind& kind, int B, const int* H, const int* W, bool has_mask, int* p) {
  uint64_t hash = 1469598103934665603ull;
  hash = ragged_hash_word(ragged_hash_word(ragged_hash_word(hash, kind.stamp), has_mask), (uint32_t)B);
  for (int i = 0; i < B; ++i) {
    if (int rc = ragged_image_size(H[i], W[i])) return rc;
    if ((H[i] >> MSSSIM_LEVELS) < 1 || (W[i] >> MSSSIM_LEVELS) < 1)  // metric.py:185-192 pools once more after the fifth level
      return ragged_failf(CURL_E_SHAPE, "%s: image %d is %dx%d; MS-SSIM needs H, W >= 32 (five pyramid levels, each followed by a 2x2 pooling)",
                          kind.what, i, H[i], W[i]);
    hash = ragged_hash_word(ragged_hash_word(hash, (uint32_t)H[i]), (uint32_t)W[i]);
  }
  memset(p, 0, ms_plan_words(B) * sizeof(int));
  uint64_t grid[kMsLevels] = {0, 0, 0, 0, 0}, planes = 0;
  RaggedArenas arenas;
  for (int i = 0; i < B; ++i) {
    int* d = p + kMsHeaderWords + (size_t)i * kMsDescWords;
    d[MD_INDEX] = i, d[MD_H] = H[i], d[MD_W] = W[i];
    uint64_t off_img, off_mask, off_rgb;
    if (int rc = arenas.place((uint64_t)H[i] * (uint64_t)W[i], 3, has_mask, off_img, off_mask, off_rgb)) return rc;
    put64(d + MD_RGB_OFF, off_rgb), put64(d + MD_MASK_OFF, off_mask);
    for (int l = 0; l < kMsLevels; ++l) {
      int* v = d + kMsLevelWord + l * kMsLevelWords;
      const int h = H[i] >> l, w = W[i] >> l;
      const uint64_t tiles = (uint64_t)ssim_tiles(h, w);
      if (grid[l] + tiles > 0x7fffffffull) return fail(CURL_E_SHAPE, "ragged batch: a launch's grid exceeds 2^31 - 1 workgroups");
      v[ML_H] = h, v[ML_W] = w, v[ML_TILES_X] = (int)ssim_tiles_x(w), v[ML_TILES] = (int)tiles, v[ML_FIRST] = (int)grid[l];
      grid[l] += tiles;
      if (l >= 1) {
        planes = RaggedArenas::align(planes);
        put64(v + ML_PLANES, planes);
        planes += (uint64_t)kind.planes * sizeof(float) * (uint64_t)h * (uint64_t)w;
      }
    }
  }
  uint64_t pair0[kMsLevels], pairs = 0;
  for (int l = 0; l < kMsLevels; ++l) pair0[l] = pairs, pairs += grid[l];
  if (pairs > 0x7fffffffull) return fail(CURL_E_SHAPE, "ragged batch: a launch's grid exceeds 2^31 - 1 workgroups");
  for (int i = 0; i < B; ++i)
    for (int l = 0; l < kMsLevels; ++l) {
      int* v = p + kMsHeaderWords + (size_t)i * kMsDescWords + kMsLevelWord + l * kMsLevelWords;
      v[ML_PAIR] = (int)(pair0[l] + (uint64_t)v[ML_FIRST]);
    }
  planes = RaggedArenas::align(planes);
  p[MH_STAMP] = (int)kind.stamp, p[MH_B] = B, p[MH_OP] = (int)kind.op, p[MH_HAS_MASK] = has_mask, p[MH_LAUNCHES] = kMsLevels + 1;
  for (int l = 0; l < kMsLevels; ++l) p[MH_GRID0 + l] = (int)grid[l], p[MH_PAIR0 + l] = (int)pair0[l];
  put64(p + MH_RGB_BYTES, arenas.out), put64(p + MH_MASK_BYTES, arenas.mask), put64(p + MH_HASH, hash);
  const uint64_t terms_off = planes + pairs * 2 * sizeof(double);
  put64(p + MH_PARTIAL_OFF, planes), put64(p + MH_WS_BYTES, terms_off + grid[0] * kind.terms * sizeof(double));
  if (kind.terms) put64(p + LH_TERMS_OFF, terms_off);
  return 0;
}

// A host plan is the caller's memory: what the entries read from it is checked for being a plan's
static int ms_host_plan(const MsPlanKind& kind, const void* host_plan) {
  if (!host_plan) return fail(CURL_E_NULL, "host_plan is NULL");
  if ((uintptr_t)host_plan % 8) return fail(CURL_E_WORKSPACE, "ragged batch: the host plan must be 8-byte aligned");
  const int* p = static_cast<const int*>(host_plan);
  bool ok = (unsigned)p[MH_STAMP] == kind.stamp && p[MH_B] >= 1 && p[MH_B] <= kRaggedMaxImages;
  uint64_t pairs = 0;
  for (int l = 0; ok && l < kMsLevels; ++l) {
    ok = p[MH_GRID0 + l] >= p[MH_B] && (uint64_t)(unsigned)p[MH_PAIR0 + l] == pairs;
    pairs += (uint64_t)(unsigned)p[MH_GRID0 + l];
  }
  const uint64_t terms_off = get64(p + MH_PARTIAL_OFF) + pairs * 2 * sizeof(double);
  ok = ok && get64(p + MH_PARTIAL_OFF) % 8 == 0 && (!kind.terms || get64(p + LH_TERMS_OFF) == terms_off) &&
       get64(p + MH_WS_BYTES) == terms_off + (uint64_t)(unsigned)p[MH_GRID0] * kind.terms * sizeof(double);
  if (!ok) return ragged_failf(CURL_E_WORKSPACE, "%s: host_plan holds no plan (%s)", kind.what, kind.plan_fn);
  return 0;
}

// the three host-only functions of a kind: *_plan_bytes, *_plan, *_workspace_bytes
static size_t ms_plan_bytes(int B) { return B < 1 || B > kRaggedMaxImages ? 0 : ms_plan_words(B) * sizeof(int); }
static int ms_plan(const MsPlanKind& kind, int B, const int* H, const int* W, int has_mask, void* host_buf, size_t bytes) {
  g_err[0] = 0;
  if (int rc = ragged_plan_buffer(H && W, "H / W is NULL", host_buf, B, bytes, ms_plan_words, kind.plan_bytes_fn)) return rc;
  return ms_build(kind, B, H, W, has_mask != 0, static_cast<int*>(host_buf));
}
static size_t ms_workspace_bytes(const MsPlanKind& kind, const void* host_plan) {
  const int rc = ms_host_plan(kind, host_plan);
  g_err[0] = 0;
  if (rc || static_cast<const int*>(host_plan)[MH_OP] != (int)kind.op) return 0;
  return (size_t)get64(static_cast<const int*>(host_plan) + MH_WS_BYTES);
}

// every check of a kind's launch entry: the forward entries' on this layout's plan, then the entry's own; no HIP call
static int ms_check(const MsPlanKind& kind, const uint8_t* a_arena, size_t a_bytes, const uint8_t* b_arena, size_t b_bytes,
                    const uint8_t* mask_arena, size_t mask_bytes, const double* stats, size_t stats_bytes, const void* workspace,
                    size_t workspace_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, int window_size, unsigned flags) {
  g_err[0] = 0;
  if (!a_arena || !b_arena) return fail(CURL_E_NULL, "arena pointer is NULL");
  if (!plan_dev) return fail(CURL_E_NULL, "plan_dev is NULL");
  if (int rc = ms_host_plan(kind, host_plan)) return rc;
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (flags must be 0)");
  const int* p = static_cast<const int*>(host_plan);
  if (p[MH_OP] != (int)kind.op) return fail(CURL_E_WORKSPACE, "ragged batch: the plan was made for another operator");
  if (mask_arena && !p[MH_HAS_MASK]) return fail(CURL_E_WORKSPACE, "ragged batch: a mask arena with a plan that was made without masks");
  if ((uintptr_t)plan_dev % 8) return fail(CURL_E_WORKSPACE, "ragged batch: plan_dev must be 8-byte aligned");
  if (plan_bytes < ms_plan_words(p[MH_B]) * sizeof(int))
    return ragged_failf(CURL_E_WORKSPACE, "ragged batch: plan_dev is too small (%s)", kind.plan_bytes_fn);
  const uint64_t rgb_bytes = get64(p + MH_RGB_BYTES);
  const size_t image_stats = kind.rows * kMsLevels * sizeof(double);
  if (a_bytes < rgb_bytes) return ragged_failf(CURL_E_WORKSPACE, "%s: the %s arena is smaller than the plan's", kind.what, kind.a_name);
  if (b_bytes < rgb_bytes) return ragged_failf(CURL_E_WORKSPACE, "%s: the %s arena is smaller than the plan's", kind.what, kind.b_name);
  if (mask_arena && mask_bytes < get64(p + MH_MASK_BYTES)) return fail(CURL_E_WORKSPACE, "ragged batch: the mask arena is smaller than the plan's");
  if (!stats) return ragged_failf(CURL_E_WORKSPACE, "%s: stats is NULL", kind.what);
  if ((uintptr_t)stats % 8) return ragged_failf(CURL_E_WORKSPACE, "%s: stats must be 8-byte aligned", kind.what);
  if (stats_bytes < (size_t)p[MH_B] * image_stats)
    return ragged_failf(CURL_E_WORKSPACE, "%s: stats is too small (%u bytes per image)", kind.what, (unsigned)image_stats);
  if (!workspace) return ragged_failf(CURL_E_WORKSPACE, "%s: workspace is NULL", kind.what);
  if ((uintptr_t)workspace % 8) return ragged_failf(CURL_E_WORKSPACE, "%s: workspace must be 8-byte aligned", kind.what);
  if (workspace_bytes < get64(p + MH_WS_BYTES))
    return ragged_failf(CURL_E_WORKSPACE, "%s: workspace is too small (%s)", kind.what, kind.workspace_fn);
  if (!on_grid(4, a_arena, b_arena, mask_arena)) return fail(CURL_E_SHAPE, "ragged batch: the arenas must be 4-byte aligned");
  if (window_size < 1 || window_size > 2 * SSIM_R + 1 || (window_size & 1) == 0) return fail(CURL_E_KNOTS, "window_size must be odd and <= 11");
  return 0;
}

// what the six launches of an entry share, read from the (checked) arguments
struct MsCall {
  hipStream_t s;
  const int* p;     // the host plan
  const int* plan;  // its device copy
  unsigned char* ws;
  double* partial;
  unsigned long long partial_off, hash, mask_bytes;
  unsigned B;
  MsCall(const void* host_plan, const void* plan_dev, void* workspace, const uint8_t* mask_arena, size_t mask_bytes_, curl_stream_t stream)
      : s((hipStream_t)stream), p(static_cast<const int*>(host_plan)), plan(static_cast<const int*>(plan_dev)),
        ws(static_cast<unsigned char*>(workspace)), partial_off(get64(p + MH_PARTIAL_OFF)), hash(get64(p + MH_HASH)),
        mask_bytes(mask_arena ? mask_bytes_ : 0), B((unsigned)p[MH_B]) {
    partial = reinterpret_cast<double*>(ws + partial_off);
  }
};

// the six launches: bytes(grid, first pair), four times level(grid, first pair) with win.level set, finish(pairs): the kind's kernels
template <class Bytes, class Level, class Finish>
static int ms_launch(const MsCall& c, SsimArgs& win, int window_size, const char* name, Bytes bytes, Level level, Finish finish) {
  win.levels = kMsLevels, win.radius = window_size / 2;  // the window and the level: everything else travels beside it
  unsigned pairs = 0;
  for (int l = 0; l < kMsLevels; ++l) {
    const unsigned grid = (unsigned)c.p[MH_GRID0 + l];
    double* first = c.partial + 2 * (size_t)(unsigned)c.p[MH_PAIR0 + l];
    win.level = l;
    if (l == 0) bytes(grid, first);
    else level(grid, first);
    pairs += grid;
  }
  finish(pairs);
  return hip_done(name);
}

extern "C" {

size_t curl_msssim_ragged_plan_bytes(int B) { return ms_plan_bytes(B); }

int curl_msssim_ragged_plan(int B, const int* H, const int* W, int has_mask, void* host_buf, size_t bytes) {
  return ms_plan(kMsPlan, B, H, W, has_mask, host_buf, bytes);
}

size_t curl_msssim_ragged_workspace_bytes(const void* host_plan) { return ms_workspace_bytes(kMsPlan, host_plan); }

int curl_msssim_ragged_u8hwc(const uint8_t* a_arena, size_t a_bytes, const uint8_t* b_arena, size_t b_bytes,
                             const uint8_t* mask_arena, size_t mask_bytes, double* stats, size_t stats_bytes, void* workspace,
                             size_t workspace_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, int window_size,
                             unsigned flags, curl_stream_t stream) {
  if (int rc = ms_check(kMsPlan, a_arena, a_bytes, b_arena, b_bytes, mask_arena, mask_bytes, stats, stats_bytes, workspace, workspace_bytes,
                        host_plan, plan_dev, plan_bytes, window_size, flags))
    return rc;
  const MsCall c(host_plan, plan_dev, workspace, mask_arena, mask_bytes, stream);
  SsimArgs win{};
  ssim_window(window_size, win.g);
  return ms_launch(
      c, win, window_size, "curl_msssim_ragged_u8hwc",
      [&](unsigned grid, double* first) {
        hipLaunchKernelGGL(msssim_ragged_bytes_kernel, dim3(grid), dim3(256), 0, c.s, win, c.plan, a_arena, b_arena, mask_arena, c.ws, first,
                           (unsigned long long)a_bytes, (unsigned long long)b_bytes, c.mask_bytes, c.partial_off, c.hash, kMsStamp, c.B);
      },
      [&](unsigned grid, double* first) {
        hipLaunchKernelGGL(msssim_ragged_level_kernel, dim3(grid), dim3(256), 0, c.s, win, c.plan, c.ws, first, c.partial_off, c.hash, kMsStamp,
                           c.B);
      },
      [&](unsigned pairs) {
        hipLaunchKernelGGL(msssim_ragged_finish_kernel, dim3(c.B), dim3(256), 0, c.s, c.plan, (const double*)c.partial, stats, c.hash, kMsStamp,
                           c.B, pairs);
      });
}

}  // extern "C"

