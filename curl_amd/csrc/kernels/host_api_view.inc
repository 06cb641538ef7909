// host_api_view.inc -- part of curl_kernels.hip (one translation unit; included after host_api.inc, whose argument checks
// and error text it uses, and after host_api_ragged.inc, whose arena layout the batch entries share).  The entry points of
// include/curl_hip_view.h and include/curl_hip_view_ragged.h.
// ------------------------------------------------------------------------------------------------
// host side: the encoder's view from image bytes
// ------------------------------------------------------------------------------------------------
constexpr unsigned kViewLdsBudget = 48u * 1024u;  // of the CU's 160 KiB: three workgroups share a CU at the very least

// The tile and its LDS.  Columns: 32 per tile (a row of a tile is one 128-byte store per plane), halved while the X rows, one
// output row's window of horizontal results and one staged input row do not fit (only beyond ~60x shrinking).  Rows: as many
// as keep the window near 32 input rows -- 8 at the 3.1x of a 1500 x 1000 photograph, 400 workgroups per image --, 16 at
// most, halved while the budget is exceeded.  What is left of the budget stages input rows, a chunk at a time.
static int view_tiling(ViewArgs& a, int H, int W, int size, int C, bool has_mask) {
  const ViewGeometry g = view_geometry(H, W, size);
  const ViewAxis ax = view_axis(W, g.ow), ay = view_axis(H, g.oh);
  a.ksx = ax.ksize, a.ksy = ay.ksize;
  // the samples between the first tap of output n0 and the last tap of output n0 + n - 1: floor(c + s + .5) - floor(c' - s + .5)
  // < (n - 1) scale + 2 s + 1
  const auto window = [](int n, const ViewAxis& x) { return (int)((n - 1) * x.scale + 2.0 * x.support) + 2; };
  const auto imin = [](int x, int y) { return x < y ? x : y; };
  const auto align4 = [](unsigned v) { return (v + 3u) & ~3u; };
  const auto fixed = [&](int tc_log2, int tr) {  // table rows + horizontal results
    const int tc = 1 << tc_log2;
    return 4u * (unsigned)(tc * view_lds_row(ax.ksize) + tr * view_lds_row(ay.ksize) + window(tr, ay) * tc);
  };
  const auto row_bytes = [&](int tc_log2, unsigned& pi, unsigned& pm) {
    const int cols = window(imin(1 << tc_log2, size), ax);
    pi = align4((unsigned)(cols * C) + 3u), pm = has_mask ? align4((unsigned)cols + 3u) : 0u;
    return pi + pm;
  };
  unsigned pi, pm;
  int tc_log2 = 5;
  while (tc_log2 > 0 && fixed(tc_log2, 1) + row_bytes(tc_log2, pi, pm) > kViewLdsBudget) --tc_log2;
  if (fixed(tc_log2, 1) + row_bytes(tc_log2, pi, pm) > kViewLdsBudget) return fail(CURL_E_SHAPE, "encoder view: the resampling window does not fit the LDS budget");
  int tr = 16;
  while (tr > 1 && (tr * ay.support > 32.0 || fixed(tc_log2, tr) + imin(window(tr, ay), 4) * row_bytes(tc_log2, pi, pm) > kViewLdsBudget)) tr >>= 1;
  const unsigned rb = row_bytes(tc_log2, pi, pm), fx = fixed(tc_log2, tr);
  a.tc_log2 = tc_log2, a.tr = tr;
  a.ncols_cap = window(imin(1 << tc_log2, size), ax), a.nrows_cap = window(tr, ay);
  a.chunk_rows = imin(a.nrows_cap, (int)((kViewLdsBudget - fx) / rb));
  a.pitch_img = (int)pi, a.pitch_mask = (int)pm;
  view_layout(a);
  return 0;
}
static int check_view_shape(int H, int W, int size) {
  if (H <= 0 || W <= 0) return fail(CURL_E_SHAPE, "B, H, W must be positive");
  if (size < kViewMinSize || size > kViewMaxSize) return fail(CURL_E_SHAPE, "encoder view: size must be 8 .. 1024");
  if (view_plan_ints(H, W, size) == 0) return fail(CURL_E_SHAPE, "encoder view: min(H, W) / size exceeds 64");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// host side: the views of a batch of images of different sizes (include/curl_hip_view_ragged.h)
// ------------------------------------------------------------------------------------------------
static size_t view_ragged_fixed_words(int B) { return kViewRaggedHeaderWords + (size_t)B * kViewRaggedDescWords; }
static uint64_t view_ragged_key(int H, int W) { return ((uint64_t)(uint32_t)H << 32) | (uint32_t)W; }
// the words view_build_plan writes after its header for this shape: the two tables
static size_t view_table_words(int H, int W, int size) { return view_plan_ints(H, W, size) - (size_t)kViewHeaderInts; }

// The distinct shapes of a batch, sorted (images of one shape share one pair of tables), and the plan's words; 0 outside the
// limits.  No text: curl_encoder_view_ragged_plan names the limit.
static size_t view_ragged_plan_words(int B, const int* H, const int* W, int size, std::vector<uint64_t>& keys) {
  keys.clear();
  if (B < 1 || B > kRaggedMaxImages || !H || !W) return 0;
  keys.reserve((size_t)B);
  for (int i = 0; i < B; ++i) {
    if (view_plan_ints(H[i], W[i], size) == 0 || (uint64_t)H[i] * (uint64_t)W[i] > (1ull << 30)) return 0;
    keys.push_back(view_ragged_key(H[i], W[i]));
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  size_t words = view_ragged_fixed_words(B);
  for (uint64_t k : keys) words += view_table_words((int)(k >> 32), (int)(uint32_t)k, size);
  return words;
}

// A host plan is the caller's memory: what the launch entry reads from it is checked for being a plan's
static int view_ragged_host_plan(const void* host_plan) {
  if (!host_plan) return fail(CURL_E_NULL, "host_plan is NULL");
  if ((uintptr_t)host_plan % 8) return fail(CURL_E_WORKSPACE, "encoder views: the host plan must be 8-byte aligned");
  const int* p = static_cast<const int*>(host_plan);
  if ((unsigned)p[VH_STAMP] != kViewRaggedStamp || p[VH_B] < 1 || p[VH_B] > kRaggedMaxImages || p[VH_SIZE] < kViewMinSize ||
      p[VH_SIZE] > kViewMaxSize || p[VH_GRID] < p[VH_B] || p[VH_LDS] < 1 || (unsigned)p[VH_LDS] > kViewLdsBudget ||
      get64(p + VH_PLAN_BYTES) < view_ragged_fixed_words(p[VH_B]) * sizeof(int))
    return fail(CURL_E_WORKSPACE, "encoder views: host_plan holds no plan (curl_encoder_view_ragged_plan)");
  return 0;
}

extern "C" {

size_t curl_encoder_view_plan_bytes(int H, int W, int size) { return view_plan_ints(H, W, size) * sizeof(int); }

int curl_encoder_view_plan(int H, int W, int size, void* host_buf, size_t bytes) {
  g_err[0] = 0;
  if (!host_buf) return fail(CURL_E_NULL, "host_buf is NULL");
  if (int rc = check_view_shape(H, W, size)) return rc;
  if ((uintptr_t)host_buf % 4) return fail(CURL_E_WORKSPACE, "encoder view: the plan buffer must be 4-byte aligned");
  if (bytes < curl_encoder_view_plan_bytes(H, W, size)) return fail(CURL_E_WORKSPACE, "encoder view: the plan buffer is too small (curl_encoder_view_plan_bytes)");
  view_build_plan(H, W, size, static_cast<int*>(host_buf));
  return 0;
}

int curl_encoder_view_u8hwc(const unsigned char* img, int channels, const unsigned char* mask, const void* plan_dev, size_t plan_bytes,
                            float* view, float* mask_view, int B, int H, int W, int size, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, view, B, H, W)) return rc;
  if (!plan_dev) return fail(CURL_E_NULL, "plan_dev is NULL");
  if (channels != 3 && channels != 4) return fail(CURL_E_SHAPE, "channels must be 3 (RGB) or 4 (RGBA)");
  if (int rc = check_view_shape(H, W, size)) return rc;
  if ((mask == nullptr) != (mask_view == nullptr)) return fail(CURL_E_MASK, "mask and mask_view must both be set or both be NULL");
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (flags must be 0)");
  if ((uintptr_t)plan_dev % 4) return fail(CURL_E_WORKSPACE, "encoder view: the plan must be 4-byte aligned");
  if (plan_bytes < curl_encoder_view_plan_bytes(H, W, size)) return fail(CURL_E_WORKSPACE, "encoder view: the plan is too small (curl_encoder_view_plan_bytes)");
  if ((uintptr_t)view % 4 || (uintptr_t)mask_view % 4) return fail(CURL_E_SHAPE, "view / mask_view must be 4-byte aligned");
  ViewArgs a = {};
  a.img = img, a.mask = mask, a.plan = static_cast<const int*>(plan_dev), a.view = view, a.mask_view = mask_view;
  a.H = H, a.W = W, a.size = size, a.C = channels;
  if (int rc = view_tiling(a, H, W, size, channels, mask != nullptr)) return rc;
  const unsigned tiles_y = (unsigned)((size + a.tr - 1) / a.tr);
  hipLaunchKernelGGL(encoder_view_kernel, dim3((unsigned)a.tiles_x * tiles_y, (unsigned)B), dim3(256), view_lds_bytes(a), (hipStream_t)stream, img, mask,
                     a.plan, view, mask_view, H, W, size, channels, a.ksx, a.ksy, a.tc_log2, a.tr, a.ncols_cap, a.nrows_cap, a.chunk_rows, a.pitch_img,
                     a.pitch_mask);
  return hip_done("encoder_view_kernel");
}

size_t curl_encoder_view_ragged_plan_bytes(int B, const int* H, const int* W, int size) {
  std::vector<uint64_t> keys;
  return view_ragged_plan_words(B, H, W, size, keys) * sizeof(int);
}

int curl_encoder_view_ragged_plan(int B, const int* H, const int* W, const int* channels, int has_mask, int size, void* host_buf,
                                  size_t bytes) {
  g_err[0] = 0;
  if (!H || !W || !channels) return fail(CURL_E_NULL, "H / W / channels is NULL");
  if (!host_buf) return fail(CURL_E_NULL, "host_buf is NULL");
  if (B < 1) return fail(CURL_E_SHAPE, "encoder views: B must be positive");
  if (B > kRaggedMaxImages) return fail(CURL_E_SHAPE, "B exceeds 65535 images per call");
  for (int i = 0; i < B; ++i) {
    if (int rc = check_view_shape(H[i], W[i], size)) return rc;
    if ((uint64_t)H[i] * (uint64_t)W[i] > (1ull << 30)) return fail(CURL_E_SHAPE, "encoder views: an image's H*W exceeds 2^30 pixels");
    if (channels[i] != 3 && channels[i] != 4) return fail(CURL_E_SHAPE, "encoder views: channels must be 3 (RGB) or 4 (RGBA)");
  }
  std::vector<uint64_t> keys;
  const size_t words = view_ragged_plan_words(B, H, W, size, keys);
  if ((uintptr_t)host_buf % 8) return fail(CURL_E_WORKSPACE, "encoder views: the plan buffer must be 8-byte aligned");
  if (words == 0 || bytes < words * sizeof(int))
    return fail(CURL_E_WORKSPACE, "encoder views: the plan buffer is too small (curl_encoder_view_ragged_plan_bytes)");

  // every image's tiling first (it can refuse, and nothing is written then)
  std::vector<ViewArgs> tilings((size_t)B);
  uint64_t grid = 0;
  unsigned lds = 0;
  for (int i = 0; i < B; ++i) {
    ViewArgs& a = tilings[(size_t)i];
    a = ViewArgs{};
    a.H = H[i], a.W = W[i], a.size = size, a.C = channels[i];
    if (int rc = view_tiling(a, H[i], W[i], size, channels[i], has_mask != 0)) return rc;
    grid += (uint64_t)a.tiles_x * (uint64_t)((size + a.tr - 1) / a.tr);
    lds = std::max(lds, view_lds_bytes(a));
  }
  if (grid > 0x7fffffffull) return fail(CURL_E_SHAPE, "encoder views: the grid exceeds 2^31 - 1 workgroups");

  int* p = static_cast<int*>(host_buf);
  memset(p, 0, view_ragged_fixed_words(B) * sizeof(int));
  uint64_t hash = 1469598103934665603ull;
  hash = ragged_hash_word(ragged_hash_word(ragged_hash_word(hash, (uint32_t)size), has_mask != 0), (uint32_t)B);
  std::vector<uint64_t> table_of(keys.size(), 0);  // the first word of a shape's tables, once they are written
  std::vector<int> one;                            // a single-image plan: its header, then the tables
  RaggedArenas arenas;
  uint64_t first = 0, next_table = view_ragged_fixed_words(B);
  for (int i = 0; i < B; ++i) {
    const ViewArgs& a = tilings[(size_t)i];
    hash = ragged_hash_word(ragged_hash_word(ragged_hash_word(hash, (uint32_t)H[i]), (uint32_t)W[i]), (uint32_t)channels[i]);
    const size_t k = (size_t)(std::lower_bound(keys.begin(), keys.end(), view_ragged_key(H[i], W[i])) - keys.begin());
    const size_t table_words = view_table_words(H[i], W[i], size);
    if (table_of[k] == 0) {
      one.resize(table_words + (size_t)kViewHeaderInts);
      view_build_plan(H[i], W[i], size, one.data());
      memcpy(p + next_table, one.data() + kViewHeaderInts, table_words * sizeof(int));
      table_of[k] = next_table, next_table += table_words;
    }
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((size + a.tr - 1) / a.tr);
    int* d = p + kViewRaggedHeaderWords + (size_t)i * kViewRaggedDescWords;
    d[VD_FIRST] = (int)first, d[VD_INDEX] = i, d[VD_H] = H[i], d[VD_W] = W[i], d[VD_CHANNELS] = channels[i], d[VD_TILES] = (int)tiles;
    d[VD_KSX] = a.ksx, d[VD_KSY] = a.ksy, d[VD_TC_LOG2] = a.tc_log2, d[VD_TR] = a.tr, d[VD_NCOLS_CAP] = a.ncols_cap, d[VD_NROWS_CAP] = a.nrows_cap;
    d[VD_CHUNK_ROWS] = a.chunk_rows, d[VD_PITCH_IMG] = a.pitch_img, d[VD_PITCH_MASK] = a.pitch_mask, d[VD_LDS] = (int)view_lds_bytes(a);
    put64(d + VD_TABLE, table_of[k]), d[VD_TABLE_WORDS] = (int)table_words;
    first += tiles;
    uint64_t off_img, off_mask, off_out;
    if (int rc = arenas.place((uint64_t)H[i] * (uint64_t)W[i], channels[i], has_mask != 0, off_img, off_mask, off_out)) return rc;
    put64(d + VD_IMG_OFF, off_img), put64(d + VD_MASK_OFF, off_mask);
  }
  p[VH_STAMP] = (int)kViewRaggedStamp, p[VH_B] = B, p[VH_SIZE] = size, p[VH_HAS_MASK] = has_mask != 0, p[VH_GRID] = (int)grid, p[VH_LDS] = (int)lds;
  p[VH_TABLES] = (int)keys.size();
  put64(p + VH_IMG_BYTES, arenas.img), put64(p + VH_MASK_BYTES, arenas.mask), put64(p + VH_HASH, hash);
  put64(p + VH_PLAN_BYTES, (uint64_t)words * sizeof(int));
  return 0;
}

int curl_encoder_view_ragged_u8hwc(const uint8_t* img_arena, size_t img_bytes, const uint8_t* mask_arena, size_t mask_bytes,
                                   const void* host_plan, const void* plan_dev, size_t plan_bytes, float* view, float* mask_view, int size,
                                   unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (!img_arena) return fail(CURL_E_NULL, "arena pointer is NULL");
  if (!view) return fail(CURL_E_NULL, "view is NULL");
  if (!plan_dev) return fail(CURL_E_NULL, "plan_dev is NULL");
  if (int rc = view_ragged_host_plan(host_plan)) return rc;
  if ((mask_arena == nullptr) != (mask_view == nullptr)) return fail(CURL_E_MASK, "mask_arena and mask_view must both be set or both be NULL");
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (flags must be 0)");
  const int* p = static_cast<const int*>(host_plan);
  if (p[VH_SIZE] != size) return fail(CURL_E_WORKSPACE, "encoder views: the plan was made for another size");
  if (mask_arena && !p[VH_HAS_MASK]) return fail(CURL_E_WORKSPACE, "encoder views: a mask arena with a plan that was made without masks");
  if ((uintptr_t)plan_dev % 8) return fail(CURL_E_WORKSPACE, "encoder views: plan_dev must be 8-byte aligned");
  if (plan_bytes < get64(p + VH_PLAN_BYTES)) return fail(CURL_E_WORKSPACE, "encoder views: plan_dev is too small (curl_encoder_view_ragged_plan_bytes)");
  if (img_bytes < get64(p + VH_IMG_BYTES)) return fail(CURL_E_WORKSPACE, "encoder views: the image arena is smaller than the plan's");
  if (mask_arena && mask_bytes < get64(p + VH_MASK_BYTES)) return fail(CURL_E_WORKSPACE, "encoder views: the mask arena is smaller than the plan's");
  if ((uintptr_t)view % 4 || (uintptr_t)mask_view % 4) return fail(CURL_E_SHAPE, "view / mask_view must be 4-byte aligned");
  hipLaunchKernelGGL(encoder_view_ragged_kernel, dim3((unsigned)p[VH_GRID]), dim3(256), (unsigned)p[VH_LDS], (hipStream_t)stream,
                     static_cast<const int*>(plan_dev), img_arena, mask_arena, view, mask_view, (unsigned long long)img_bytes,
                     (unsigned long long)(mask_arena ? mask_bytes : 0), (unsigned long long)(get64(p + VH_PLAN_BYTES) / sizeof(int)),
                     (unsigned long long)get64(p + VH_HASH), kViewRaggedStamp, (unsigned)p[VH_B], size, (unsigned)p[VH_LDS]);
  return hip_done("encoder_view_ragged_kernel");
}

}  // extern "C"
