// host_api_view.inc -- part of curl_kernels.hip (one translation unit; included after host_api.inc, whose argument checks
// and error text it uses).  The entry points of include/curl_hip_view.h.
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
static unsigned view_lds_bytes(const ViewArgs& a) { return a.off_stage + (unsigned)a.chunk_rows * (unsigned)(a.pitch_img + a.pitch_mask); }

static int check_view_shape(int H, int W, int size) {
  if (H <= 0 || W <= 0) return fail(CURL_E_SHAPE, "B, H, W must be positive");
  if (size < kViewMinSize || size > kViewMaxSize) return fail(CURL_E_SHAPE, "encoder view: size must be 8 .. 1024");
  if (view_plan_ints(H, W, size) == 0) return fail(CURL_E_SHAPE, "encoder view: min(H, W) / size exceeds 64");
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

}  // extern "C"
