// host_api_ragged_loss.inc -- part of curl_kernels.hip (one translation unit; included after host_api_ragged_msssim.inc, whose
// plan builder and plan check it uses with a kind of its own).  The entry points of include/curl_hip_ragged_loss.h.
// ------------------------------------------------------------------------------------------------
// host side: the CURLLoss statistics of a batch of byte images of different sizes
// ------------------------------------------------------------------------------------------------
static const MsPlanKind kLsPlan{kLsStamp, kLsOp, 2u, (unsigned)kLsTerms, "ragged loss", "curl_loss_ragged_plan"};

// The reference's window, bit for bit (metric.py:104-118 in torch): the float32 Gaussian divided by its float32 sum, and
// torch's sum of these few values is the correctly rounded one (ssim_window adds them in float32 one by one: at 11 taps another
// float, every weight an ulp off and the window's total 1.5e-7 off -- invisible to three-channel float32 statistics, not to
// float64 ones).  -> gscale: sqrt(total of the reference's 2-D window round(g_i g_j)) / sum(g), which gives the separable
// float64 window that total.
static double ls_window(int ws, float* g) {
  double sum = 0.0;
  for (int x = 0; x < ws; ++x) {
    g[x] = (float)exp(-(double)((x - ws / 2) * (x - ws / 2)) / (2.0 * 1.5 * 1.5));
    sum += (double)g[x];
  }
  const float fsum = (float)sum;
  double s1 = 0.0, s2 = 0.0;
  for (int x = 0; x < ws; ++x) g[x] /= fsum, s1 += (double)g[x];
  for (int i = 0; i < ws; ++i)
    for (int j = 0; j < ws; ++j) s2 += (double)(float)(g[i] * g[j]);
  return sqrt(s2) / s1;
}

extern "C" {

size_t curl_loss_ragged_plan_bytes(int B) {
  if (B < 1 || B > kRaggedMaxImages) return 0;
  return ms_plan_words(B) * sizeof(int);
}

int curl_loss_ragged_plan(int B, const int* H, const int* W, int has_mask, void* host_buf, size_t bytes) {
  g_err[0] = 0;
  if (!H || !W) return fail(CURL_E_NULL, "H / W is NULL");
  if (!host_buf) return fail(CURL_E_NULL, "host_buf is NULL");
  if (B < 1) return fail(CURL_E_SHAPE, "ragged batch: B must be positive");
  if (B > kRaggedMaxImages) return fail(CURL_E_SHAPE, "B exceeds 65535 images per call");
  if ((uintptr_t)host_buf % 8) return fail(CURL_E_WORKSPACE, "ragged batch: the plan buffer must be 8-byte aligned");
  if (bytes < ms_plan_words(B) * sizeof(int))
    return fail(CURL_E_WORKSPACE, "ragged batch: the plan buffer is too small (curl_loss_ragged_plan_bytes)");
  return ms_build(kLsPlan, B, H, W, has_mask != 0, static_cast<int*>(host_buf));
}

size_t curl_loss_ragged_workspace_bytes(const void* host_plan) {
  const int rc = ms_host_plan(kLsPlan, host_plan);
  g_err[0] = 0;
  if (rc || static_cast<const int*>(host_plan)[MH_OP] != (int)kLsOp) return 0;
  return (size_t)get64(static_cast<const int*>(host_plan) + MH_WS_BYTES);
}

int curl_loss_ragged_u8hwc(const uint8_t* pred_arena, size_t pred_bytes, const uint8_t* target_arena, size_t target_bytes,
                           const uint8_t* mask_arena, size_t mask_bytes, double* stats, size_t stats_bytes, void* workspace,
                           size_t workspace_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, int window_size,
                           unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  // curl_msssim_ragged_u8hwc's checks in its order and wording, on this header's plan
  if (!pred_arena || !target_arena) return fail(CURL_E_NULL, "arena pointer is NULL");
  if (!plan_dev) return fail(CURL_E_NULL, "plan_dev is NULL");
  if (int rc = ms_host_plan(kLsPlan, host_plan)) return rc;
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (flags must be 0)");
  const int* p = static_cast<const int*>(host_plan);
  if (p[MH_OP] != (int)kLsOp) return fail(CURL_E_WORKSPACE, "ragged batch: the plan was made for another operator");
  if (mask_arena && !p[MH_HAS_MASK]) return fail(CURL_E_WORKSPACE, "ragged batch: a mask arena with a plan that was made without masks");
  if ((uintptr_t)plan_dev % 8) return fail(CURL_E_WORKSPACE, "ragged batch: plan_dev must be 8-byte aligned");
  const unsigned B = (unsigned)p[MH_B];
  if (plan_bytes < ms_plan_words((int)B) * sizeof(int))
    return fail(CURL_E_WORKSPACE, "ragged batch: plan_dev is too small (curl_loss_ragged_plan_bytes)");
  const uint64_t rgb_bytes = get64(p + MH_RGB_BYTES), ws_bytes = get64(p + MH_WS_BYTES), partial_off = get64(p + MH_PARTIAL_OFF);
  if (pred_bytes < rgb_bytes) return fail(CURL_E_WORKSPACE, "ragged loss: the pred arena is smaller than the plan's");
  if (target_bytes < rgb_bytes) return fail(CURL_E_WORKSPACE, "ragged loss: the target arena is smaller than the plan's");
  if (mask_arena && mask_bytes < get64(p + MH_MASK_BYTES)) return fail(CURL_E_WORKSPACE, "ragged batch: the mask arena is smaller than the plan's");
  if (!stats) return fail(CURL_E_WORKSPACE, "ragged loss: stats is NULL");
  if ((uintptr_t)stats % 8) return fail(CURL_E_WORKSPACE, "ragged loss: stats must be 8-byte aligned");
  if (stats_bytes < (size_t)B * 3 * kMsLevels * sizeof(double)) return fail(CURL_E_WORKSPACE, "ragged loss: stats is too small (120 bytes per image)");
  if (!workspace) return fail(CURL_E_WORKSPACE, "ragged loss: workspace is NULL");
  if ((uintptr_t)workspace % 8) return fail(CURL_E_WORKSPACE, "ragged loss: workspace must be 8-byte aligned");
  if (workspace_bytes < ws_bytes) return fail(CURL_E_WORKSPACE, "ragged loss: workspace is too small (curl_loss_ragged_workspace_bytes)");
  if (!on_grid(4, pred_arena, target_arena, mask_arena)) return fail(CURL_E_SHAPE, "ragged batch: the arenas must be 4-byte aligned");
  if (window_size < 1 || window_size > 2 * SSIM_R + 1 || (window_size & 1) == 0) return fail(CURL_E_KNOTS, "window_size must be odd and <= 11");

  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  double* partial = reinterpret_cast<double*>(ws + partial_off);
  double* terms = reinterpret_cast<double*>(ws + get64(p + LH_TERMS_OFF));
  const int* plan = static_cast<const int*>(plan_dev);
  const unsigned long long hash = get64(p + MH_HASH), mb = mask_arena ? mask_bytes : 0;
  SsimArgs win{};  // the window and the level: everything else travels beside it
  win.levels = kMsLevels, win.radius = window_size / 2;
  const double gscale = ls_window(window_size, win.g);
  unsigned pairs = 0;
  for (int l = 0; l < kMsLevels; ++l) {
    const unsigned grid = (unsigned)p[MH_GRID0 + l];
    double* first = partial + 2 * (size_t)(unsigned)p[MH_PAIR0 + l];
    win.level = l;
    if (l == 0)
      hipLaunchKernelGGL(loss_ragged_bytes_kernel, dim3(grid), dim3(256), 0, s, win, plan, pred_arena, target_arena, mask_arena, ws, first,
                         terms, (unsigned long long)pred_bytes, (unsigned long long)target_bytes, mb, (unsigned long long)partial_off, hash,
                         kLsStamp, B, gscale);
    else
      hipLaunchKernelGGL(loss_ragged_level_kernel, dim3(grid), dim3(256), 0, s, win, plan, ws, first, (unsigned long long)partial_off, hash,
                         kLsStamp, B, gscale);
    pairs += grid;
  }
  hipLaunchKernelGGL(loss_ragged_finish_kernel, dim3(B), dim3(256), 0, s, plan, (const double*)partial, (const double*)terms, stats, hash,
                     kLsStamp, B, pairs, (unsigned)p[MH_GRID0]);
  return hip_done("curl_loss_ragged_u8hwc");
}

}  // extern "C"
