// host_api_ragged_loss.inc -- part of curl_kernels.hip (one translation unit; included after host_api_ragged_msssim.inc, whose
// plan builder and plan check it uses with a kind of its own).  The entry points of include/curl_hip_ragged_loss.h.
// ------------------------------------------------------------------------------------------------
// host side: the CURLLoss statistics of a batch of byte images of different sizes
// ------------------------------------------------------------------------------------------------
static const MsPlanKind kLsPlan{kLsStamp, kLsOp, 2u, (unsigned)kLsTerms, 3u, "ragged loss", "pred", "target", "curl_loss_ragged_plan",
                                "curl_loss_ragged_plan_bytes", "curl_loss_ragged_workspace_bytes"};

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

size_t curl_loss_ragged_plan_bytes(int B) { return ms_plan_bytes(B); }

int curl_loss_ragged_plan(int B, const int* H, const int* W, int has_mask, void* host_buf, size_t bytes) {
  return ms_plan(kLsPlan, B, H, W, has_mask, host_buf, bytes);
}

size_t curl_loss_ragged_workspace_bytes(const void* host_plan) { return ms_workspace_bytes(kLsPlan, host_plan); }

int curl_loss_ragged_u8hwc(const uint8_t* pred_arena, size_t pred_bytes, const uint8_t* target_arena, size_t target_bytes,
                           const uint8_t* mask_arena, size_t mask_bytes, double* stats, size_t stats_bytes, void* workspace,
                           size_t workspace_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, int window_size,
                           unsigned flags, curl_stream_t stream) {
  if (int rc = ms_check(kLsPlan, pred_arena, pred_bytes, target_arena, target_bytes, mask_arena, mask_bytes, stats, stats_bytes, workspace,
                        workspace_bytes, host_plan, plan_dev, plan_bytes, window_size, flags))
    return rc;
  const MsCall c(host_plan, plan_dev, workspace, mask_arena, mask_bytes, stream);
  double* terms = reinterpret_cast<double*>(c.ws + get64(c.p + LH_TERMS_OFF));
  SsimArgs win{};
  const double gscale = ls_window(window_size, win.g);
  return ms_launch(
      c, win, window_size, "curl_loss_ragged_u8hwc",
      [&](unsigned grid, double* first) {
        hipLaunchKernelGGL(loss_ragged_bytes_kernel, dim3(grid), dim3(256), 0, c.s, win, c.plan, pred_arena, target_arena, mask_arena, c.ws,
                           first, terms, (unsigned long long)pred_bytes, (unsigned long long)target_bytes, c.mask_bytes, c.partial_off, c.hash,
                           kLsStamp, c.B, gscale);
      },
      [&](unsigned grid, double* first) {
        hipLaunchKernelGGL(loss_ragged_level_kernel, dim3(grid), dim3(256), 0, c.s, win, c.plan, c.ws, first, c.partial_off, c.hash, kLsStamp,
                           c.B, gscale);
      },
      [&](unsigned pairs) {
        hipLaunchKernelGGL(loss_ragged_finish_kernel, dim3(c.B), dim3(256), 0, c.s, c.plan, (const double*)c.partial, (const double*)terms,
                           stats, c.hash, kLsStamp, c.B, pairs, (unsigned)c.p[MH_GRID0]);
      });
}

}  // extern "C"

