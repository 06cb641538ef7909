// host_api_ragged_fg.inc -- part of curl_kernels.hip (one translation unit; included after host_api_ragged.inc, whose plan,
// argument checks and error text it uses).  The entry points of include/curl_hip_ragged_fg.h.
// ------------------------------------------------------------------------------------------------
// host side: the foreground-aware byte edge for a batch of images of different sizes
// ------------------------------------------------------------------------------------------------
// check_ragged with the mask arena required (a plan made without masks is refused there: the arena is not NULL); no HIP call
static int check_ragged_fg(RaggedArgs& r, const uint8_t* img, size_t img_bytes, const uint8_t* mask, size_t mask_bytes, uint8_t* out,
                           size_t out_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, int op_count, unsigned flags) {
  if (!img || !out) return fail(CURL_E_NULL, "arena pointer is NULL");
  if (!mask) return fail(CURL_E_MASK, "mask_arena is NULL (the foreground entries need the masks)");
  return check_ragged(r, img, img_bytes, mask, mask_bytes, out, out_bytes, host_plan, plan_dev, plan_bytes, op_count, flags);
}

// launch_stream_ragged's launches for stream_ragged_fg_kernel: the plan's grids and block sizes, one launch per non-empty
// class (the curve collapse first); everything is checked by now
template <class Op>
static int launch_stream_ragged_fg(RaggedArgs r, const void* host_plan, const float* coef, unsigned coef_stride, hipStream_t s,
                                   const char* name, const PrepArgs* prep = nullptr) {
  const int* p = static_cast<const int*>(host_plan);
  if (prep)
    if (int rc = launch_prep(*prep, p[RH_B], s)) return rc;
  StreamArgs a{};
  a.coef = coef;
  a.coef_stride = coef_stride;
  if (p[RH_N_DWORD] > 0) {
    r.table = kRaggedHeaderWords, r.count = (unsigned)p[RH_N_DWORD];
    hipLaunchKernelGGL((stream_ragged_fg_kernel<Op, 4, true>), dim3((unsigned)p[RH_GRID_DWORD]), dim3((unsigned)p[RH_THREADS_DWORD]), 0, s, a, r.plan, r.img, r.mask,
                       r.out, r.img_bytes, r.mask_bytes, r.out_bytes, r.hash, r.stamp, r.table, r.count);
  }
  if (p[RH_N_BYTE] > 0) {
    r.table = kRaggedHeaderWords + (unsigned)p[RH_N_DWORD] * kRaggedDescWords, r.count = (unsigned)p[RH_N_BYTE];
    hipLaunchKernelGGL((stream_ragged_fg_kernel<Op, 1, false>), dim3((unsigned)p[RH_GRID_BYTE]), dim3((unsigned)p[RH_THREADS_BYTE]), 0, s, a, r.plan, r.img, r.mask,
                       r.out, r.img_bytes, r.mask_bytes, r.out_bytes, r.hash, r.stamp, r.table, r.count);
  }
  return hip_done(name);
}

extern "C" {

int curl_trispace_fwd_ragged_fg_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* coeffs, const uint8_t* mask_arena,
                                      size_t mask_bytes, uint8_t* out_arena, size_t out_bytes, const void* host_plan,
                                      const void* plan_dev, size_t plan_bytes, int num_coeffs, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (!coeffs) return fail(CURL_E_NULL, "coeffs is NULL");
  if (!img_arena || !out_arena) return fail(CURL_E_NULL, "arena pointer is NULL");
  int order;
  if (int rc = unpack_num_coeffs(num_coeffs, num_coeffs, order)) return rc;
  RaggedArgs r{};
  if (int rc = check_ragged_fg(r, img_arena, img_bytes, mask_arena, mask_bytes, out_arena, out_bytes, host_plan, plan_dev, plan_bytes,
                               num_coeffs, flags))
    return rc;
  if (int rc = check_coeffs_aligned(coeffs, num_coeffs)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_order(num_coeffs, [&](auto V, auto D) {
    typedef TriSpaceOp<V, D> T;
    return launch_stream_ragged_fg<typename T::Op>(r, host_plan, coeffs, T::kCoefStride, s,
                                                   T::kRows ? "trispace_rows_ragged_fg_u8hwc" : "trispace_ragged_fg_u8hwc");
  });
}

int curl_layer_fwd_ragged_fg_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* rawL, const float* rawR,
                                   const float* rawH, const uint8_t* mask_arena, size_t mask_bytes, uint8_t* out_arena,
                                   size_t out_bytes, float* reg, void* workspace, size_t workspace_bytes, const void* host_plan,
                                   const void* plan_dev, size_t plan_bytes, int Kl, int Kr, int Kh, unsigned flags,
                                   curl_stream_t stream) {
  g_err[0] = 0;
  RaggedArgs r{};
  if (int rc = check_ragged_fg(r, img_arena, img_bytes, mask_arena, mask_bytes, out_arena, out_bytes, host_plan, plan_dev, plan_bytes, 0,
                               flags))
    return rc;
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, true, workspace, workspace_bytes, static_cast<const int*>(host_plan)[RH_B], reg))
    return rc;
  return launch_stream_ragged_fg<OpLayer>(r, host_plan, k.ws, k.stride, (hipStream_t)stream, "curl_layer_ragged_fg_u8hwc", &k.prep);
}

}  // extern "C"
