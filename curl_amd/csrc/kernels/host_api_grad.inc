// host_api_grad.inc -- part of curl_kernels.hip (one translation unit; included after host_api.inc, whose argument checks,
// float4 verdict and error text it uses).  The entry points of include/curl_hip_grad.h.
// ------------------------------------------------------------------------------------------------
// host side: the fused polynomial model's image gradient
// ------------------------------------------------------------------------------------------------
template <int V>
static void launch_trispace_img_grad(const float* img, const float* coeffs, const float* gout, float* gimg, int B, int H, int W,
                                     int residual_only, hipStream_t s) {
  const size_t HW = (size_t)H * W;
  const bool aligned = planes_vec4(HW, nullptr, CURL_MASK_NONE, 16, img, gout, gimg);
  const unsigned n = (unsigned)(HW / (aligned ? 4 : 1)), per = 256u * kTriImgGradSteps;  // groups per plane, per workgroup
  const dim3 grid((n + per - 1u) / per, (unsigned)B);  // <= 2^20 x 65535 (check_img)
  dispatch_vec_mask<kMasksNone>(aligned, CURL_MASK_NONE, [&](auto VEC, auto) {
    hipLaunchKernelGGL((trispace_img_grad_kernel<V, VEC>), grid, dim3(256), 0, s, img, coeffs, gout, gimg, n, (unsigned)W, (float)W,
                       (float)H, residual_only);
  });
}

extern "C" {

int curl_trispace_bwd_img_f32(const float* img, const float* coeffs, const float* grad_out, float* grad_img, int B, int H, int W,
                              int num_coeffs, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, grad_out, B, H, W)) return rc;
  if (!coeffs || !grad_img) return fail(CURL_E_NULL, "coeffs / grad_img is NULL");
  if (int rc = check_num_coeffs(num_coeffs, "num_coeffs must be 126 or 35")) return rc;
  if (flags & ~(unsigned)CURL_F_RESIDUAL_ONLY) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (CURL_F_RESIDUAL_ONLY or 0)");
  if (int rc = check_coeffs_aligned(coeffs, num_coeffs)) return rc;
  if ((const void*)grad_img == (const void*)img || (const void*)grad_img == (const void*)coeffs)
    return fail(CURL_E_SHAPE, "grad_img must not alias img or coeffs");
  const int ro = (flags & CURL_F_RESIDUAL_ONLY) ? 1 : 0;
  if (num_coeffs == PolyEval<5>::kCoeffs) launch_trispace_img_grad<5>(img, coeffs, grad_out, grad_img, B, H, W, ro, (hipStream_t)stream);
  else launch_trispace_img_grad<3>(img, coeffs, grad_out, grad_img, B, H, W, ro, (hipStream_t)stream);
  return hip_done("trispace_img_grad_kernel");
}

}  // extern "C"
