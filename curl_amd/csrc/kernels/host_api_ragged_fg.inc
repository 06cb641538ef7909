// host_api_ragged_fg.inc -- part of curl_kernels.hip (one translation unit; included after host_api_ragged.inc, whose two
// forward entries these are with fg set: the mask arena required, stream_ragged_fg_kernel on the same plan).  The entry points
// of include/curl_hip_ragged_fg.h.
// ------------------------------------------------------------------------------------------------
// host side: the foreground-aware byte edge for a batch of images of different sizes
// ------------------------------------------------------------------------------------------------
extern "C" {

int curl_trispace_fwd_ragged_fg_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* coeffs, const uint8_t* mask_arena,
                                      size_t mask_bytes, uint8_t* out_arena, size_t out_bytes, const void* host_plan,
                                      const void* plan_dev, size_t plan_bytes, int num_coeffs, unsigned flags, curl_stream_t stream) {
  return trispace_fwd_ragged(img_arena, img_bytes, coeffs, mask_arena, mask_bytes, out_arena, out_bytes, host_plan, plan_dev, plan_bytes,
                             num_coeffs, flags, stream, true);
}

int curl_layer_fwd_ragged_fg_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* rawL, const float* rawR,
                                   const float* rawH, const uint8_t* mask_arena, size_t mask_bytes, uint8_t* out_arena,
                                   size_t out_bytes, float* reg, void* workspace, size_t workspace_bytes, const void* host_plan,
                                   const void* plan_dev, size_t plan_bytes, int Kl, int Kr, int Kh, unsigned flags,
                                   curl_stream_t stream) {
  return layer_fwd_ragged(img_arena, img_bytes, rawL, rawR, rawH, mask_arena, mask_bytes, out_arena, out_bytes, reg, workspace,
                          workspace_bytes, host_plan, plan_dev, plan_bytes, Kl, Kr, Kh, flags, stream, true);
}

}  // extern "C"
