// host_api_fg.inc -- part of curl_kernels.hip (one translation unit; included after host_api.inc, whose argument checks,
// launch geometry and error text it uses).  The entry points of include/curl_hip_fg.h.
// ------------------------------------------------------------------------------------------------
// host side: the foreground-aware byte edge
// ------------------------------------------------------------------------------------------------
// launch_stream_u8's launch for stream_fg_kernel: the same dword-or-byte verdict on the 4-byte grid (image, output and mask;
// four RGBA pixels are four dwords), the same geometry, one tile shape per op, no tuning fields
template <class Op>
static int launch_stream_fg(const uint8_t* in, int channels, uint8_t* out, const uint8_t* fg_mask, const float* coef,
                            unsigned coef_stride, int B, int H, int W, hipStream_t s, const char* name,
                            const PrepArgs* prep = nullptr) {
  const size_t HW = (size_t)H * W;
  Geometry g;
  if (int rc = make_geometry(g, Tuning(), planes_vec4(HW, nullptr, CURL_MASK_NONE, 4, in, out, fg_mask) ? 4 : 1, 1, 0, HW, B)) return rc;
  if constexpr (Op::kRowTiles)
    if (int rc = make_row_geometry(g, B, H, W)) return rc;
  if (prep)
    if (int rc = launch_prep(*prep, B, s)) return rc;
  StreamArgs a{};
  a.in = reinterpret_cast<const float*>(in);
  a.out = reinterpret_cast<float*>(out);
  a.white = fg_mask;
  a.coef = coef;
  a.coef_stride = coef_stride;
  a.n = g.n;
  a.blocks_per_image = g.blocks_per_image;
  a.n_blocks = g.n_blocks;
  a.W = (unsigned)W;
  a.H = (unsigned)H;
  a.units = g.units, a.segs = g.segs;
  a.plane = a.n;
  const dim3 grid(g.blocks_per_image, g.n_images), block(g.threads);
  if (g.vec == 4) hipLaunchKernelGGL((stream_fg_kernel<Op, 4, true>), grid, block, 0, s, a, (unsigned)channels);
  else hipLaunchKernelGGL((stream_fg_kernel<Op, 1, false>), grid, block, 0, s, a, (unsigned)channels);
  return hip_done(name);
}

static int check_fg(const uint8_t* fg_mask, int channels, unsigned flags) {
  if (!fg_mask) return fail(CURL_E_MASK, "fg_mask is NULL (the foreground entries need the mask)");
  if (channels != 3 && channels != 4) return fail(CURL_E_SHAPE, "channels must be 3 (RGB) or 4 (RGBA)");
  if (flags) return fail(CURL_E_FLAGS, "unsupported flag bit for this entry point (flags must be 0)");
  return 0;
}

extern "C" {

int curl_trispace_fwd_fg_u8hwc(const uint8_t* img, int channels, const float* coeffs, const uint8_t* fg_mask, uint8_t* out,
                               int B, int H, int W, int num_coeffs, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (!coeffs) return fail(CURL_E_NULL, "coeffs is NULL");
  if (int rc = check_fg(fg_mask, channels, flags)) return rc;
  int order;
  if (int rc = unpack_num_coeffs(num_coeffs, num_coeffs, order)) return rc;
  if (int rc = check_coeffs_aligned(coeffs, num_coeffs)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_order(num_coeffs, [&](auto V, auto D) {
    typedef TriSpaceOp<V, D> T;
    return launch_stream_fg<typename T::Op>(img, channels, out, fg_mask, coeffs, T::kCoefStride, B, H, W, s,
                                            T::kRows ? "trispace_rows_fg_u8hwc" : "trispace_fg_u8hwc");
  });
}

int curl_layer_fwd_fg_u8hwc(const uint8_t* img, int channels, const float* rawL, const float* rawR, const float* rawH,
                            const uint8_t* fg_mask, uint8_t* out, float* reg, void* workspace, size_t workspace_bytes, int B,
                            int H, int W, int Kl, int Kr, int Kh, unsigned flags, curl_stream_t stream) {
  g_err[0] = 0;
  if (int rc = check_img(img, out, B, H, W)) return rc;
  if (int rc = check_fg(fg_mask, channels, flags)) return rc;
  KnotSetup k;
  if (int rc = layer_knots(k, rawL, rawR, rawH, Kl, Kr, Kh, true, workspace, workspace_bytes, B, reg)) return rc;
  return launch_stream_fg<OpLayer>(img, channels, out, fg_mask, k.ws, k.stride, B, H, W, (hipStream_t)stream,
                                   "curl_layer_fg_u8hwc", &k.prep);
}

}  // extern "C"
