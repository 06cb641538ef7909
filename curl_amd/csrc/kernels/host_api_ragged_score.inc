// host_api_ragged_score.inc -- part of curl_kernels.hip (one translation unit; included after host_api_ragged.inc, whose plan
// checks and error text it uses).  The entry points of include/curl_hip_ragged_score.h.
// ------------------------------------------------------------------------------------------------
// host side: the exact score of a batch of byte images of different sizes
// ------------------------------------------------------------------------------------------------
// the pairs pass 1 writes: one per workgroup of either launch of a plan of operator 0 (checked by the caller)
static size_t score_pairs(const int* p) { return (size_t)(unsigned)p[RH_GRID_DWORD] + (size_t)(unsigned)p[RH_GRID_BYTE]; }

extern "C" {

size_t curl_ragged_score_workspace_bytes(const void* host_plan) {
  if (ragged_host_plan(host_plan) || static_cast<const int*>(host_plan)[RH_OP] != 0) return 0;
  return score_pairs(static_cast<const int*>(host_plan)) * 2 * sizeof(ScorePartial);
}

int curl_sse_ragged_u8hwc(const uint8_t* a_arena, size_t a_bytes, const uint8_t* b_arena, size_t b_bytes,
                          const uint8_t* mask_arena, size_t mask_bytes, uint64_t* sums, size_t sums_bytes, void* workspace,
                          size_t workspace_bytes, const void* host_plan, const void* plan_dev, size_t plan_bytes, unsigned flags,
                          curl_stream_t stream) {
  g_err[0] = 0;
  // the forward entries' order: the plan, then the arenas -- a and b both held to the plan's OUT arena (an image arena of RGBA
  // images is larger), under their own names
  if (!a_arena || !b_arena) return fail(CURL_E_NULL, "arena pointer is NULL");
  if (int rc = check_ragged_plan(host_plan, plan_dev, plan_bytes, 0, flags, mask_arena != nullptr)) return rc;
  const int* p = static_cast<const int*>(host_plan);
  const uint64_t rgb_bytes = get64(p + RH_OUT_BYTES);
  if (mask_arena && mask_bytes < get64(p + RH_MASK_BYTES)) return fail(CURL_E_WORKSPACE, "ragged batch: the mask arena is smaller than the plan's");
  if (!on_grid(4, a_arena, mask_arena, b_arena)) return fail(CURL_E_SHAPE, "ragged batch: the arenas must be 4-byte aligned");
  if (a_bytes < rgb_bytes) return fail(CURL_E_WORKSPACE, "ragged score: the a arena is smaller than the plan's out arena");
  if (b_bytes < rgb_bytes) return fail(CURL_E_WORKSPACE, "ragged score: the b arena is smaller than the plan's out arena");
  const unsigned B = (unsigned)p[RH_B];
  if (!sums) return fail(CURL_E_WORKSPACE, "ragged score: sums is NULL");
  if ((uintptr_t)sums % 8) return fail(CURL_E_WORKSPACE, "ragged score: sums must be 8-byte aligned");
  if (sums_bytes < (size_t)B * 2 * sizeof(uint64_t)) return fail(CURL_E_WORKSPACE, "ragged score: sums is too small (16 bytes per image)");
  if (!workspace) return fail(CURL_E_WORKSPACE, "ragged score: workspace is NULL");
  if ((uintptr_t)workspace % 8) return fail(CURL_E_WORKSPACE, "ragged score: workspace must be 8-byte aligned");
  if (workspace_bytes < score_pairs(p) * 2 * sizeof(ScorePartial))
    return fail(CURL_E_WORKSPACE, "ragged score: workspace is too small (curl_ragged_score_workspace_bytes)");

  hipStream_t s = (hipStream_t)stream;
  ScorePartial* partial = static_cast<ScorePartial*>(workspace);
  const int* plan = static_cast<const int*>(plan_dev);
  const unsigned long long hash = get64(p + RH_HASH);
  const unsigned n_dword = (unsigned)p[RH_N_DWORD], grid_dword = (unsigned)p[RH_GRID_DWORD], grid_byte = (unsigned)p[RH_GRID_BYTE];
  const unsigned long long mb = mask_arena ? mask_bytes : 0;
  if (n_dword > 0)
    hipLaunchKernelGGL((sse_ragged_partial_kernel<4>), dim3(grid_dword), dim3(256), 0, s, plan, a_arena, b_arena, mask_arena, partial,
                       (unsigned long long)a_bytes, (unsigned long long)b_bytes, mb, hash, kRaggedStamp, kRaggedHeaderWords, n_dword);
  if (p[RH_N_BYTE] > 0)
    hipLaunchKernelGGL((sse_ragged_partial_kernel<1>), dim3(grid_byte), dim3(256), 0, s, plan, a_arena, b_arena, mask_arena,
                       partial + 2 * (size_t)grid_dword, (unsigned long long)a_bytes, (unsigned long long)b_bytes, mb, hash, kRaggedStamp,
                       kRaggedHeaderWords + n_dword * kRaggedDescWords, (unsigned)p[RH_N_BYTE]);
  hipLaunchKernelGGL(sse_ragged_final_kernel, dim3(B), dim3(256), 0, s, plan, partial, reinterpret_cast<unsigned long long*>(sums), hash,
                     kRaggedStamp, B, n_dword, grid_dword, grid_byte);
  return hip_done("curl_sse_ragged_u8hwc");
}

}  // extern "C"
