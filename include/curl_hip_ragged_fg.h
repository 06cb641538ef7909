/* curl_hip_ragged_fg.h -- C ABI of libcurlhip.so, continued: the file-to-file byte paths for a batch of images of different
 * sizes, foreground-aware.
 *
 * Conventions, error codes and the stream type are curl_hip.h's; the ragged batch, its three arenas and the plan are
 * curl_hip_ragged.h's, unchanged.  This header exists beside that one because its entries refuse every flag bit and its
 * declarations are pinned (tests/test_ragged_abi.py holds _lib.SIGNATURES_RAGGED to exactly that header's).
 *
 * replaces: curl_trispace_fwd_ragged_u8hwc / curl_layer_fwd_ragged_u8hwc with a mask arena, for masks that are segmentation
 *           masks (infer.py:46, "turn background white like in app"): where a mask byte is 0 the result is white whatever the
 *           pixel, so a wavefront whose mask bytes are all 0 stores white and never reads its pixels, and a workgroup of such
 *           wavefronts does not stage its coefficient table or fold its row either.
 *
 * Both entries:
 *   plan        curl_ragged_plan's, built with has_mask = 1 (a plan built without masks: CURL_E_WORKSPACE).  The layout, the
 *               stamp and the hash are curl_hip_ragged.h's: ONE uploaded plan serves the sibling entry and this one.
 *   mask_arena  required (NULL: CURL_E_MASK): image i's H_i*W_i 'L' mask bytes at mask_off[i].  m = byte / 255; the result is
 *               out * m + (1 - m), two roundings, as in the sibling entries; a byte of 0 gives (255, 255, 255).
 *   img_arena   as the sibling's.  The pixel bytes under a mask byte of 0 need not be read: they may hold anything.
 *   flags       must be 0 (CURL_E_FLAGS).
 * Every other argument and every other check is the sibling's (curl_hip_ragged.h), all of them before the first HIP call.
 * For finite coefficients / knots every byte of the out arena's images equals what the sibling entry writes with the same
 * mask arena; padding bytes of the out arena are never written, the image and mask arenas never at all.  One launch per
 * class of images (the layer: and the curve collapse), no scratch, no atomics: the same bytes on a repeated call, for an
 * image alone or in any company and order.  A stale or foreign device plan gives no output (the kernels' stamp, hash and
 * extent checks are the sibling's; the mask arena's extents are checked for every workgroup).
 */
#ifndef CURL_HIP_RAGGED_FG_H
#define CURL_HIP_RAGGED_FG_H

#include <stddef.h>
#include <stdint.h>

#include "curl_hip_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TriSpaceRegNet's per-pixel part on every image of the batch.  coeffs [B,3,3,n] float32 and num_coeffs exactly as
 * curl_trispace_fwd_ragged_u8hwc takes them. */
int curl_trispace_fwd_ragged_fg_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* coeffs, const uint8_t* mask_arena,
                                      size_t mask_bytes, uint8_t* out_arena, size_t out_bytes, const void* host_plan,
                                      const void* plan_dev, size_t plan_bytes, int num_coeffs, unsigned flags, curl_stream_t stream);

/* CURLLayer.forward without a layer mask on every image of the batch; the plan is the one of operator 0.  The knot arguments,
 * reg (nullable, [B]) and the workspace exactly as curl_layer_fwd_ragged_u8hwc takes them; reg and the workspace rows hold the
 * same bits as after that entry. */
int curl_layer_fwd_ragged_fg_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* rawL, const float* rawR,
                                   const float* rawH, const uint8_t* mask_arena, size_t mask_bytes, uint8_t* out_arena,
                                   size_t out_bytes, float* reg, void* workspace, size_t workspace_bytes, const void* host_plan,
                                   const void* plan_dev, size_t plan_bytes, int Kl, int Kr, int Kh, unsigned flags,
                                   curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_RAGGED_FG_H */
