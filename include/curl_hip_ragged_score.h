/* curl_hip_ragged_score.h -- C ABI of libcurlhip.so, continued: the exact score of a batch of byte images of different sizes
 * against their targets, every image of the batch in one pass.
 *
 * Conventions, error codes and the stream type are curl_hip.h's; the ragged batch, its arenas and the plan are
 * curl_hip_ragged.h's, unchanged.  This header exists beside that one for the reason the other side headers do: the recorded
 * launch plan (tests/data/launch_plan.txt) enumerates curl_hip.h's declarations, and the ABI tests hold every existing
 * _lib.SIGNATURES* table to exactly its header's.
 *
 * replaces: per image, curl_u8hwc_to_f32chw of the result and of the target and curl_psnr_f32 with the float mask
 *           (evaluate.py:102, metric.py:35-68): 24 bytes of float image per pixel and a float32 sum of values that are
 *           integers to begin with.  For 8-bit images the masked squared error IS an integer; here it is summed exactly from
 *           the 7 bytes per pixel (3 + 3 + 1) the batch already has on the device.
 *
 * Arenas.  a_arena and b_arena are both laid out as the plan's OUT arena: image i's H_i*W_i*3 interleaved RGB bytes at the
 * descriptor's out_off -- what the *_ragged_u8hwc entries return, and what an image arena of 3-channel images of those shapes
 * is.  The mask arena is the plan's: image i's H_i*W_i bytes at mask_off.  None of the three is written.
 *
 * Plan.  curl_ragged_plan's for operator 0 (the curve layer's flat tiles: 256 lanes, one group per lane, 1 024 pixels per
 * workgroup in the dword class and 256 in the byte class), with or without masks.  The plan's channels words only place
 * img_off; they are not read here.  ONE uploaded plan serves curl_layer_fwd_ragged_u8hwc and this entry.
 *
 * Two passes, no atomics, no memset, integer arithmetic only: pass 1 is one launch per non-empty class with the plan's
 * grids, every workgroup writing its (sum, count) pair of uint32 into the workspace; pass 2 is one launch of B workgroups
 * that sum their image's pairs in uint64.  The results are the same bits on every call, for an image alone or in any company
 * and order.  Safety of the device copy is curl_hip_ragged.h's: a stale or foreign device plan writes nothing at all (sums
 * and the workspace keep what they held), never an access outside the arenas.
 */
#ifndef CURL_HIP_RAGGED_SCORE_H
#define CURL_HIP_RAGGED_SCORE_H

#include <stddef.h>
#include <stdint.h>

#include "curl_hip_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 8 * (grid of the dword launch + grid of the byte launch) of the host plan; 0 for a buffer that is no plan
 * or a plan of another operator.  No HIP call. */
size_t curl_ragged_score_workspace_bytes(const void* host_plan);

/* For every image i of the batch: sums[2*i] = sum over the pixels whose mask byte is != 0 (all pixels without
 * a mask arena) and the 3 channels of (a - b)^2, sums[2*i+1] = the number of those pixels.  Exact, uint64.
 *
 * sums: [B,2] uint64 in image INDEX order, 8-byte aligned, sums_bytes >= 16*B.  workspace: 8-byte aligned, workspace_bytes
 * >= curl_ragged_score_workspace_bytes(host_plan); its contents afterwards are the workgroups' partial pairs.  mask_arena
 * nullable (mask_bytes is then not read).  host_plan / plan_dev / plan_bytes as curl_layer_fwd_ragged_u8hwc takes them.
 * Checked before the first HIP call: NULLs (CURL_E_NULL), flags != 0 (CURL_E_FLAGS), a host plan without the stamp or
 * misaligned, a plan of another operator, a mask arena with a plan made without masks, a plan_dev too small or misaligned,
 * an arena smaller than the plan's, sums or workspace NULL, too small or off the 8-byte grid (all CURL_E_WORKSPACE), an
 * arena base off the 4-byte grid (CURL_E_SHAPE). */
int curl_sse_ragged_u8hwc(const uint8_t* a_arena, size_t a_bytes, const uint8_t* b_arena, size_t b_bytes,
                          const uint8_t* mask_arena, size_t mask_bytes, uint64_t* sums, size_t sums_bytes,
                          void* workspace, size_t workspace_bytes, const void* host_plan, const void* plan_dev,
                          size_t plan_bytes, unsigned flags, curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_RAGGED_SCORE_H */
