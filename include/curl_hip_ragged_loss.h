/* curl_hip_ragged_loss.h -- C ABI of libcurlhip.so, continued: the statistics of the reference's CURLLoss (model.py:78-116) of
 * a batch of byte images of different sizes against their targets, the whole batch in six launches.
 *
 * Conventions, error codes and the stream type are curl_hip.h's; the arenas are curl_hip_ragged.h's; the plan is
 * curl_hip_ragged_msssim.h's twin.  This header exists beside the others for the reason they do: the ABI tests hold every
 * existing _lib.SIGNATURES* table to exactly its header's declarations.
 *
 * replaces: per image, curl_u8hwc_to_f32chw of the result and of the target, curl_loss_terms_f32 with its two full-resolution
 *           float L planes and curl_msssim_fwd_f32 on them (model.py:89-116 on a [1,3,H,W] batch): about fifteen launches and
 *           40 bytes of float image per pixel, for a folder one image at a time.  Here level 0 is computed from the 7 bytes
 *           per pixel (3 + 3 + 1) the batch already has on the device; no full-resolution float plane is ever written.
 *
 * What is scored is the BYTES: the prediction is byte / 255 of the pixels written to the output file, not a network's unrounded
 * float output.  Every image is scored on its own, as CURLLoss()(pred[None], target[None], mask[None]) scores it.
 *
 * Arenas.  pred_arena and target_arena: image i's H_i*W_i*3 interleaved RGB bytes at rgb_off[i]; mask_arena (optional): image
 * i's H_i*W_i bytes at mask_off[i].  Offsets follow curl_hip_ragged.h's rule, so they equal the out_off / mask_off of a
 * curl_ragged_plan for operator 0 and the same shape list.  None of the three is written.  A pixel's values are
 * float32(byte) / 255 (the correctly rounded quotient, to_tensor's) where its mask byte is not 0 -- everywhere without a mask
 * arena -- and 0 where the mask byte is 0 (model.py:90's `* mask` with data.py:190's `mask > 0`).
 *
 * The PLAN is built on the host into the caller's memory, uploaded by the caller, and handed to the entry as both copies.
 * Its layout is curl_hip_ragged_msssim.h's word for word, with these differences:
 *   header  [0] stamp CURL_LOSS_RAGGED_STAMP   [2] operator CURL_LOSS_RAGGED_OP   [18] the hash runs over this stamp
 *           [16] (i64) workspace bytes: planes, pairs and term partials
 *           [28] (i64) byte offset in the workspace of the level-0 workgroups' term partials (behind the pairs)
 *   level   [+6] (i64) byte offset in the workspace of the level's TWO float planes (l >= 1): the prediction's clamped L
 *           [h][w] float32, then the target's (8*h*w bytes, against 24*h*w there)
 * The workspace holds the float planes of levels 1..4 of every image, then one pair of float64 (sum of the SSIM map, sum of the
 * contrast-structure map over the tile) per workgroup of the five level launches, then five float64 per workgroup of the
 * level-0 launch (the tile's four term sums and its count).
 *
 * Limits (CURL_E_SHAPE from curl_loss_ragged_plan): 1 <= B <= 65535; H_i*W_i <= 2^30; H_i, W_i >= 32 (the message names the
 * first offending image); every launch's grid <= 2^31 - 1 workgroups.
 *
 * Six launches whatever B is -- level 0 from the bytes, levels 1..4 on the workspace's planes, one finish --, no atomics, no
 * memset, every sum in a fixed order: the same bits on every call, for an image alone or in any company and order.  Safety
 * of the device copy is curl_hip_ragged_msssim.h's: every workgroup first compares the device plan's stamp and hash with the
 * host plan's and returns untouched when they differ (stats and the workspace keep what they held); it checks its
 * descriptor's extents against all three arenas and the workspace before it forms an address, and writes zeros if one fails.
 */
#ifndef CURL_HIP_RAGGED_LOSS_H
#define CURL_HIP_RAGGED_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "curl_hip_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CURL_LOSS_RAGGED_STAMP 0x4C535231 /* "1RSL" */
#define CURL_LOSS_RAGGED_OP 6
#define CURL_LOSS_RAGGED_HEADER_WORDS 32
#define CURL_LOSS_RAGGED_DESC_WORDS 64
#define CURL_LOSS_RAGGED_LEVEL_WORD 16 /* a descriptor's first level word */
#define CURL_LOSS_RAGGED_LEVEL_WORDS 8
#define CURL_LOSS_RAGGED_TERMS_WORD 28 /* header: (i64) byte offset of the term partials */
#define CURL_LOSS_RAGGED_TERMS 5       /* float64 per level-0 workgroup: four term sums and the count */

/* Bytes of the plan of B images; 0 for a B outside 1 .. 65535.  No HIP call. */
size_t curl_loss_ragged_plan_bytes(int B);

/* Fills host_buf (HOST memory, 8-byte aligned, `bytes` >= curl_loss_ragged_plan_bytes(B)) with the plan of the B images
 * H[i] x W[i].  has_mask: the batch has a mask arena.  No HIP call.  CURL_E_NULL, CURL_E_SHAPE (the limits above),
 * CURL_E_WORKSPACE (host_buf too small / misaligned). */
int curl_loss_ragged_plan(int B, const int* H, const int* W, int has_mask, void* host_buf, size_t bytes);

/* The workspace bytes a host plan asks for (its word [16]); 0 for a buffer that is no such plan.  No HIP call. */
size_t curl_loss_ragged_workspace_bytes(const void* host_plan);

/* stats[i][0][0..4] = over image i's pixels whose mask byte is not 0 (all pixels without a mask arena): the sum over the three
 * channels of |p - t|, the sum of the cosine similarity, the sum of |Lab_p - Lab_t| (Lab clamped to [0, 1]), the sum of
 * |cone_p - cone_t| (the HSV cone of model.py:65-76), and N, the number of those pixels, an exact integer -- raw sums, not yet
 * divided.  stats[i][1][l] / stats[i][2][l] = the mean over level l's h*w values of the SSIM map / the contrast-structure map
 * of the ONE-channel clamped-L planes (model.py:103-105's MSSSIMMetric(num_channel=1)).  stats: [B][3][5] float64 in image
 * INDEX order, 8-byte aligned, stats_bytes >= 120*B.  workspace: 8-byte aligned, workspace_bytes >=
 * curl_loss_ragged_workspace_bytes(host_plan).  mask_arena nullable (mask_bytes is then not read).  window_size odd, 1 .. 11.
 * Checked before the first HIP call, in curl_msssim_ragged_u8hwc's order and with its codes: NULLs (CURL_E_NULL), flags != 0
 * (CURL_E_FLAGS), a host plan without the stamp, misaligned or of another operator, a mask arena with a plan made without
 * masks, a plan_dev too small or misaligned, an arena smaller than the plan's, stats or workspace NULL, too small or off the
 * 8-byte grid (all CURL_E_WORKSPACE), an arena base off the 4-byte grid (CURL_E_SHAPE), window_size (CURL_E_KNOTS). */
int curl_loss_ragged_u8hwc(const uint8_t* pred_arena, size_t pred_bytes, const uint8_t* target_arena, size_t target_bytes,
                           const uint8_t* mask_arena, size_t mask_bytes, double* stats, size_t stats_bytes,
                           void* workspace, size_t workspace_bytes, const void* host_plan, const void* plan_dev,
                           size_t plan_bytes, int window_size, unsigned flags, curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_RAGGED_LOSS_H */
