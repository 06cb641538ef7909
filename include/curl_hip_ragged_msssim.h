/* curl_hip_ragged_msssim.h -- C ABI of libcurlhip.so, continued: the MS-SSIM statistics of a batch of byte images of
 * different sizes against their targets, the whole batch in six launches.
 *
 * Conventions, error codes and the stream type are curl_hip.h's; the arenas are curl_hip_ragged.h's.  This header exists
 * beside the others for the reason they do: the recorded launch plan (tests/data/launch_plan.txt) enumerates curl_hip.h's
 * declarations, and the ABI tests hold every existing _lib.SIGNATURES* table to exactly its header's.
 *
 * replaces: per image, curl_u8hwc_to_f32chw of the result and of the target, two mask multiplies and curl_msssim_fwd_f32
 *           (evaluate.py:102-105, metric.py:75-211 on gt * mask and out * mask): about fourteen launches and 24 bytes of
 *           float image per pixel, for a folder one image at a time.  Here level 0 is computed from the 7 bytes per pixel
 *           (3 + 3 + 1) the batch already has on the device; no full-resolution float image is ever written.
 *
 * Arenas.  a_arena and b_arena: image i's H_i*W_i*3 interleaved RGB bytes at rgb_off[i]; mask_arena (optional): image i's
 * H_i*W_i bytes at mask_off[i].  Offsets follow curl_hip_ragged.h's rule (index order, each rounded up to CURL_RAGGED_ALIGN),
 * so they equal the out_off / mask_off of a curl_ragged_plan for operator 0 and the same shape list.  None of the three is
 * written.  A pixel's values are float32(byte) / 255 (the correctly rounded quotient, to_tensor's) where its mask byte is not
 * 0 -- everywhere without a mask arena -- and 0 where the mask byte is 0.
 *
 * The PLAN is built on the host into the caller's memory, uploaded by the caller, and handed to the entry as both copies, as
 * in curl_hip_ragged.h.  Layout, int32 words, 8-byte aligned; "(i64)" is a little-endian int64 in two words:
 *   header, 32 words:
 *     [0] stamp (CURL_MSSSIM_RAGGED_STAMP)   [1] B   [2] operator (CURL_MSSSIM_RAGGED_OP)   [3] has_mask   [4] launches (6)
 *     [5..9] grid of the launch of level 0..4: the sum of the images' tiles at that level
 *     [12] (i64) a / b arena bytes   [14] (i64) mask arena bytes (0 without masks)   [16] (i64) workspace bytes
 *     [18] (i64) hash of (has_mask, B, every H, W)   [20] (i64) byte offset of the partial pairs in the workspace
 *     [22..26] index of level 0..4's first partial pair (a running sum of the grids)   the rest 0
 *   then B descriptors of 64 words, in image index order:
 *     [0] image index i   [1] H   [2] W   [4] (i64) rgb_off   [6] (i64) mask_off (0 without masks)
 *     [16 + 8*l ...], l = 0..4, pyramid level l:
 *       [+0] h = H >> l   [+1] w = W >> l  (floor halving, avg_pool2d(x, (2, 2)))
 *       [+2] tiles per row = ceil(w / 32)   [+3] tiles = that * ceil(h / 32)
 *       [+4] first workgroup of the image in the level's launch (a running sum)   [+5] index of its first partial pair
 *       [+6] (i64) byte offset in the workspace of the level's float planes (l >= 1; 0 for l = 0): a's three planes
 *            [3][h][w] float32, then b's
 *     the rest 0
 * The workspace holds the float planes of levels 1..4 of every image, then one pair of float64 (sum of the SSIM map, sum of
 * the contrast-structure map over the tile's 3 channels) per workgroup of the five level launches.
 *
 * Limits (CURL_E_SHAPE from curl_msssim_ragged_plan): 1 <= B <= 65535; H_i*W_i <= 2^30; H_i, W_i >= 32 (metric.py:185-192
 * pools once more after the fifth level -- the limit of curl_msssim_fwd_f32; the message names the first offending image).
 *
 * Six launches whatever B is -- level 0 from the bytes, levels 1..4 on the workspace's planes, one finish --, no atomics, no
 * memset, every sum in a fixed order: the same bits on every call, for an image alone or in any company and order.  Safety
 * of the device copy is curl_hip_ragged.h's: every workgroup first compares the device plan's stamp and hash with the host
 * plan's and returns untouched when they differ (stats and the workspace keep what they held); it checks its descriptor's
 * extents against all three arenas and the workspace before it forms an address, and writes a zero pair if one fails.
 */
#ifndef CURL_HIP_RAGGED_MSSSIM_H
#define CURL_HIP_RAGGED_MSSSIM_H

#include <stddef.h>
#include <stdint.h>

#include "curl_hip_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CURL_MSSSIM_RAGGED_STAMP 0x4D535231 /* "1RSM" */
#define CURL_MSSSIM_RAGGED_OP 5             /* the five pyramid levels */
#define CURL_MSSSIM_RAGGED_HEADER_WORDS 32
#define CURL_MSSSIM_RAGGED_DESC_WORDS 64
#define CURL_MSSSIM_RAGGED_LEVEL_WORD 16 /* a descriptor's first level word */
#define CURL_MSSSIM_RAGGED_LEVEL_WORDS 8

/* Bytes of the plan of B images; 0 for a B outside 1 .. 65535.  No HIP call. */
size_t curl_msssim_ragged_plan_bytes(int B);

/* Fills host_buf (HOST memory, 8-byte aligned, `bytes` >= curl_msssim_ragged_plan_bytes(B)) with the plan of the B images
 * H[i] x W[i].  has_mask: the batch has a mask arena.  No HIP call.  CURL_E_NULL, CURL_E_SHAPE (the limits above),
 * CURL_E_WORKSPACE (host_buf too small / misaligned). */
int curl_msssim_ragged_plan(int B, const int* H, const int* W, int has_mask, void* host_buf, size_t bytes);

/* The workspace bytes a host plan asks for (its word [16]); 0 for a buffer that is no such plan.  No HIP call. */
size_t curl_msssim_ragged_workspace_bytes(const void* host_plan);

/* stats[i][0][l] = the mean over image i's 3*h*w values of level l's SSIM map, stats[i][1][l] = that of its
 * contrast-structure map: what curl_msssim_fwd_f32 returns as ssims / mcs for the float images, the float64 mean kept as
 * float64.  stats: [B][2][5] float64 in image INDEX order, 8-byte aligned, stats_bytes >= 80*B.  workspace: 8-byte aligned,
 * workspace_bytes >= curl_msssim_ragged_workspace_bytes(host_plan).  mask_arena nullable (mask_bytes is then not read).
 * window_size odd, 1 .. 11.  Checked before the first HIP call: NULLs (CURL_E_NULL), flags != 0 (CURL_E_FLAGS), a host plan
 * without the stamp, misaligned or of another operator, a mask arena with a plan made without masks, a plan_dev too small
 * or misaligned, an arena smaller than the plan's, stats or workspace NULL, too small or off the 8-byte grid (all
 * CURL_E_WORKSPACE), an arena base off the 4-byte grid (CURL_E_SHAPE), window_size (CURL_E_KNOTS). */
int curl_msssim_ragged_u8hwc(const uint8_t* a_arena, size_t a_bytes, const uint8_t* b_arena, size_t b_bytes,
                             const uint8_t* mask_arena, size_t mask_bytes, double* stats, size_t stats_bytes,
                             void* workspace, size_t workspace_bytes, const void* host_plan, const void* plan_dev,
                             size_t plan_bytes, int window_size, unsigned flags, curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_RAGGED_MSSSIM_H */
