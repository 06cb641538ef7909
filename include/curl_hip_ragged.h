/* curl_hip_ragged.h -- C ABI of libcurlhip.so, continued: the file-to-file byte paths for a batch of images of different
 * sizes, one launch per class of images.
 *
 * Conventions, error codes and the stream type are curl_hip.h's.  This header exists beside it for the reason
 * curl_hip_view.h and curl_hip_fg.h do: the recorded launch plan (tests/data/launch_plan.txt) enumerates curl_hip.h's
 * declarations.
 *
 * replaces: a loop of curl_trispace_fwd_u8hwc / curl_layer_fwd_u8hwc calls, one per photograph (infer.py:35-47 per file).
 *           Every output byte equals what the sibling entry writes for that image alone.
 *
 * A RAGGED BATCH is B images (H_i, W_i, channels_i), channels_i 3 or 4 (of 4 the first three are read).  They live in
 * three ARENAS, one device buffer per role:
 *   image arena  image i's H_i*W_i*channels_i interleaved bytes at byte offset img_off[i];
 *   mask arena   (optional) image i's H_i*W_i 'L' mask bytes at mask_off[i];
 *   out arena    image i's H_i*W_i*3 result bytes at out_off[i].
 * Every offset is a multiple of CURL_RAGGED_ALIGN (16) bytes; the images follow one another in index order with only the
 * padding that needs (the dword kernels need the 4-byte grid; 16 makes a group of four RGBA pixels naturally aligned).  An
 * arena's size is its last image's offset plus that image's bytes.  Padding bytes of the out arena are never written; the
 * image and mask arenas are never written at all.
 *
 * The PLAN is the batch's layout and tiling for ONE operator.  The library builds it on the host into the caller's host
 * memory; the caller uploads a copy (the library allocates no device memory and copies nothing) and hands both to the launch
 * entries: the host copy for the grids and the argument checks, the device copy for the kernels.  It may be kept for every
 * later batch of the same shape list.
 *
 * Classes.  An image is enhanced by the dword kernel (four pixels per lane, dword accesses) iff H_i*W_i % 4 == 0 -- for the
 * spatial order-4 model (126 coefficients), whose workgroups cover one image row each, iff W_i % 4 == 0 --, else by the byte
 * kernel: the sibling entries' rule.  The plan holds one descriptor table per class and an entry launches each non-empty one:
 * at most two launches (the layer: and the curve collapse).  A launch's grid is the sum of its images' workgroups.
 *
 * Layout of the plan (host and device copy alike), int32 words, 8-byte aligned; "(i64)" is a little-endian int64 in two
 * consecutive words starting at an even index:
 *   header, 32 words:
 *     [0] stamp (CURL_RAGGED_STAMP)      [1] B                    [2] operator: the coefficient count, 0 = the curve layer
 *     [3] has_mask                       [4] number of launches   [5] dword-class images   [6] byte-class images
 *     [7] block size of the dword launch [8] its grid             [9] block size of the byte launch   [10] its grid
 *     [11] 0    [12] (i64) image arena bytes    [14] (i64) mask arena bytes (0 without masks)    [16] (i64) out arena bytes
 *     [18] (i64) hash of (operator, has_mask, B, every H, W, channels)    [20..31] 0
 *   then B descriptors of 16 words: the dword class's (in index order), then the byte class's (in index order):
 *     [0] first workgroup of the image within its launch (a running sum)      [1] image index i
 *     [2] H  [3] W  [4] channels  [5] groups n = H*W / 4 (dword class) or H*W (byte class)
 *     [6] groups per row and [7] workgroups per row (spatial order-4 model; else 0)     [8] workgroups of the image   [9] 0
 *     [10] (i64) img_off   [12] (i64) mask_off (0 without masks)   [14] (i64) out_off
 * Callers read the per-image offsets from the descriptors (word [1] names the image).
 *
 * Limits (CURL_E_SHAPE from curl_ragged_plan): 1 <= B <= 65535; H_i, W_i >= 1 and H_i*W_i <= 2^30; channels_i 3 or 4; each
 * launch's grid <= 2^31 - 1 workgroups; each arena < 2^63 bytes.
 *
 * Safety of the device copy: every workgroup first compares the device plan's stamp and hash with the host plan's, which
 * travel as kernel arguments, and returns without touching an arena when they differ; it then checks its descriptor's
 * extents (offset + bytes <= arena bytes, all three arenas) before it forms an address.  A stale or foreign plan gives no
 * output, never an access outside the arenas.
 */
#ifndef CURL_HIP_RAGGED_H
#define CURL_HIP_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#include "curl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CURL_RAGGED_ALIGN 16
#define CURL_RAGGED_STAMP 0x52474731 /* "1GGR" */
#define CURL_RAGGED_HEADER_WORDS 32
#define CURL_RAGGED_DESC_WORDS 16
#define CURL_RAGGED_MAX_IMAGES 65535

/* Bytes of the plan of B images for the operator num_coeffs_or_0 names: the packed num_coeffs of curl_trispace_fwd_u8hwc
 * (126 | 35 plain, or CURL_POLY_COEFFS(count, order)), or 0 for the curve layer.  0 for a B outside 1 .. 65535 or a count
 * that names no operator.  No HIP call. */
size_t curl_ragged_plan_bytes(int B, int num_coeffs_or_0);

/* Fills host_buf (HOST memory, 8-byte aligned, `bytes` >= curl_ragged_plan_bytes) with the plan of the B images H[i] x W[i]
 * x channels[i].  has_mask: the batch has a mask arena.  No HIP call.  CURL_E_NULL, CURL_E_SHAPE (the limits above),
 * CURL_E_KNOTS (a count that names no operator), CURL_E_WORKSPACE (host_buf too small / misaligned). */
int curl_ragged_plan(int B, const int* H, const int* W, const int* channels, int has_mask, int num_coeffs_or_0, void* host_buf,
                     size_t bytes);

/* The three arena sizes a host plan asks for (mask_bytes: 0 without masks).  CURL_E_NULL; CURL_E_WORKSPACE for a buffer that
 * is no plan (stamp).  No HIP call. */
int curl_ragged_arena_bytes(const void* host_plan, size_t* img_bytes, size_t* mask_bytes, size_t* out_bytes);

/* TriSpaceRegNet's per-pixel part on every image of the batch.  coeffs [B,3,3,n] float32 and num_coeffs exactly as
 * curl_trispace_fwd_u8hwc takes them (image i: row i); mask_arena nullable (no compositing, as white_mask = NULL there; a
 * mask arena with a plan built without masks: CURL_E_WORKSPACE).  host_plan: the plan in host memory; plan_dev: its copy in
 * device memory, 8-byte aligned, plan_bytes >= curl_ragged_plan_bytes.  Checked before the first HIP call: NULLs
 * (CURL_E_NULL), flags != 0 (CURL_E_FLAGS), num_coeffs (CURL_E_KNOTS), a host plan with a wrong stamp or made for another
 * operator, a plan_dev too small or misaligned, an arena smaller than the plan's (all CURL_E_WORKSPACE), an arena base off
 * the 4-byte grid and the coefficient alignment of the sibling (CURL_E_SHAPE).  No scratch, no atomics: the same bytes on a
 * repeated call, for an image alone or in any company and order. */
int curl_trispace_fwd_ragged_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* coeffs, const uint8_t* mask_arena,
                                   size_t mask_bytes, uint8_t* out_arena, size_t out_bytes, const void* host_plan,
                                   const void* plan_dev, size_t plan_bytes, int num_coeffs, unsigned flags, curl_stream_t stream);

/* CURLLayer.forward without a layer mask (the mask arena is the white background's, as in curl_layer_fwd_fg_u8hwc) on every
 * image of the batch; the plan is the one of operator 0.  The knot arguments, reg (nullable, [B]) and the workspace exactly as
 * curl_layer_fwd_fg_u8hwc takes them for B images; reg and the workspace rows hold the same bits as after that entry. */
int curl_layer_fwd_ragged_u8hwc(const uint8_t* img_arena, size_t img_bytes, const float* rawL, const float* rawR,
                                const float* rawH, const uint8_t* mask_arena, size_t mask_bytes, uint8_t* out_arena,
                                size_t out_bytes, float* reg, void* workspace, size_t workspace_bytes, const void* host_plan,
                                const void* plan_dev, size_t plan_bytes, int Kl, int Kr, int Kh, unsigned flags,
                                curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_RAGGED_H */
