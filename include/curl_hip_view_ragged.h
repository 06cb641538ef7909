/* curl_hip_view_ragged.h -- C ABI of libcurlhip.so, continued: the encoder's input views of a batch of images of different
 * sizes, straight from the image bytes, in ONE launch.
 *
 * Conventions, error codes and the stream type are curl_hip.h's; the view itself -- geometry, arithmetic, limits -- is
 * curl_hip_view.h's.  This header exists beside that one for the reason curl_hip_ragged.h exists beside curl_hip.h: the tests
 * of each earlier header hold it to the list of entry points it was released with.
 *
 * replaces: a loop of curl_encoder_view_u8hwc calls, one per photograph, and the concatenation of their results.  Every value
 *           equals what that entry writes for the image alone, bit for bit (Pillow's): one copy of the tile code serves both.
 *
 * The BATCH is curl_hip_ragged.h's: B images (H_i, W_i, channels_i), channels_i 3 or 4 (of 4 the first three are read), in an
 * image arena and, optionally, a mask arena; image i's bytes at img_off[i] / mask_off[i], every offset a multiple of 16, in
 * index order with only the padding that needs.  The offsets are the ones curl_ragged_plan gives the same list (one layout
 * function in the library): the arenas that feed curl_*_fwd_ragged_u8hwc feed this entry as they are.  The arenas are read at
 * any byte alignment and never written.
 *
 * Outputs: view [B,3,size,size] and mask_view [B,1,size,size] float32, image i's view at index i.
 *
 * The PLAN is the batch's layout, every image's tiling and the coefficient tables of every DISTINCT (H, W) -- images of one
 * shape share one pair of tables.  The library builds it on the host into the caller's host memory; the caller uploads a copy
 * (the library allocates no device memory and copies nothing) and hands both to the launch entry: the host copy for the grid
 * and the argument checks, the device copy for the kernel.  It may be kept for every later batch of the same shape list.
 *
 * Tiling.  Every image keeps the tile, the window caps and the LDS layout curl_encoder_view_u8hwc gives it alone.  The grid is
 * the sum of the images' tiles; a workgroup finds its image by a binary search of the descriptors' first workgroups.  The
 * launch reserves the largest image's LDS (never more than 48 KiB); each workgroup lays its own image's numbers out in it.
 *
 * Layout of the plan (host and device copy alike), int32 words, 8-byte aligned; "(i64)" is a little-endian int64 in two
 * consecutive words starting at an even index:
 *   header, 32 words:
 *     [0] stamp (CURL_VIEW_RAGGED_STAMP)   [1] B   [2] size   [3] has_mask   [4] grid (workgroups)
 *     [5] dynamic LDS bytes of the launch = the largest descriptor's [15]   [6] number of distinct (H, W)   [7] 0
 *     [8] (i64) image arena bytes   [10] (i64) mask arena bytes (0 without masks)
 *     [12] (i64) hash of (size, has_mask, B, every H, W, channels)   [14] (i64) bytes of the whole plan   [16..31] 0
 *   then B descriptors of 32 words, in index order:
 *     [0] first workgroup of the image (a running sum)   [1] image index i   [2] H   [3] W   [4] channels
 *     [5] workgroups (tiles) of the image
 *     [6] taps per row of the column table (ksize_x)   [7] of the row table (ksize_y)
 *     [8] log2 of the tile's columns   [9] the tile's rows
 *     [10] the most input columns and [11] input rows one tile's window holds   [12] input rows staged at a time
 *     [13] LDS bytes of one staged image row   [14] of one staged mask row (0 without masks)   [15] LDS bytes of a workgroup
 *     [16] (i64) first word of the image's tables in the plan   [18] words of those tables   [19] 0
 *     [20] (i64) img_off   [22] (i64) mask_off (0 without masks)   [24..31] 0
 *   then, per distinct (H, W) in the order of first appearance, the words curl_encoder_view_plan writes after its 16-word
 *   header: `size` rows {xmin, count, k[ksize_x]} for the cropped output columns, then `size` rows {ymin, count, k[ksize_y]}.
 *
 * Limits (CURL_E_SHAPE from curl_encoder_view_ragged_plan): 1 <= B <= 65535; size 8 .. 1024; every image inside
 * curl_hip_view.h's limits (H_i, W_i >= 1, min(H_i, W_i) / size <= 64) and H_i*W_i <= 2^30; channels_i 3 or 4; the grid
 * <= 2^31 - 1 workgroups.
 *
 * Safety of the device copy: every workgroup first compares the device plan's stamp and hash with the host plan's, which
 * travel as kernel arguments, and returns without reading an arena or writing anything when they differ.  It then holds its
 * descriptor to the host plan's numbers before it forms an address: image index < B, channels 3 or 4, its tile < the image's
 * tiles, offset + H*W*channels <= arena bytes (both arenas), the tables inside the plan's bytes, the tiling fields inside
 * their ranges and the LDS they need inside the LDS the launch reserved; a descriptor that fails returns without writing.
 * Past that every index from the tables is clamped to the tile's window and to the image, as in curl_encoder_view_u8hwc:
 * stale tables under a valid header give wrong values in [0, 1], never an access outside the buffers or the LDS.
 */
#ifndef CURL_HIP_VIEW_RAGGED_H
#define CURL_HIP_VIEW_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#include "curl_hip_view.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CURL_VIEW_RAGGED_STAMP 0x52565031 /* "1PVR" */
#define CURL_VIEW_RAGGED_HEADER_WORDS 32
#define CURL_VIEW_RAGGED_DESC_WORDS 32
#define CURL_VIEW_RAGGED_MAX_IMAGES 65535

/* Bytes of the plan of the B images H[i] x W[i] at `size`; 0 outside the limits above (or for a NULL list).  No HIP call. */
size_t curl_encoder_view_ragged_plan_bytes(int B, const int* H, const int* W, int size);

/* Fills host_buf (HOST memory, 8-byte aligned, `bytes` >= curl_encoder_view_ragged_plan_bytes) with the plan of the B images
 * H[i] x W[i] x channels[i].  has_mask: the batch has a mask arena.  No HIP call.  CURL_E_NULL, CURL_E_SHAPE (the limits
 * above), CURL_E_WORKSPACE (host_buf too small / misaligned). */
int curl_encoder_view_ragged_plan(int B, const int* H, const int* W, const int* channels, int has_mask, int size,
                                  void* host_buf, size_t bytes);

/* The views of every image of the batch in one launch.  mask_arena and mask_view are both set or both NULL (CURL_E_MASK); a
 * mask arena needs a plan built with has_mask (CURL_E_WORKSPACE), a plan built with it serves a call without masks too.
 * host_plan: the plan in host memory; plan_dev: its copy in device memory, 8-byte aligned, plan_bytes >= the plan's bytes.
 * `size` is the plan's; flags must be 0 (CURL_E_FLAGS).  Checked before the first HIP call: NULLs (CURL_E_NULL), a host plan
 * with a wrong stamp or made for another size, a plan_dev too small or misaligned, an arena smaller than the plan's (all
 * CURL_E_WORKSPACE), view / mask_view off the 4-byte grid (CURL_E_SHAPE).  No scratch, no atomics: the same bits on a
 * repeated call, for an image alone or in any company and order. */
int curl_encoder_view_ragged_u8hwc(const uint8_t* img_arena, size_t img_bytes, const uint8_t* mask_arena, size_t mask_bytes,
                                   const void* host_plan, const void* plan_dev, size_t plan_bytes, float* view,
                                   float* mask_view, int size, unsigned flags, curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_VIEW_RAGGED_H */
