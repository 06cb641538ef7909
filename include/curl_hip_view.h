/* curl_hip_view.h -- C ABI of libcurlhip.so, continued: the encoder's input view straight from image bytes.
 *
 * Conventions, error codes and the stream type are curl_hip.h's.  This header exists beside it for the reason
 * curl_hip_grad.h does: the recorded launch plan (tests/data/launch_plan.txt) enumerates curl_hip.h's declarations.
 *
 * replaces: the reference's `cropper(resizer(img))` + TF.to_tensor (infer.py:32-41) -- torchvision's Resize([size]) and
 *           CenterCrop((size, size)) on the DECODED BYTES, i.e. Pillow's 8-bit antialiased bilinear resample (fixed-point,
 *           rounded to bytes after its horizontal and again after its vertical pass) -- and `> 0` for the mask.  The result
 *           equals the reference's bit for bit: the arithmetic is integer, and byte / 255 is correctly rounded.
 *
 * Geometry: the short side of H x W becomes `size`, the long one (size * long) / short (integer division); the crop margins
 * are int(round(margin / 2.0)) with Python's round (halves go to the even integer).  size 8 .. 1024; min(H, W) / size <= 64.
 *
 * The PLAN is the two tables of resampling coefficients of one (H, W, size).  It is built on the host, by the library, into
 * the caller's host memory; the caller uploads it (the library allocates no device memory and copies nothing) and may keep
 * it for every later call of that shape.
 */
#ifndef CURL_HIP_VIEW_H
#define CURL_HIP_VIEW_H

#include <stddef.h>

#include "curl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CURL_VIEW_SIZE_DEFAULT 320
#define CURL_VIEW_SIZE_MIN 8
#define CURL_VIEW_SIZE_MAX 1024
#define CURL_VIEW_MAX_SHRINK 64 /* min(H, W) / size beyond this: CURL_E_SHAPE */

/* Bytes of the plan of an H x W image at `size`; 0 for a shape outside the limits above.  No HIP call. */
size_t curl_encoder_view_plan_bytes(int H, int W, int size);

/* Fills host_buf (HOST memory, 4-byte aligned, `bytes` >= curl_encoder_view_plan_bytes) with the plan.  No HIP call.
 * Layout, all int32: a header of 16 -- a stamp, H, W, size, ow, oh, top, left, ksize_x, ksize_y, six zeros -- then `size`
 * rows {xmin, count, k[ksize_x]} for the cropped output columns, then `size` rows {ymin, count, k[ksize_y]} for the cropped
 * output rows (k in units of 2^-22).  CURL_E_NULL, CURL_E_SHAPE (limits), CURL_E_WORKSPACE (too small / misaligned). */
int curl_encoder_view_plan(int H, int W, int size, void* host_buf, size_t bytes);

/* img [B,H,W,channels] uint8 (channels 3 or 4; of 4 the first three are read), mask [B,H,W] uint8 or NULL, plan_dev the
 * uploaded plan of (H, W, size) -> view [B,3,size,size] float32 = resampled byte / 255, mask_view [B,1,size,size] float32
 * = (resampled mask byte > 0) ? 1 : 0.  mask and mask_view are both set or both NULL (CURL_E_MASK).  flags must be 0.
 * One launch, no scratch, no atomics: a repeated call gives the same bits, an image alone the same as in a batch, from any
 * byte alignment of img and mask.  plan_dev is 4-byte aligned and plan_bytes >= curl_encoder_view_plan_bytes
 * (CURL_E_WORKSPACE).  Every input index is clamped to the image from the call's own H and W: a stale or foreign plan gives
 * wrong values, never an access outside the tensors; a plan whose header names another (H, W, size) gives an all-NaN view
 * (and mask view).  Shape limits as everywhere: B <= 65535, H*W <= 2^30.  Every argument check happens before the first
 * HIP call. */
int curl_encoder_view_u8hwc(const unsigned char* img, int channels, const unsigned char* mask, const void* plan_dev,
                            size_t plan_bytes, float* view, float* mask_view, int B, int H, int W, int size,
                            unsigned flags, curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_VIEW_H */
