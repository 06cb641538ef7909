/* curl_hip_fg.h -- C ABI of libcurlhip.so, continued: the file-to-file byte paths, foreground-aware.
 *
 * Conventions, error codes and the stream type are curl_hip.h's.  This header exists beside it for the reason
 * curl_hip_grad.h and curl_hip_view.h do: the recorded launch plan (tests/data/launch_plan.txt) enumerates curl_hip.h's
 * declarations, and the refusals of curl_trispace_fwd_u8hwc / curl_layer_fwd_u8hwc (every flag bit; CURL_F_MASK_FIRST) are
 * pinned.
 *
 * replaces: infer.py:35-47 as curl_trispace_fwd_u8hwc / curl_layer_fwd_u8hwc do -- byte / 255, the model's per-pixel
 *           part, `out * tmask + (1 - tmask)` ("turn background white like in app"), truncating * 255 -- for a mask
 *           that is a segmentation mask: where a mask byte is 0 the result is white whatever the pixel, so a wavefront
 *           whose mask bytes are all 0 stores white and never reads its pixels, and a workgroup of such wavefronts does not
 *           stage its coefficient table either.
 *
 * Both entries:
 *   img      [B,H,W,channels] uint8; channels is 3 or 4, of 4 the first three are read (CURL_E_SHAPE otherwise).  The pixel
 *            bytes under a mask byte of 0 need not be read: they may hold anything.
 *   fg_mask  [B,H,W] uint8, the 'L' mask; required (NULL: CURL_E_MASK).  m = byte / 255; the result is out * m + (1 - m),
 *            two roundings, as in the sibling entries; a byte of 0 gives (255, 255, 255).
 *   out      [B,H,W,3] uint8.
 *   flags    must be 0 (CURL_E_FLAGS).
 * For finite coefficients / knots every byte of `out` equals what the sibling entry writes for the RGB bytes with
 * white_mask = fg_mask (the layer: mask_kind = CURL_MASK_NONE).  One launch (the layer: and the curve collapse), no
 * scratch, no atomics: the same bits on a repeated call, for an image alone or in a batch, from any byte alignment of img,
 * fg_mask and out (all three on the 4-byte grid and H*W a multiple of 4 -- the spatial 126-coefficient model: W -- take the
 * dword kernels).  Shape limits as everywhere: B <= 65535, H*W <= 2^30.  Every argument check happens before the first HIP
 * call.
 */
#ifndef CURL_HIP_FG_H
#define CURL_HIP_FG_H

#include <stddef.h>
#include <stdint.h>

#include "curl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TriSpaceRegNet's per-pixel part.  coeffs and num_coeffs exactly as curl_trispace_fwd_u8hwc takes them: [B,3,3,n] float32,
 * n = 126 | 35 plain or any of the eight (variables, order) counts packed with CURL_POLY_COEFFS (curl_hip_poly.h); 4-byte
 * aligned, the 126-wide table 8-byte aligned (CURL_E_SHAPE); a count that names no pair: CURL_E_KNOTS. */
int curl_trispace_fwd_fg_u8hwc(const uint8_t* img, int channels, const float* coeffs, const uint8_t* fg_mask, uint8_t* out,
                               int B, int H, int W, int num_coeffs, unsigned flags, curl_stream_t stream);

/* CURLLayer.forward without a layer mask (infer.py applies the mask only when compositing).  The knot arguments, reg
 * (nullable, [B]) and the workspace exactly as curl_layer_fwd_u8hwc takes them, CURL_K_UNEVEN included; reg and the workspace
 * rows hold the same bits as after that entry. */
int curl_layer_fwd_fg_u8hwc(const uint8_t* img, int channels, const float* rawL, const float* rawR, const float* rawH,
                            const uint8_t* fg_mask, uint8_t* out, float* reg, void* workspace, size_t workspace_bytes, int B,
                            int H, int W, int Kl, int Kr, int Kh, unsigned flags, curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_FG_H */
