/* curl_hip_grad.h -- C ABI of libcurlhip.so, continued: the image gradient of the fused polynomial model.
 *
 * Conventions, error codes and flags are curl_hip.h's.  This header exists beside it because the recorded launch plan
 * (tests/data/launch_plan.txt) enumerates curl_hip.h's declarations; the two headers are to be folded together the next
 * time that record is deliberately regenerated.
 */
#ifndef CURL_HIP_GRAD_H
#define CURL_HIP_GRAD_H

#include "curl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* replaces: autograd of curl_trispace_fwd_f32 w.r.t. the IMAGE -- what loss.backward() runs through
 *           TriSpaceRegNet.generate_residual + generate_image (model.py:499-520) when a tensor upstream of the model
 *           requires grad (a learnable stage in front of it, a saliency map); the reference gets it from eager autograd
 *           through colors.py, model.py:295-333 / 399-415, torch.sigmoid and torch.clamp.
 * img [B,3,H,W], coeffs [B,3,3,num_coeffs], grad_out [B,3,H,W] (= d loss / d out) -> grad_img [B,3,H,W], ASSIGNED.
 * flags: CURL_F_RESIDUAL_ONLY as in the forward, or 0; every other bit is CURL_E_FLAGS.  num_coeffs 126 or 35; coeffs
 * 8-byte aligned for 126, as in the forward.  The coordinates x/W, y/H of the spatial form are data: no gradient.
 * grad_img may alias grad_out (each lane reads its pixels before it stores them); it must not alias img or coeffs
 * (CURL_E_SHAPE).  Shape limits as everywhere: B <= 65535, H*W <= 2^30.
 * One per-pixel pass, no scratch, no atomics: the result is a function of the pixel and its coordinates alone -- a repeated
 * call is bit-identical, and so is an image computed alone or in a batch, from aligned or unaligned pointers.
 * torch's conventions at the discontinuities (clamp passes its bounds, max/min send the gradient to the first index,
 * masks carry none), as the other backward entry points.  Every argument check happens before the first HIP call. */
int curl_trispace_bwd_img_f32(const float* img, const float* coeffs, const float* grad_out, float* grad_img,
                              int B, int H, int W, int num_coeffs, unsigned flags, curl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CURL_HIP_GRAD_H */
