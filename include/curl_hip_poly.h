/* curl_hip_poly.h -- C ABI of libcurlhip.so, continued: polynomial orders 1..4 of the polynomial model and layers.
 *
 * Conventions, error codes and flags are curl_hip.h's; this header declares no function.  It exists beside curl_hip.h
 * because the set of macro names that header may define is a closed, recorded list (tests/test_build_resources.py); the
 * headers are to be folded together the next time that record is deliberately regenerated.
 */
#ifndef CURL_HIP_POLY_H
#define CURL_HIP_POLY_H

#include "curl_hip.h"

/* curl_poly_layer_f32's `num_variables` for ChannelPolyLayer(degree, V, 3) (model.py:206-333): V = 5 or 3 in the low 16
 * bits, the degree 1..4 in the high 16 bits -- the form CURL_K_UNEVEN gives a knot count.  coeffs is then
 * [B,3,C(V + degree, degree)]: 6, 21, 56, 126 coefficients for V = 5, 4, 10, 20, 35 for V = 3, in the order of the
 * reference's generate_powers.  A high half of 0 means degree 4: a plain 5 or 3 is what it always was, and
 * CURL_POLY_VARS(V, 4) equals it in effect.  Degree 0 has no kernel; so that it is refused instead of being read as that
 * default, the macro packs 0x7fff for it.  It, a degree above 4 and any other V are CURL_E_SHAPE.
 *
 * The backward entry points (curl_poly_layer_bwd_f32, curl_trispace_bwd_f32, curl_trispace_bwd_img_f32) stay degree 4 and
 * take a plain V or 126 | 35: pad a lower degree's table with zeros as curl_hip.h describes there. */
#define CURL_POLY_VARS(V, degree) ((int)((unsigned)(V) | ((unsigned)((degree) > 0 ? (degree) : 0x7fff) << 16)))

/* `num_coeffs` of curl_trispace_fwd_f32, curl_trispace_fwd_slab_f32 and curl_trispace_fwd_u8hwc for
 * TriSpaceRegNet(polynomial_order = order) (model.py:439-454): the coefficients per polynomial in the low 16 bits, the
 * order 1..4 in the high 16 bits.  coeffs is then [B,3,3,num_coeffs] with num_coeffs = C(V + order, order):
 *   spatial model (5 variables):      6, 21, 56, 126 for orders 1..4;      non-spatial (3 variables):  4, 10, 20, 35.
 * The eight counts are all different, so the count alone decides between the two models; the order is said as well because
 * a plain count other than 126 | 35 has always been CURL_E_KNOTS and stays so.  A high half of 0 means order 4;
 * CURL_POLY_COEFFS(126, 4) and CURL_POLY_COEFFS(35, 4) run the kernels a plain 126 and 35 run.  A count that is not the
 * order's, order 0 (packed as 0x7fff) and an order above 4 are CURL_E_KNOTS.  Alignment of coeffs: see curl_hip.h. */
#define CURL_POLY_COEFFS(num_coeffs, order) ((int)((unsigned)(num_coeffs) | ((unsigned)((order) > 0 ? (order) : 0x7fff) << 16)))

#endif /* CURL_HIP_POLY_H */
