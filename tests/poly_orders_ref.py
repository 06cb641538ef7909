"""Shared by the tests of polynomial orders 1-4 (CPU and GPU): coefficient counts, the order-d reference composed from the
oracle's pieces, zero-padding to the order-4 width, seeded inputs.  Not a test module.

oracle.trispace_residual is written for degree 4; trispace_residual below follows it (oracle/curl_oracle.py:406-418) line for
line with O.channel_poly_layer(., ., degree) as the polynomial."""
import math

import torch

ORDERS = (1, 2, 3, 4)
SHAPES = [(2, 36, 40), (1, 37, 41), (1, 3, 1030), (1, 1, 1), (2, 7, 9)]  # float4 planes and several blocks; odd H*W: the scalar
#                                            kernel; a row wider than a tile; one pixel; a few (tests/test_gpu_parity.py)


def n_coeffs(degree, V):
    return math.comb(V + degree, degree)


NEW_COUNTS = [(d, V, n_coeffs(d, V)) for V in (5, 3) for d in (1, 2, 3)]  # (degree, variables, count): 6, 21, 56, 4, 10, 20
COUNT_IDS = [f"d{d}v{V}" for d, V, _ in NEW_COUNTS]


def degree_of(nc):
    """A table width -> (degree, variables): the eight counts are all different."""
    for V in (5, 3):
        for d in ORDERS:
            if n_coeffs(d, V) == nc:
                return d, V
    raise ValueError(nc)


def trispace_residual(img, R, L, H, degree, spatial=True, rows=None):
    """TriSpaceRegNet.generate_residual (model.py:499-515) with ChannelPolyLayer(degree).  R, L, H: [B,3,n]."""
    import curl_oracle as O

    def poly(x, c):
        return O.channel_poly_layer(x, c, degree)
    rgb_res = torch.sigmoid(poly(O.cat_coords(img, spatial, rows), R))
    lab_res = O.lab2rgb(torch.sigmoid(poly(O.cat_coords(O.rgb2lab(img), spatial, rows), L)))
    hsv_res = O.hsv2rgb(torch.sigmoid(poly(O.cat_coords(O.rgb2hsv(img), spatial, rows), H)))
    rgb_res = 2 * (rgb_res - 0.5)
    lab_res = 2 * (lab_res - 0.5)
    hsv_res = 2 * (hsv_res - 0.5)
    return rgb_res + lab_res + hsv_res


def trispace(img, coeffs, residual_only=False):
    """The composed reference from a [B,3,3,n] table: the residual, or generate_image of it."""
    import curl_oracle as O
    d, V = degree_of(coeffs.shape[-1])
    res = trispace_residual(img, coeffs[:, 0], coeffs[:, 1], coeffs[:, 2], d, spatial=V == 5)
    return res if residual_only else O.generate_image(img, res)


def pad4(c):
    """An order-d table [..., n] as the order-4 table of the same polynomials: zeros for the monomials of degree > d (the
    reference's monomial order is graded, so the order-d monomials are the first n of the order-4 list)."""
    d, V = degree_of(c.shape[-1])
    return torch.nn.functional.pad(c, (0, n_coeffs(4, V) - c.shape[-1]))


def inputs(nc, shape, scale=0.2, seed=0):
    """img = rand [B,3,H,W], coeffs = randn * scale [B,3,3,nc] with the coordinate coefficients of the spatial form made to
    matter (a coordinate mix-up then shows as a ramp), w = randn [B,3,H,W]; seeded, on the CPU."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 31 * nc + 17 * B + 7 * H + 13 * W)
    img = torch.rand(B, 3, H, W, generator=g)
    c = torch.randn(B, 3, 3, nc, generator=g) * scale
    if degree_of(nc)[1] == 5:
        c[..., 4], c[..., 5] = 0.7, -0.5  # x/W and y/H (monomials 4 and 5 of the graded order at every degree >= 1)
    return img, c, torch.randn(B, 3, H, W, generator=g)
