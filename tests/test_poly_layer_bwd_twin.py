"""Host twin of the stand-alone polynomial layer's backward (tests/twin/poly_layer_bwd_twin.cpp: curl_math_poly.h compiled for
the host) against float64 autograd through the oracle's layers, and the generated derivative tables against the monomial
order itself.

Bounds (rel = max|a - b| / max|b| against the float64 oracle gradient).  The yardstick is the oracle's own float32 autograd on
the same inputs (1e-7 .. 2.4e-7 here), floored at 2^-24: no float32 result is expected closer than half an ulp of its largest
element.  The twin may be a factor k off it, k counted from the roundings its order of operations adds over torch's, not from
its results:
  image gradient:       3 chains of <= 55 sequential FMAs and 3 combining ones per value, torch a handful per term    k = 32
  coefficient gradient: a lane's chain of <= 64 pixels, 256 lane sums added in sequence (the kernel adds them as a tree;
                        the tile rows are float64 in both), torch sums pairwise: (64 + 256) / ~3 -> next power of two    k = 128
and never more than the project's polynomial-backward ceiling of 2e-4."""
import ctypes

import numpy as np
import pytest
import torch

from poly_layer_bwd_ref import CEILING, case, rel
from twin_build import FLAVOURS, twin_library

K_IMG, K_COEF = 32, 128
FLOOR = 2.0 ** -24


@pytest.fixture(scope="module", params=FLAVOURS)
def bwd_twin(request):
    """The two flavours of conftest's `twin` fixture, for this twin's own source file."""
    return twin_library("poly_layer_bwd_twin.cpp", request.param)


def _P(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _twin_grads(lib, img, c, w, steps=4):
    img, c, w = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (img, c, w))
    B, V, H, W = img.shape
    gimg, gc = np.empty_like(img), np.empty_like(c)
    assert lib.twin_poly_layer_img_grad(_P(img), _P(c), _P(w), _P(gimg), B, ctypes.c_long(H * W), V) == 0
    assert lib.twin_poly_layer_coef_grad(_P(img), _P(w), _P(gc), B, ctypes.c_long(H * W), V, steps) == 0
    return torch.from_numpy(gimg), torch.from_numpy(gc)


@pytest.mark.parametrize("V,shape,mobile", [(3, (2, 20, 64), False), (5, (1, 37, 41), False), (5, (1, 37, 41), True)],
                         ids=["v3", "v5", "v5-deg4-mobile"])
def test_twin_against_float64_autograd(bwd_twin, V, shape, mobile):
    img, c, w, ref, yard = case(V, shape, mobile)
    got = _twin_grads(bwd_twin, img, c, w)
    e_img, e_coef = rel(got[0], ref[0]), rel(got[1], ref[1])
    print(f"V={V} {shape} mobile={mobile}: image {e_img:.3g} (yardstick {yard[0]:.3g}), coeffs {e_coef:.3g} (yardstick {yard[1]:.3g})")
    assert e_img <= min(K_IMG * max(yard[0], FLOOR), CEILING)
    assert e_coef <= min(K_COEF * max(yard[1], FLOOR), CEILING)


def test_twin_tile_size_only_reorders(bwd_twin):
    """Another tile size (more pixels per lane) adds the same terms in another order."""
    img, c, w, ref, yard = case(5, (1, 37, 41))
    a, b = _twin_grads(bwd_twin, img, c, w, steps=4)[1], _twin_grads(bwd_twin, img, c, w, steps=1)[1]
    assert rel(b, ref[1]) <= min(K_COEF * max(yard[1], FLOOR), CEILING)
    assert rel(a, b) <= 2 * min(K_COEF * max(yard[1], FLOOR), CEILING)


@pytest.mark.parametrize("V", [3, 5])
def test_generated_derivative_tables(bwd_twin, V):
    """d m_t / d v_i = p_{t,i} * m_{t - e_i}: for every variable i, every coefficient index t with p_{t,i} > 0 is named exactly
    once, with multiplier p_{t,i}, by the table entry of monomial t - e_i (the monomials of degree <= 3 are the first 20 / 56
    of the graded order)."""
    from curl_amd.model import _powers
    powers = _powers(4, V)
    n3 = len(_powers(3, V))
    assert powers[:n3] == _powers(3, V)
    idx, mul = np.zeros((V, n3), np.int32), np.zeros((V, n3), np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    assert bwd_twin.twin_poly_deriv_tables(V, idx.ctypes.data_as(ip), mul.ctypes.data_as(ip)) == n3
    for i in range(V):
        want = {t: p[i] for t, p in enumerate(powers) if p[i] > 0}
        named = [int(t) for t in idx[i]]
        assert sorted(named) == sorted(want), i                     # each exactly once, and no other
        for u in range(n3):
            t = named[u]
            assert mul[i][u] == want[t], (i, u)                     # the multiplier is p_{t,i}
            e = tuple(p - (1 if k == i else 0) for k, p in enumerate(powers[t]))
            assert powers[u] == e, (i, u)                           # the monomial is t - e_i
