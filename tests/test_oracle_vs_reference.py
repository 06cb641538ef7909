"""Pins the oracle: every function of oracle/curl_oracle.py against the reference's own modules,
bit for bit, on seeded inputs incl. the edge cases of SURVEY.md section 4.  The reference's outputs on
exactly the inputs built here are stored in tests/golden/vs_reference.npz (tests/golden/make_golden_vs_reference.py
runs the reference on this module's own input builders), so the pin holds wherever the suite runs."""
import numpy as np
import pytest
import torch

import curl_oracle as O

K_LIST = [2, 3, 4, 16, 17, 18, 19, 40]
PAIRS = [(0, 0), (0, 1), (1, 1), (2, 2), (2, 0), (1, 2)]
CONVERTERS = [("RGB2LAB", O.rgb2lab), ("LAB2RGB", O.lab2rgb), ("RGB2HSV", O.rgb2hsv), ("HSV2RGB", O.hsv2rgb)]
WRAPPERS = (("adjust_rgb", 48), ("adjust_lab", 48), ("adjust_hsv", 64))


def rnd(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def same(t, a):
    """Bit for bit: the oracle's tensor t against the reference's stored array a (shape and dtype included)."""
    t = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return t.shape == a.shape and t.dtype == a.dtype and np.array_equal(t, a)


# ------------------------------------------------------------------ the inputs (make_golden_vs_reference.py builds from these)
def apply_curve_cases(K):
    """(key, x, C, reg0, cin, cout) for one knot count K: two knot spreads x the six channel pairs."""
    g = torch.Generator().manual_seed(K)
    B, H, W = 2, 19, 23  # H*W odd: not a multiple of 4
    for si, sigma in enumerate((0.1, 1.0)):
        C = torch.exp(torch.randn(B, K, generator=g) * sigma)
        for ci, co in PAIRS:
            x = torch.rand(B, 3, H, W, generator=g) * 2 - 0.5
            r0 = torch.rand(B, generator=g)
            yield f"ac_K{K}_s{si}_{ci}{co}", x, C, r0, ci, co


def in_place_inputs():
    return rnd(0, 1, 3, 4, 4), torch.exp(rnd(1, 1, 16))


def converter_inputs(golden):
    g = golden("converters")
    inputs = [rnd(3, 2, 3, 17, 31), rnd(4, 2, 3, 17, 31) * 3 - 1,
              torch.randint(0, 256, (1, 3, 32, 32), generator=torch.Generator().manual_seed(5)).float() / 255]
    return inputs + [torch.from_numpy(g[k]) for k in ("rgb_in", "lab_in", "hsv_in", "rgbwide_in")]


def psnr_inputs():
    a, b = rnd(1, 2, 3, 9, 11), rnd(2, 2, 3, 9, 11) * 1.4 - 0.2
    m = (rnd(3, 2, 1, 9, 11) > 0.3).float()
    return a, b, m


def transpose_inputs():
    return [rnd(4, 3, 5, 7).numpy(), rnd(5, 2, 3, 5, 7).numpy()]


# ------------------------------------------------------------------ the pins
@pytest.mark.parametrize("K", K_LIST)
def test_apply_curve_bitexact(golden, K):
    ref = golden("vs_reference")
    for key, x, C, r0, ci, co in apply_curve_cases(K):
        b, rb = O.apply_curve(x, C, r0.clone(), ci, co)
        assert same(b, ref[key + "_out"]) and same(rb, ref[key + "_reg"]), key


def test_apply_curve_mutates_regulariser_in_place(golden):
    ref = golden("vs_reference")
    x, C = in_place_inputs()
    r2 = torch.zeros(1)
    _, out2 = O.apply_curve(x, C, r2, 0, 0)
    # the reference returned the very tensor it was handed, updated in place (recorded when the fixture was made)
    assert bool(ref["inplace_returns_input"])
    assert out2 is r2 and same(r2, ref["inplace_reg"]) and r2.item() > 0


@pytest.mark.parametrize("name,ofn", CONVERTERS)
def test_converters_bitexact(golden, name, ofn):
    ref = golden("vs_reference")
    for i, x in enumerate(converter_inputs(golden)):
        keep = x.clone()
        assert same(ofn(x), ref[f"conv_{name}_{i}"]), (name, i)
        assert torch.equal(x, keep), "converter must not modify its input"
    assert not bool(ref[f"conv_{name}_modifies_input"])


def test_wrapper_bugs_still_present(golden):
    """The semantics this repo implements exist BECAUSE these raise: the exception each of the
    reference's adjust_* wrappers raised on (1,3,4,4) pixels and zero knots, recorded when the fixture was made."""
    ref = golden("vs_reference")
    for (fn, n), raised in zip(WRAPPERS, ref["wrapper_raises"]):
        assert str(raised) == "TypeError", (fn, n, str(raised))


def test_psnr_and_transpose(golden):
    ref = golden("vs_reference")
    a, b, m = psnr_inputs()
    assert same(O.psnr(a, b, m), ref["psnr"])
    for i, arr in enumerate(transpose_inputs()):
        assert same(O.chw_to_hwc(arr), ref[f"chw_to_hwc_{i}"])
        hwc = np.ascontiguousarray(O.chw_to_hwc(arr))
        assert same(O.hwc_to_chw(hwc), ref[f"hwc_to_chw_{i}"])
