"""Shared by the tests of the fused polynomial model's image gradient (host twin and GPU): inputs, the float64 oracle gradient,
the float32 yardstick, the exception set and the error measure.  Not a test module.

Reference: float64 autograd through the oracle of ((residual or generate_image) * w).sum() with respect to the image.
rel_px = per-pixel max over channels of |got - g64|, divided by G = max|g64|.
Yardstick: the oracle's own float32 autograd against float64 on the same inputs (its largest rel_px outside the exception
set), floored at 2^-24.  The code under test may be K yardsticks and never more than CEILING.
K, fixed before any GPU run by counting roundings on the longest path to one value, the method of
tests/test_gpu_poly_layer_bwd.py: the kernel has the forward Horner chain under sigma' (<= 125 sequential FMAs), three
derivative chains of <= 55 and three combining FMAs, and ~40 operations of gate, tapes (hardware exp2 / log2 / rcp, 1 ulp each),
pullbacks and final adds: ~330.  torch has ~3 roundings per monomial term and 7 levels of pairwise sum: ~10.  330 / 10 -> 32,
the K of the stand-alone layer's image gradient.
Exception set (random-float cases only): pixels where the float64 gradient itself moves by more than 1e-3 G when the image
moves by +-1e-6 along three random sign patterns -- near them float32 may take the other side of a converter's branch.  At
most 0.1 % of a case's pixels; reported; still finite.  8-bit content has no exception set."""
import functools
import os

import numpy as np
import torch

from poly_layer_bwd_ref import CEILING  # the project's polynomial-backward ceiling, 2e-4

K = 32
FLOOR = 2.0 ** -24
EXC_MOVE, EXC_STEP, EXC_FRACTION = 1e-3, 1e-6, 1e-3


def bound(yard):
    return min(K * max(yard, FLOOR), CEILING)


def oracle_grad(img, coeffs, w, residual_only, dtype=torch.float64):
    """d ((residual or image) * w).sum() / d img by autograd through the oracle, in `dtype`."""
    import curl_oracle as O
    i = img.detach().clone().to(dtype).requires_grad_()
    c = coeffs.detach().to(dtype)
    res = O.trispace_residual(i, c[:, 0], c[:, 1], c[:, 2], spatial=coeffs.shape[-1] == 126)
    out = res if residual_only else O.generate_image(i, res)
    (out * w.to(dtype)).sum().backward()
    return i.grad


def rel_px(got, g64):
    """[B,H,W]: per-pixel max over channels of |got - g64| / max|g64|"""
    got, g64 = torch.as_tensor(got).detach().cpu().double(), g64.double()
    return (got - g64).abs().amax(1) / g64.abs().max()


def inputs(nc, shape, seed=0):
    """img = rand [B,3,H,W], coeffs = randn * 0.3 [B,3,3,nc] (B distinct tables), w = randn [B,3,H,W]; seeded, on the CPU."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + nc + 17 * B + 7 * H + 13 * W)
    return torch.rand(B, 3, H, W, generator=g), torch.randn(B, 3, 3, nc, generator=g) * 0.3, torch.randn(B, 3, H, W, generator=g)


def exception_set(img, coeffs, w, residual_only, g64):
    """[B,H,W] bool: the float64 gradient moves by more than EXC_MOVE * G under +-EXC_STEP along three random sign patterns."""
    g = torch.Generator().manual_seed(4242)
    G = g64.abs().max()
    exc = torch.zeros(g64.shape[0], g64.shape[2], g64.shape[3], dtype=torch.bool)
    for _ in range(3):
        s = (torch.randint(0, 2, img.shape, generator=g) * 2 - 1).double()
        for sign in (1.0, -1.0):
            moved = oracle_grad(img.double() + sign * EXC_STEP * s, coeffs, w, residual_only)
            exc |= (moved - g64).abs().amax(1) > EXC_MOVE * G
    return exc


@functools.lru_cache(maxsize=None)
def case(nc, residual_only, shape, seed=0):
    """One random-float parity case, computed once per session: (img, coeffs, w, g64, yardstick, exception set).  Callers must
    not modify what they get."""
    img, c, w = inputs(nc, shape, seed)
    g64 = oracle_grad(img, c, w, residual_only)
    exc = exception_set(img, c, w, residual_only, g64)
    r32 = rel_px(oracle_grad(img, c, w, residual_only, torch.float32), g64)
    yard = float(r32[~exc].max()) if bool((~exc).any()) else 0.0
    return img, c, w, g64, yard, exc


@functools.lru_cache(maxsize=None)
def case_8bit(nc, residual_only, B=1):
    """8-bit content: a 64x96 cut of the golden photograph crop, black, white, grey and the three primaries written into row 0
    (exact ties, exact zeros, clamp bounds: the subgradient conventions at the discontinuities).  No exception set: every pixel
    is held to the bound.  B copies of the picture under B distinct coefficient tables."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real8.npz")
    u8 = np.load(path)["crop_u8"][:64, :96].copy()
    u8[0, :6] = np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    img = (torch.from_numpy(u8).permute(2, 0, 1).float() / 255.0)[None].repeat(B, 1, 1, 1).contiguous()
    g = torch.Generator().manual_seed(88 + nc + B)
    c = torch.randn(B, 3, 3, nc, generator=g) * 0.1
    w = torch.randn(B, 3, 64, 96, generator=g)
    g64 = oracle_grad(img, c, w, residual_only)
    yard = float(rel_px(oracle_grad(img, c, w, residual_only, torch.float32), g64).max())
    return img, c, w, g64, yard


def check(got, g64, yard, exc=None, label=""):
    """Print the kernel / yardstick ratio, then hold every pixel outside `exc` to the bound and every pixel to finiteness."""
    got = torch.as_tensor(got).detach().cpu()
    r = rel_px(got, g64)
    n = r.numel()
    n_exc = int(exc.sum()) if exc is not None else 0
    keep = ~exc if exc is not None else torch.ones_like(r, dtype=torch.bool)
    worst = float(r[keep].max()) if bool(keep.any()) else 0.0
    print(f"\nRATIO {label}: {worst:.3g} / {max(yard, FLOOR):.3g} = {worst / max(yard, FLOOR):.2f}  (bound {bound(yard):.3g}; "
          f"exception set {n_exc} of {n} pixels" + (f": {exc.nonzero().tolist()}" if n_exc else "") + ")")
    assert bool(torch.isfinite(got).all()), label
    assert n_exc <= EXC_FRACTION * n, (label, n_exc, n)
    assert worst <= bound(yard), (label, worst, yard, bound(yard))
    return worst / max(yard, FLOOR)
