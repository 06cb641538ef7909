"""Shared by the stand-alone polynomial layer's backward tests (host twin and GPU): inputs, the float64 oracle gradients,
the float32 yardstick and the error measure.  Not a test module."""
import functools

import torch

CEILING = 2e-4  # the project's polynomial-backward ceiling (tests/test_gpu_parity.py, trispace_backward): never exceeded


def rel(a, b):
    """max|a - b| / max|b|"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


def inputs(V, shape, seed=0, scale=0.3):
    """img = rand [B,V,H,W], coeffs = randn * scale [B,3,NC], w = randn [B,3,H,W] (the upstream gradient), seeded, on the CPU."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 100 * V + B + 7 * H + 13 * W)
    img = torch.rand(B, V, H, W, generator=g)
    c = torch.randn(B, 3, 126 if V == 5 else 35, generator=g) * scale
    w = torch.randn(B, 3, H, W, generator=g)
    return img, c, w


def oracle_grads(img, c, w, dtype=torch.float64, mobile=False):
    """(grad_img, grad_coeffs) of sum(layer(img, c) * w) by autograd through the oracle's layer, in `dtype`."""
    import curl_oracle as O
    i, k = img.detach().clone().to(dtype).requires_grad_(), c.detach().clone().to(dtype).requires_grad_()
    out = O.deg4_mobile_poly_layer(i, k) if mobile else O.channel_poly_layer(i, k, 4)
    (out * w.to(dtype)).sum().backward()
    return i.grad, k.grad


@functools.lru_cache(maxsize=None)
def case(V, shape, mobile=False, seed=0):
    """One parity case, computed once per session: inputs, float64 reference, and the yardstick = the error of the oracle's
    own float32 autograd on the same inputs against float64, per gradient.  Callers must not modify what they get."""
    img, c, w = inputs(V, shape, seed)
    ref = oracle_grads(img, c, w, torch.float64, mobile)
    f32 = oracle_grads(img, c, w, torch.float32, mobile)
    return img, c, w, ref, (rel(f32[0], ref[0]), rel(f32[1], ref[1]))
