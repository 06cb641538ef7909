"""Backward of the fused layer with the paper's piecewise-linear curves (curl_math_bwd.h: curl_layer_pwl_bwd, knot_bwd_pwl) on a
host twin of its own (tests/twin/pwl_twin.cpp), against float64 autograd through a PWL restatement of the layer (below: the
oracle's converters and stage order, each curve the gather form C_i + slope_i f of the paper): random inputs, 8-bit values
with pixels on the knots, saturated inputs (clamps active), bool and soft masks, K = 2, 16 and 256 knots per curve."""
import ctypes

import numpy as np
import pytest
import torch

import curl_oracle as O
from twin_build import FLAVOURS, twin_library

TOL = 2e-4  # knot gradients: relative to the largest; the image gradient: relative to its largest magnitude


# ------------------------------------------------------------------ the restatement (float64 autograd runs through it)
def pwl_scale(x, C):
    """The paper's curve at x [B,H,W] from the exp'd knots C [B,K]: i = clamp(floor(S x), 0, K-2), f = clamp(S x - i, 0, 1),
    scale = C_i + (C_{i+1} - C_i) f.  floor carries no gradient; clamp passes it at its bounds (torch's convention)."""
    B, K = C.shape
    s = (K - 1) * x
    i = torch.clamp(torch.floor(s), 0, K - 2).detach()
    f = torch.clamp(s - i, 0.0, 1.0)
    idx = i.long().reshape(B, -1)
    slope = C[:, 1:] - C[:, :-1]
    Ci = torch.gather(C, 1, idx).reshape(x.shape)
    si = torch.gather(slope, 1, idx).reshape(x.shape)
    return Ci + si * f


def pwl_adjust(img, raw, pairs):
    """curves.py's apply_curve chain (the whole image clamped after every curve) with the paper's curve."""
    reg = torch.zeros(img.shape[0], dtype=img.dtype)
    for C, (cin, cout) in zip([torch.exp(p) for p in torch.chunk(raw, len(pairs), dim=1)], pairs):
        reg = reg + O.curve_regulariser(C)
        out = img.clone()
        out[:, cout] = img[:, cout] * pwl_scale(img[:, cin], C)
        img = torch.clamp(out, 0.0, 1.0)
    return img, reg


def pwl_layer(img, mask, L, R, H):
    """CURLLayer.forward (oracle's curl_layer) with every curve the paper's: what curl_layer_fwd_f32(..., CURL_F_PWL) computes."""
    three = [(0, 0), (1, 1), (2, 2)]
    lab, reg_lab = pwl_adjust(O.rgb2lab(img), L, three)
    rgb, reg_rgb = pwl_adjust(O.lab2rgb(lab * mask), R, three)
    hsv, reg_hsv = pwl_adjust(O.rgb2hsv(rgb * mask), H, [(0, 0), (0, 1), (1, 1), (2, 2)])
    out = torch.clamp(img + O.hsv2rgb(hsv * mask), 0.0, 1.0) * mask
    return out, (reg_rgb + reg_lab) + reg_hsv


def oracle_grads(img, mask, L, R, H, gout, greg, dtype=torch.float64):
    """-> (out, grad_img, grad_L, grad_R, grad_H) by autograd through pwl_layer in `dtype` (numpy arrays, or tensors in)."""
    t = [torch.as_tensor(np.asarray(a)).to(dtype) for a in (img, L, R, H)]
    for a in t:
        a.requires_grad_(True)
    m = torch.ones_like(t[0][:, :1]) if mask is None else torch.as_tensor(np.asarray(mask)).to(dtype)
    out, reg = pwl_layer(t[0], m, t[1], t[2], t[3])
    ((out * torch.as_tensor(np.asarray(gout)).to(dtype)).sum() + (reg * torch.as_tensor(np.asarray(greg)).to(dtype)).sum()).backward()
    return (out.detach().numpy(),) + tuple(a.grad.numpy() for a in t)


def kinks(want32, want64, scale):
    """Pixels where float32 and float64 autograd through the restatement disagree: S x lands on another segment, or a clamp's
    gate closes, in one precision and not in the other -- either one-sided derivative is an answer there."""
    return (np.abs(np.asarray(want32, np.float64) - want64) > TOL * scale).any(axis=1, keepdims=True)


def check_image_grad(got, want, want32, what, max_kinks=0.01):
    scale = max(np.abs(want).max(), 1e-30)
    kink = np.broadcast_to(kinks(want32, want, scale), want.shape)
    assert kink.mean() <= max_kinks, (what, float(kink.mean()))
    d = np.abs(np.asarray(got, np.float64) - want)[~kink]
    assert np.quantile(d, 0.999) <= TOL * scale and d.max() <= 20 * TOL * scale, (what, float(d.max() / scale))


def check_knot_grad(got, want, what, tol=TOL):
    r = float(np.abs(np.asarray(got, np.float64) - want).max() / max(1e-12, np.abs(want).max()))
    assert r <= tol, (what, r)


def smooth_knots(B, n, K, g, amp=0.3):
    """Raw knots of n curves: a random level per curve plus a random walk of K steps of 4 amp / K each -- the curves stay as
    gentle at K = 256 as at K = 16 (independent knots would make S slope grow with K, and the chain's float32 rounding with it)."""
    walk = torch.cumsum(torch.randn(B, n, K, generator=g), 2) * (4 * amp / K)
    return (torch.randn(B, n, 1, generator=g) * amp + walk).reshape(B, n * K)


def knot_tol(want32, want):
    """TOL, or three times the float32 restatement's own error where that is larger: at K = 256 a curve is 255 short segments,
    and the pixels float32 puts on the neighbouring one move their share between two knots (up to 1.3e-4 of the largest)."""
    return max(TOL, 3 * float(np.abs(np.asarray(want32, np.float64) - want).max() / max(1e-12, np.abs(want).max())))


def make_case(case, K, seed, B=2, H=12, W=20):
    """K: knots per curve, one count or one per segment (Kl, Kr, Kh)."""
    Kl, Kr, Kh = (K, K, K) if isinstance(K, int) else K
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g)
    if case == "grid8":
        K = Kr
        img = torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255
        # pixels exactly on knots of the RGB curves' inputs where the 8-bit grid has them (k / (K-1) = b / 255)
        img[:, :, :2] = (torch.randint(0, K, (B, 3, 2, W), generator=g) * (255 // (K - 1) if 255 % (K - 1) == 0 else 0)).float() / 255
    if case == "saturated":
        img = img * 1.6 - 0.3
    mask, binary = None, True
    if case == "boolmask":
        mask = (torch.rand(B, 1, H, W, generator=g) > 0.3).float()
    if case == "softmask":
        mask, binary = torch.rand(B, 1, H, W, generator=g), False
    L, R, Hk = (smooth_knots(B, n, k, g) for n, k in ((3, Kl), (3, Kr), (4, Kh)))
    gout = torch.randn(B, 3, H, W, generator=g)
    greg = torch.rand(B, generator=g)
    return (img.numpy(), None if mask is None else mask.numpy(), binary, L.numpy(), R.numpy(), Hk.numpy(), gout.numpy(),
            greg.numpy())


# ------------------------------------------------------------------ the twin
@pytest.fixture(scope="module", params=FLAVOURS)
def pwl_twin(request):
    """The two flavours of conftest's `twin` fixture, for this twin's own source file."""
    return twin_library("pwl_twin.cpp", request.param)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def twin_layer(lib, img, mask, binary, L, R, Hk, gout, greg):
    img, gout, greg = _f32(img), _f32(gout), _f32(greg)
    raw = _f32(np.concatenate([L, R, Hk], 1))
    mask = None if mask is None else _f32(mask)
    B, _, H, W = img.shape
    Kl, Kr, Kh = L.shape[1] // 3, R.shape[1] // 3, Hk.shape[1] // 4
    gi, gr, fwd = np.zeros_like(img), np.zeros_like(raw), np.zeros_like(img)
    lib.twin_layer_pwl_bwd(_p(img), _p(mask), int(binary), _p(raw), _p(gout), _p(greg), _p(gi), _p(gr), _p(fwd), B,
                           ctypes.c_long(H * W), Kl, Kr, Kh)
    return gi, np.split(gr, [3 * Kl, 3 * Kl + 3 * Kr], axis=1), fwd


CASES = ["random", "grid8", "saturated", "boolmask", "softmask"]


@pytest.mark.parametrize("K", [2, 16, 256])
@pytest.mark.parametrize("case", CASES)
def test_pwl_layer_backward_vs_oracle_autograd(pwl_twin, case, K):
    img, mask, binary, L, R, Hk, gout, greg = make_case(case, K, 300 + CASES.index(case) + K)
    gi, (gL, gR, gH), fwd = twin_layer(pwl_twin, img, mask, binary, L, R, Hk, gout, greg)
    out, wi, wL, wR, wH = oracle_grads(img, mask, L, R, Hk, gout, greg)
    _, wi32, *w32 = oracle_grads(img, mask, L, R, Hk, gout, greg, torch.float32)
    # the oracle is the function the pullback differentiates: its forward is the twin's recomputed forward
    assert np.abs(fwd - out).max() <= 1e-5, (case, K, float(np.abs(fwd - out).max()))
    check_image_grad(gi, wi, wi32, (case, K, "img"))
    for got, want, want32, name in ((gL, wL, w32[0], "L"), (gR, wR, w32[1], "R"), (gH, wH, w32[2], "H")):
        check_knot_grad(got, want, (case, K, name), knot_tol(want32, want))


def test_pwl_regulariser_only(pwl_twin):
    """grad_out = 0: the knot gradient is the regulariser's alone, the image gradient exactly 0."""
    img, mask, binary, L, R, Hk, gout, greg = make_case("random", 16, 9)
    gout = np.zeros_like(gout)
    gi, (gL, gR, gH), _ = twin_layer(pwl_twin, img, mask, binary, L, R, Hk, gout, greg)
    _, _, wL, wR, wH = oracle_grads(img, mask, L, R, Hk, gout, greg)
    assert np.abs(gi).max() == 0
    for got, want, name in ((gL, wL, "L"), (gR, wR, "R"), (gH, wH, "H")):
        check_knot_grad(got, want, name)


def test_pwl_is_not_the_affine_backward(pwl_twin):
    """The knot gradients of the paper's curves differ from the reference's affine form's on the same inputs: a backward
    that quietly ran the affine form would not pass the checks above."""
    img, mask, binary, L, R, Hk, gout, greg = make_case("random", 16, 11)
    _, (gL, _, _), _ = twin_layer(pwl_twin, img, mask, binary, L, R, Hk, gout, greg)
    x = torch.from_numpy(img).double()
    k = [torch.from_numpy(a).double().requires_grad_(True) for a in (L, R, Hk)]
    out, reg = O.curl_layer(x, torch.ones_like(x[:, :1]), *k, L.shape[1], R.shape[1], Hk.shape[1])
    ((out * torch.from_numpy(gout).double()).sum() + (reg * torch.from_numpy(greg).double()).sum()).backward()
    assert np.abs(gL - k[0].grad.numpy()).max() > 10 * TOL * np.abs(gL).max()
