"""The knot-count cases of the curve kernels and their yardstick, shared by tests/test_knot_paths.py (host twins) and
tests/test_gpu_knot_paths.py (the kernels).  A plain module: no fixtures, nothing read from outside the repository.

Why not plain float64: kernels and reference both HOLD float32 knots, C = float32(exp(raw)).  That one rounding,
6e-8, reaches the output amplified by about S K (S = K - 1), so the reference's own float32 result leaves its float64
evaluation by 2e-5 at K = 26 and 5e-4 at K = 256: no fixed bound against plain float64 survives K > 16, and one widened to fit
catches nothing.  The yardstick here is the oracle in float64 STARTING FROM those float32 knots (`rounded`): what prep_image
says it computes ("exp in float64, rounded once to float32"), with the chain behind it exact.  Against it the K = 16 bounds of
tests/test_gpu_parity.py and tests/test_gpu_backward.py hold unchanged at every count; they are stated once, below.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import curl_oracle as O

H_FD = 1e-6  # the finite-difference step of curl_oracle.input_sensitivity / gradient_curvature

SMALL, BIG = (2, 7, 9), (2, 36, 40)  # scalar kernels, less than one block / float4, several blocks; two images, two knot rows
SHAPES = (SMALL, BIG)


# ------------------------------------------------------------------ the yardstick
def rounded(raw):
    """float64, equal in value to log(float32(exp(raw64))), with raw64's gradient (straight-through): the oracle's exp then
    lands on the float32 knot the kernels hold, and d / d raw keeps its factor exp(raw)."""
    raw = raw.double()
    held = torch.exp(raw.detach()).float().double()
    return raw + (torch.log(held) - raw.detach())


def sigma(K):
    """The suite's 0.1 at K = 16, shrinking like 1 / (K - 1) beyond: the curve is affine in x with coefficients of order
    S * (knot variation), and independent knots of 0.1 saturate the whole frame well before K = 256."""
    return min(0.1, 1.5 / (K - 1))


def knots(B, counts, g):
    """Raw knots of one segment, counts = knots per curve (torch.chunk's split: only the last may be shorter).  INDEPENDENT
    normals on purpose: every knot's regulariser gradient then differs from its neighbours'."""
    return torch.randn(B, sum(counts), generator=g) * sigma(counts[0])


def _bump(x, k, d):
    p = x.clone()
    p[:, k] += d
    return p


class Yardstick:
    """fn(img, mask, *raws) -> (out, reg), any oracle composite, in float64 on the rounded knots, for the loss
    sum(out * w) + sum(reg * wr):
        out, reg, g_img, g_knots     values and gradients
        S, C                         per pixel [B,H,W]: the chain's input sensitivity and the image gradient's curvature
        G, jump                      max |g_img|; the exception set H_FD * C > 1e-3 * G
        reg_knots                    knot gradients of the regulariser alone (w = 0, wr = greg = (1, -0.5, ...))
        mask_ex, w_ex, full_knots    mask / cotangent with the exception set taken out, and the knot gradients under them
        pixel_share                  per segment: the part of full_knots that comes through the pixels, of the segment's scale
        delta                        per segment: how far full_knots move (relative) when every image value moves by +-H_FD"""

    def __init__(self, fn, img, mask, raws, w, wr):
        self.fn = fn
        self.x, self.w, self.wr = img.double(), w.double(), wr.double()
        self.mask = mask
        self.raws = [r.double() for r in raws]
        B = img.shape[0]
        self.greg = torch.tensor([(-0.5) ** b for b in range(B)], dtype=torch.float64)  # (1, -0.5, ...)
        m64 = self._m64(mask)
        self.out, self.reg, self.g_img, self.g_knots = self.grads(self.x, m64, self.w, self.wr)
        out, g = self.out, self.g_img
        self.S = torch.zeros_like(out[:, 0])
        self.C = torch.zeros_like(out[:, 0])
        for k in range(3):
            for sgn in (1.0, -1.0):
                p = _bump(self.x, k, sgn * H_FD)
                o, _, gp, _ = self.grads(p, m64, self.w, self.wr)
                self.S = torch.maximum(self.S, (o - out).abs().amax(1) / H_FD)
                self.C = torch.maximum(self.C, (gp - g).abs().amax(1) / H_FD)
        self.G = float(g.abs().max())
        self.jump = H_FD * self.C > 1e-3 * self.G
        self.live = float((g.abs().amax(1) > 0).double().mean())
        self.reg_knots = self.grads(self.x, m64, torch.zeros_like(self.w), self.greg)[3]
        # the knot gradients are sums over the pixels: one gate taken on the other side moves them by that pixel's whole share,
        # so they are compared with the exception set out of BOTH evaluations (tests/test_gpu_backward.py)
        self.mask_ex, self.w_ex, self.full_knots = mask, w, self.g_knots
        if bool(self.jump.any()):
            keep = ~self.jump[:, None]
            if mask is None:
                self.w_ex = w * keep
            else:
                self.mask_ex = mask & keep if mask.dtype == torch.bool else mask * keep
            self.full_knots = self.grads(self.x, self._m64(self.mask_ex), self.w_ex.double(), self.wr)[3]
        # what of them the pixels contribute (wr = 0), relative to the segment's scale
        pix = self.grads(self.x, self._m64(self.mask_ex), self.w_ex.double(), torch.zeros_like(self.wr))[3]
        self.pixel_share = [float(p.abs().max() / f.abs().max().clamp(min=1e-300)) for p, f in zip(pix, self.full_knots)]
        self.delta = [0.0] * len(raws)
        for draw in (0, 1):
            sign = torch.randint(0, 2, self.x.shape, generator=torch.Generator().manual_seed(977 + draw)).double() * 2 - 1
            moved = self.grads(self.x + H_FD * sign, self._m64(self.mask_ex), self.w_ex.double(), self.wr)[3]
            for i, (a, b) in enumerate(zip(moved, self.full_knots)):
                self.delta[i] = max(self.delta[i], float((a - b).abs().max() / b.abs().max().clamp(min=1e-300)))

    @staticmethod
    def _m64(mask):
        return None if mask is None else mask.double()

    def grads(self, x, m64, w, wr):
        x = x.detach().clone().requires_grad_(True)
        ks = [r.detach().clone().requires_grad_(True) for r in self.raws]
        out, reg = self.fn(x, m64, *[rounded(k) for k in ks])
        ((out * w).sum() + (reg * wr).sum()).backward()
        return out.detach(), reg.detach(), x.grad, [k.grad for k in ks]


def _d(t):
    return torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t.detach().cpu()).double()


def check_conditions(Y, what):
    """What a case must be, by the yardstick alone, before anything is compared with it: not a saturated frame, and no
    exception set to speak of (none at all at 2 x 7 x 9).  The layer's image gradient also arrives through model.py:170's
    img + residual while every curve before it is clamped dead (K = 256, 2 x 36 x 40, seed 1: 89 % of the pixels carry
    gradient, and not one reaches the L or R knots); so every segment's knots must hear from the pixels too, or the full
    cotangent checks the regulariser once more."""
    assert Y.G > 0.5, (what, Y.G)
    assert Y.live >= 0.3, (what, Y.live)
    assert min(Y.pixel_share) >= 0.1, (what, Y.pixel_share)
    assert int(Y.jump.sum()) <= 1e-3 * Y.jump.numel(), (what, int(Y.jump.sum()))


def check_forward(Y, out, reg, what):
    """Per pixel |out - yardstick| <= max(1e-5, 2e-6 S) (tests/test_gpu_parity.py); reg relative <= 2e-6: the float32 result's
    own rounding is 6e-8, one dropped or doubled knot moves reg by more than 1e-3.  -> worst error / bound of the pixels."""
    d = (_d(out) - Y.out).abs().amax(1)
    ratio = float((d / torch.clamp(2e-6 * Y.S, min=1e-5)).max())
    assert ratio <= 1.0, (what, "forward", ratio)
    if float(Y.reg.abs().max()) > 0:
        r = float(((_d(reg) - Y.reg).abs() / Y.reg.abs().clamp(min=1e-300)).max())
    else:  # two knots per curve everywhere: no second difference
        r = float(_d(reg).abs().max())
    assert r <= 2e-6, (what, "reg", r)
    return ratio


def check_image_grad(Y, g_img, what):
    """Per pixel |g - yardstick| <= max(2e-6 G, 2e-6 C) outside the exception set, <= 2 G inside (a gate flipped, nothing worse)
    (tests/test_gpu_backward.py).  -> worst error / bound outside the exception set."""
    d = (_d(g_img) - Y.g_img).abs().amax(1)
    bound = torch.clamp(2e-6 * Y.C, min=2e-6 * Y.G)
    ratio = float((d / bound)[~Y.jump].max())
    assert ratio <= 1.0, (what, "image gradient", ratio)
    assert float(d[Y.jump].max() if bool(Y.jump.any()) else 0.0) <= 2.0 * Y.G, (what, "image gradient in the exception set")
    return ratio


def check_reg_knots(Y, got, what):
    """grad_out = 0, grad_reg = Y.greg: every segment within 1e-6 of its largest entry (a gradient shifted by one knot is off
    by 1.5 to 2 of that scale; the float32 reference itself by 4e-6).  K = 2 has no second difference: exact zeros.
    -> worst error / scale."""
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, Y.reg_knots)):
        a, scale = _d(a), float(b.abs().max())
        assert bool(torch.isfinite(a).all()), (what, "regulariser knots", i)
        err = float((a - b).abs().max())
        assert err <= 1e-6 * scale, (what, "regulariser knots", i, err / max(scale, 1e-300))
        worst = max(worst, err / scale if scale > 0 else 0.0)
    return worst


def check_full_knots(Y, got, what):
    """The knot gradients under (Y.mask_ex, Y.w_ex, wr): every segment within max(2e-5, delta) of its scale; delta is the
    reference's own (Yardstick).  -> worst error / bound."""
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, Y.full_knots)):
        a, scale = _d(a), float(b.abs().max())
        assert bool(torch.isfinite(a).all()), (what, "knots", i)
        err, bound = float((a - b).abs().max()), max(2e-5, Y.delta[i]) * scale
        assert err <= bound, (what, "knots", i, err / max(scale, 1e-300), max(2e-5, Y.delta[i]))
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst


# ------------------------------------------------------------------ the cases
def even(n, K):
    return (K,) * n


def chunked(n, N):
    """torch.chunk of N raw parameters into n curves: ceil(N / n) each, the last one the remainder."""
    K = -(-N // n)
    return (K,) * (n - 1) + (N - (n - 1) * K,)


def _layer(Kl, Kr, Kh):
    return (even(3, Kl), even(3, Kr), even(4, Kh))


# name -> (knots per curve of L, R, H; seed at SMALL; seed at BIG).  A seed is the first (from 1) at which check_conditions
# holds and the host twins (tests/test_knot_paths.py) are inside every bound; where a seed moved on, the row says why.
LAYER_CASES = {
    # knot_bwd5's five-knot window clamped on both sides; no used slope at all at 2
    "k2": (_layer(2, 2, 2), 1, 1),
    "k3": (_layer(3, 3, 3), 1, 1),
    "k4": (_layer(4, 4, 4), 1, 1),
    "k5": (_layer(5, 5, 5), 1, 1),
    # prep_image's per-curve 16-lane collapse: one lane idle, all busy, a second round
    "k15_16_17": (_layer(15, 16, 17), 1, 1),
    # prep_image's 256-thread walk: 3 * 24 + 3 * 24 + 4 * 28 = 256 knots, one round exactly; 259, a second round for three
    "n256": (_layer(24, 24, 28), 1, 1),
    "n259": (_layer(25, 24, 28), 1, 1),
    # knots_bwd_kernel: 1 024 knots, knot_bwd5 alone; 1 027, the tail loop's knot_bwd takes the last three
    "n1024": (_layer(100, 100, 106), 1, 1),
    "n1027": (_layer(101, 100, 106), 1, 1),
    # the most include/curl_hip.h promises
    # (2 x 36 x 40, seed 1: no pixel reaches the L or R knots -- check_conditions)
    "k256": (_layer(256, 256, 256), 1, 2),
    # KNOT_OF's segment offsets with three different counts
    "k2_256_5": (_layer(2, 256, 5), 1, 1),
    "k256_2_2": (_layer(256, 2, 2), 1, 1),
    # CURL_K_UNEVEN, the guard-band sweep's raw counts 13 / 26 / 25: (5,5,3), (9,9,8), (7,7,7,4) -- KP_LAST in KNOT_OF
    "uneven_small": ((chunked(3, 13), chunked(3, 26), chunked(4, 25)), 1, 1),
    # ... and a large one, 767 / 26 / 343: (256,256,255), (9,9,8), (86,86,86,85) -- 1 136 knots, an uneven tail loop
    # (2 x 36 x 40, seed 1: the host twin's L gradient is 6.63e-5 of its scale from the yardstick, delta 6.51e-5 -- both
    # flavours, and the kernel 6.89e-5: the case's conditioning, not its code; the seed moved on, no factor added)
    "uneven_large": ((chunked(3, 767), chunked(3, 26), chunked(4, 343)), 1, 2),
}

# op -> name -> (knots per curve; seed at SMALL; seed at BIG): 255 / 258 and 256 / 260 knots straddle stage_knots_bwd_kernel's
# 256 threads, raw 13 and raw 25 are the uneven splits (5,5,3) and (7,7,7,4)
_THREE = {"k2": even(3, 2), "k4": even(3, 4), "k85": even(3, 85), "k86": even(3, 86), "k256": even(3, 256), "raw13": chunked(3, 13)}
_FOUR = {"k2": even(4, 2), "k4": even(4, 4), "k64": even(4, 64), "k65": even(4, 65), "k256": even(4, 256), "raw25": chunked(4, 25)}
STAGE_OPS = {"adjust_rgb": _THREE, "adjust_lab": _THREE, "lab_stage": _THREE, "adjust_hsv": _FOUR, "hsv_stage": _FOUR}
STAGE_SEEDS = {("hsv_stage", "k256", BIG): 2}  # where seed 1 does not do (there: 13 % of the pixels carry gradient)


def is_even(counts):
    return all(len(set(c)) == 1 for c in counts)


def composite(op, counts):
    """The oracle composite of `op` as fn(img, mask, *raws) for Yardstick."""
    n = [sum(c) for c in counts]
    if op == "layer":
        return lambda x, m, L, R, H: O.curl_layer(x, torch.ones_like(x[:, :1]) if m is None else m, L, R, H, *n)
    if op in ("lab_stage", "hsv_stage"):
        return lambda x, m, k: getattr(O, op)(x, torch.ones_like(x[:, :1]) if m is None else m, k, n[0])
    return lambda x, m, k: getattr(O, op)(x, k)


def inputs(op, counts, shape, seed):
    """-> img, mask, raws, w, wr (float32 tensors; the mask bool at SMALL, fractional float32 at BIG: both specialisations;
    None for the curve ops, which take none)."""
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    img = torch.rand(B, 3, H, W, generator=g)
    raws = tuple(knots(B, c, g) for c in counts)
    w = torch.randn(B, 3, H, W, generator=g)
    wr = torch.rand(B, generator=g)
    r = torch.rand(B, 1, H, W, generator=g)
    mask = None
    if not op.startswith("adjust"):
        mask = r > 0.1 if shape == SMALL else torch.where(r > 0.1, 0.5 + 0.5 * r, torch.zeros(()))
    return img, mask, raws, w, wr


def case_table():
    """Every (op, name, shape) of the tables above."""
    rows = [("layer", name, shape) for name in LAYER_CASES for shape in SHAPES]
    rows += [(op, name, shape) for op, names in STAGE_OPS.items() for name in names for shape in SHAPES]
    return rows


def case_id(row):
    op, name, shape = row
    return f"{op}-{name}-{shape[1]}x{shape[2]}"


def lookup(op, name, shape):
    """-> (counts, seed)"""
    if op == "layer":
        counts, s_small, s_big = LAYER_CASES[name]
        return counts, s_small if shape == SMALL else s_big
    return (STAGE_OPS[op][name],), STAGE_SEEDS.get((op, name, shape), 1)


@functools.lru_cache(maxsize=None)
def reference(op, name, shape):
    """The case's inputs and its Yardstick, computed once per process and shared; nobody writes to them."""
    counts, seed = lookup(op, name, shape)
    img, mask, raws, w, wr = inputs(op, counts, shape, seed)
    Y = Yardstick(composite(op, counts), img, mask, raws, w, wr)
    return SimpleNamespace(op=op, name=name, shape=shape, counts=counts, img=img, mask=mask, raws=raws, w=w, wr=wr, Y=Y)
