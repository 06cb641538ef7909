"""What "right" means for a gradient of the criterion's pointwise terms (model.py:89-109), pixel by pixel -- shared by
tests/test_gpu_criterion.py, tests/test_gpu_backward.py and tests/test_loss.py (a plain module, not a conftest).

The yardsticks are float64 autograd through curl_oracle (`g64`) and the same autograd in float32 on the CPU (`g32`):
  live       mask != 0
  ordinary   live and |pred * mask|_inf >= 1/255
  S          max |g64[px]|_inf over the ordinary pixels
  tol(px)    1e-5 * max(S, |g64[px]|_inf)  (+ an allowance the caller adds, e.g. the MS-SSIM share)
             1e-5 is the device figure test_loss_backward_where_prediction_equals_target_and_at_black holds; a black
             prediction, whose cosine gradient is target / (1e-8 |target|), is held relative to ITS OWN magnitude, an ordinary
             pixel relative to S -- never to the black pixels
  ambiguous  |g32[px] - g64[px]|_inf > tol(px): the reference's own float32 decides a kink (a sign, a clamp gate, a hue
             sector) the other way
A gradient passes when every non-ambiguous pixel is within tol(px) of g64, every ambiguous pixel within tol(px) of g64 OR of
g32, and every masked-out pixel is exactly 0.  That ambiguous pixels are rare (<= 0.1 % of the live ones) is a condition on
the INPUTS: loss_gradient_reference asserts it from the oracle alone, before anything else runs."""
import torch

import curl_oracle as O

REL = 1e-5                 # tol(px) / max(S, |g64[px]|)
ORDINARY_FROM = 1.0 / 255  # |pred * mask|_inf from which a live pixel counts towards S
MAX_AMBIGUOUS = 1e-3       # share of the live pixels


def full_mask(mask, pred):
    """The mask as [B,1,H,W] float64 (None: ones; a one-image mask is broadcast as the reference does)."""
    B, _, H, W = pred.shape
    if mask is None:
        return torch.ones(B, 1, H, W, dtype=torch.float64)
    return mask.reshape(-1, 1, H, W).to(torch.float64).expand(B, 1, H, W)


def oracle_gradient(pred, tgt, mask, w, g_Lp=None, dtype=torch.float64, extra=None):
    """d / d pred of w[0] rgb + w[1] cosine + w[2] lab + w[3] hsv + <g_Lp, L_pred> (+ extra(L_pred, L_target)) through the
    oracle, evaluated in `dtype` on the CPU."""
    p = pred.detach().clone().to(dtype).requires_grad_(True)
    m = torch.ones(pred.shape[0], 1, *pred.shape[2:], dtype=dtype) if mask is None else (mask if mask.dtype == torch.bool else mask.to(dtype))
    rgb, cosine, lab, hsv, Lp, Lt = O.curl_loss_terms(p, tgt.to(dtype), m)
    total = w[0] * rgb + w[1] * cosine + w[2] * lab + w[3] * hsv
    if g_Lp is not None:
        total = total + (Lp * g_Lp.to(dtype)).sum()
    if extra is not None:
        total = total + extra(Lp, Lt)
    total.backward()
    return p.grad


def sum_weights(w, mask, pred):
    """The weights of the per-pixel SUMS (d term / d sum, what ops.loss_terms_backward takes) for term weights w: float32 [4]."""
    B, _, H, W = pred.shape
    unmasked = 3.0 * (float(B * H * W) if mask is None else float(mask.double().sum()))
    return torch.tensor([w[0] / unmasked, -w[1] / (B * H * W), w[2] / unmasked, w[3] / unmasked], dtype=torch.float64).float()


class Reference:
    """g64, g32 and everything derived from them alone.  `allow` [B,H,W] (optional) is added to tol(px)."""

    def __init__(self, pred, tgt, mask, g64, g32, allow=None, label=""):
        self.pred, self.tgt, self.label = pred.detach().double().cpu(), tgt.detach().double().cpu(), label
        self.mask = full_mask(None if mask is None else mask.detach().cpu(), pred)
        self.g64, self.g32 = g64.detach().double().cpu(), g32.detach().double().cpu()
        m = self.mask[:, 0]
        self.live = m != 0
        self.ordinary = self.live & ((self.pred * self.mask).abs().amax(1) >= ORDINARY_FROM)
        mag = self.g64.abs().amax(1)
        self.S = float(mag[self.ordinary].max()) if bool(self.ordinary.any()) else 0.0
        self.tol = REL * torch.clamp(mag, min=self.S)
        if allow is not None:
            self.tol = self.tol + allow.detach().double().cpu()
        self.ambiguous = self.live & ((self.g32 - self.g64).abs().amax(1) > self.tol)
        n_live = int(self.live.sum())
        self.ambiguous_share = int(self.ambiguous.sum()) / max(1, n_live)
        # a condition on the inputs, from the reference alone.  (Below 1000 live pixels one pixel is already more than 0.1 %:
        # there the count itself must be 0.)
        assert int(self.ambiguous.sum()) <= MAX_AMBIGUOUS * n_live, (
            f"{label}: {int(self.ambiguous.sum())} of {n_live} live pixels are ambiguous in the reference's own float32 "
            f"(> {MAX_AMBIGUOUS:.1%}): choose other inputs")

    def describe(self, got, b, y, x):
        f = lambda t: [float(v) for v in t[b, :, y, x]]  # noqa: E731
        return (f"{self.label} pixel (b={b}, y={y}, x={x}): pred={f(self.pred)} target={f(self.tgt)} "
                f"mask={float(self.mask[b, 0, y, x])} ambiguous={bool(self.ambiguous[b, y, x])}\n"
                f"  got={f(got)}\n  g64={f(self.g64)}\n  g32={f(self.g32)}\n  tol={float(self.tol[b, y, x]):.3e} S={self.S:.3e}")

    def worst(self, got):
        """max over the non-ambiguous live pixels of |got - g64|_inf / tol(px) (the figure DESIGN.md tabulates)."""
        got = got.detach().double().cpu()
        r = (got - self.g64).abs().amax(1) / self.tol.clamp(min=1e-300)
        sel = self.live & ~self.ambiguous
        return float(r[sel].max()) if bool(sel.any()) else 0.0

    def check(self, got):
        """Assert `got` [B,3,H,W] against the protocol; on failure the message names the worst pixel."""
        got = got.detach().double().cpu()
        assert got.shape == self.g64.shape, (got.shape, self.g64.shape)
        dead = ~self.live
        bad_dead = dead & (got != 0).any(1)  # (NaN != 0 is True: a NaN under the mask fails here)
        if bool(bad_dead.any()):
            b, y, x = (int(v) for v in bad_dead.nonzero()[0])
            raise AssertionError(f"masked-out pixel is not exactly 0 ({int(bad_dead.sum())} such)\n" + self.describe(got, b, y, x))
        d64 = (got - self.g64).abs().amax(1)
        d32 = (got - self.g32).abs().amax(1)
        d64 = torch.where(torch.isnan(d64), torch.full_like(d64, float("inf")), d64)
        d32 = torch.where(torch.isnan(d32), torch.full_like(d32, float("inf")), d32)
        err = torch.where(self.ambiguous, torch.minimum(d64, d32), d64)
        over = self.live & ~(err <= self.tol)
        if bool(over.any()):
            ratio = torch.where(over, err / self.tol.clamp(min=1e-300), torch.zeros_like(err))
            b, y, x = (int(v) for v in (ratio == ratio.max()).nonzero()[0])
            raise AssertionError(f"{int(over.sum())} live pixels beyond tol(px); the worst is {float(ratio.max()):.3g} x tol\n"
                                 + self.describe(got, b, y, x))
        return self.worst(got)


def loss_gradient_reference(pred, tgt, mask, w, g_Lp=None, extra=None, allow=None, label=""):
    """The reference for d / d pred of the weighted terms (oracle_gradient's objective), with the input condition asserted."""
    g64 = oracle_gradient(pred, tgt, mask, w, g_Lp, torch.float64, extra)
    g32 = oracle_gradient(pred, tgt, mask, w, g_Lp, torch.float32, extra)
    return Reference(pred, tgt, mask, g64, g32, allow, label)


# ------------------------------------------------------------------------------------------------------------------
# MS-SSIM statistics (metric.py:120-208): the per-level means and their pullback under INDEPENDENT cotangents
# ------------------------------------------------------------------------------------------------------------------
MSSSIM_LEVELS = 5


def msssim_level_stats(a, b, window_size):
    """(ssims [B,5], mcs [B,5]) through the oracle's ssim_and_cs, level by level over avg_pool2d, in a's dtype."""
    import torch.nn.functional as F
    window = O.msssim_window(window_size, a.shape[1])
    ssims, mcs = [], []
    for _ in range(MSSSIM_LEVELS):
        s, c = O.ssim_and_cs(a, b, window)
        ssims.append(s)
        mcs.append(c)
        a, b = F.avg_pool2d(a, (2, 2)), F.avg_pool2d(b, (2, 2))
    return torch.stack(ssims, 1), torch.stack(mcs, 1)


class MsssimReference:
    """Statistics and d (sum g_ssims ssims + g_mcs mcs) / d a in float64 and in float32, and the oracle's own float32-vs-
    float64 deviations r32: MS-SSIM is ill-conditioned in float32 (a variance is a difference of two blurs), so the
    tolerance is not fixed in advance but taken from r32 -- allow `factor` x r32 for the gradient, capped at 1e-3 of its
    scale, and max(2e-6, factor x r32) for the statistics; factor 4 because two float32 evaluations with different summation
    orders are compared."""

    def __init__(self, a, b, window_size):
        self.window_size = window_size
        self.out, self.leaf = {}, {}
        for dtype in (torch.float64, torch.float32):
            leaf = a.detach().clone().to(dtype).requires_grad_(True)
            self.leaf[dtype] = leaf
            self.out[dtype] = msssim_level_stats(leaf, b.to(dtype), window_size)
        s64, s32 = self.out[torch.float64], self.out[torch.float32]
        self.stats64 = torch.stack((s64[0].detach(), s64[1].detach()))
        self.r32_stats = float((torch.stack((s32[0].detach(), s32[1].detach())).double() - self.stats64).abs().max())
        self.stats_bound = max(2e-6, 4.0 * self.r32_stats)

    def gradient(self, g_ssims, g_mcs, factor=4.0):
        """-> (g64, r32, bound, scale) for these cotangents [B,5] each."""
        g = {}
        for dtype in (torch.float64, torch.float32):
            s, c = self.out[dtype]
            total = (g_ssims.to(dtype) * s).sum() + (g_mcs.to(dtype) * c).sum()
            g[dtype], = torch.autograd.grad(total, self.leaf[dtype], retain_graph=True)
        g64 = g[torch.float64]
        r32 = float((g[torch.float32].double() - g64).abs().max())
        scale = float(g64.abs().max())
        return g64, r32, min(factor * r32, 1e-3 * scale), scale


def msssim_allowance(pred, tgt, mask, term, window_size=11):
    """For the whole criterion: what the MS-SSIM share of each pixel's gradient may be off by, [B,H,W].  `term(Lp, Lt)` is
    the MS-SSIM part of the objective.  Its gradient on the L plane is allowed A = min(4 r32, 1e-3 scale) (MsssimReference's
    rule, r32 from the oracle alone); a pixel's share of that is A * |d L_pred / d pred|_inf there."""
    p = pred.detach().clone().double().requires_grad_(True)
    m = torch.ones(pred.shape[0], 1, *pred.shape[2:], dtype=torch.float64) if mask is None else (mask if mask.dtype == torch.bool else mask.double())
    Lp, Lt = O.curl_loss_terms(p, tgt.double(), m)[4:6]
    dL, = torch.autograd.grad(Lp.sum(), p)
    g = {}
    for dtype in (torch.float64, torch.float32):
        leaf = Lp.detach().to(dtype).requires_grad_(True)
        g[dtype], = torch.autograd.grad(term(leaf, Lt.detach().to(dtype)), leaf)
    r32 = float((g[torch.float32].double() - g[torch.float64]).abs().max())
    A = min(4.0 * r32, 1e-3 * float(g[torch.float64].abs().max()))
    return A * dL.abs().amax(1)


# ------------------------------------------------------------------------------------------------------------------
# choosing inputs: pixels whose answer float32 cannot decide
# ------------------------------------------------------------------------------------------------------------------
# The L1 terms' gradients are signs of differences of COMPUTED values (clamped Lab, HSV cone) and pass clamp gates.  Where such
# a difference is not 0 but below the rounding of the values themselves, its sign belongs to whoever rounds: `ambiguous` above
# finds the pixels where the ORACLE's float32 falls the other way, but a second float32 evaluation (the kernel's: hardware
# sin / cos, fused multiply-adds) may fall differently where the oracle's happened to agree with float64 -- on the k/255 grid
# with the prediction a few steps from the target, two cone coordinates 1.3e-8 apart turned up within 8 000 pixels.  Such a
# pixel tests nothing: both signs are right.  These helpers find them FROM FLOAT64 ALONE so that a test can leave them out of
# its inputs (never out of its comparison).  KINK_EPS is four times the 1e-6 the forward tests hold these values to.
KINK_EPS = 4e-6


def _terms(pred, tgt, mask, dtype=torch.float64):
    m = full_mask(mask, pred).to(dtype)
    p, t = pred.to(dtype) * m, tgt.to(dtype) * m
    return p, t, O.rgb2lab(p), O.rgb2lab(t), O._hsv_cone(p), O._hsv_cone(t)


def undecidable_signs(pred, tgt, mask):
    """[B,H,W] bool: a live pixel with pred != target where a clamped-Lab or cone difference is within KINK_EPS of 0, or where
    an a / b value of the prediction is within KINK_EPS of its clamp's ends.  A difference of exactly 0 is decided only where
    it is 0 by construction (both sides clamped to one end, two greys' chroma, equal maxima): 0 in float64 AND in float32 --
    not where float64 alone happens to cancel (two hues mirrored about 3/4 have the same sine)."""
    p, t, lab_p, lab_t, cone_p, cone_t = _terms(pred, tgt, mask)
    _, _, lab_p32, lab_t32, cone_p32, cone_t32 = _terms(pred, tgt, mask, torch.float32)
    d = torch.cat((lab_p.clamp(0, 1) - lab_t.clamp(0, 1), cone_p - cone_t), 1).abs()
    d32 = torch.cat((lab_p32.clamp(0, 1) - lab_t32.clamp(0, 1), cone_p32 - cone_t32), 1).abs()
    near = ((d < KINK_EPS) & ~((d == 0) & (d32 == 0))).any(1)
    ab = lab_p[:, 1:]
    near |= ((ab.abs() < KINK_EPS) | ((ab - 1).abs() < KINK_EPS)).any(1)
    return near & (p != t).any(1)


def undecidable_L_gate(pred, tgt, mask):
    """[B,H,W] bool: the prediction's L is within KINK_EPS of an end of model.py:55's clamp -- white, above all -- and the
    pixel is not BLACK (L = 0 exactly in every precision, where the reference's gate passes: that case is wanted)."""
    p, _, lab_p, _, _, _ = _terms(pred, tgt, mask)
    L = lab_p[:, 0]
    return ((L.abs() < KINK_EPS) | ((L - 1).abs() < KINK_EPS)) & (p != 0).any(1)


def decidable_inputs(pred, tgt, mask, g_Lp=None):
    """-> pred, g_Lp with the undecidable pixels taken out of the INPUTS: there the prediction becomes the target (every
    difference exactly 0, whatever the precision), and g_Lp is 0 where the L gate is undecidable.  Typically 0 to 0.1 % of
    the pixels; the comparison then runs over every pixel."""
    pred = torch.where(undecidable_signs(pred, tgt, mask)[:, None], tgt, pred)
    if g_Lp is not None:
        g_Lp = torch.where(undecidable_L_gate(pred, tgt, mask)[:, None], torch.zeros(()), g_Lp)
    return pred, g_Lp


def criterion_reference(pred, tgt, mask, label=""):
    """The whole criterion, model.py:111-116, with the MS-SSIM term as the reference builds it (window 11 on the clamped L
    planes, one channel), through the oracle in float64 and float32; the MS-SSIM share of a pixel's gradient gets
    msssim_allowance on top of tol(px)."""
    term = lambda Lp, Lt: 2.0 * (1.0 - O.msssim(Lp, Lt, 11, 1)).mean()  # noqa: E731  (10 * ssim_loss / 5)
    allow = msssim_allowance(pred, tgt, mask, term)
    return loss_gradient_reference(pred, tgt, mask, (0.2, 0.2, 0.2, 0.2), extra=term, allow=allow, label=label)
