"""GPU: the training criterion's kernels -- loss_terms_kernel, layer_loss_kernel, loss_terms_bwd_kernel, msssim_level_kernel
and msssim_grad_kernel -- held to float64 autograd through the oracle, pixel by pixel (tests/criterion_check.py), at the
shapes where each kernel takes another path, under every mask form, and under cotangents no module ever produces."""
import numpy as np
import pytest
import torch

import criterion_check as CC
import curl_oracle as O

pytestmark = pytest.mark.gpu

W_TERMS = (1.3, 0.7, 2.0, 0.5)  # rgb, cosine, lab, hsv
# [B,H,W] of [B,3,H,W]: 256 pixels (float4: 1024) per block; float4 needs H*W % 4 == 0 and 16-byte aligned planes
BWD_SHAPES = [(1, 1, 1),      # scalar, one lane
              (2, 7, 9),      # scalar, under one block
              (1, 37, 53),    # scalar, 8 blocks and a tail (1961 = 7 * 256 + 169)
              (2, 4, 1028)]   # float4: 1028 quads = 5 blocks, the last with 4 lanes
FWD_SHAPES = BWD_SHAPES + [(1, 229, 229),   # scalar, 205 blocks: loss_terms_final_kernel's 204-phase walk wraps
                           (1, 460, 460)]   # float4, 207 blocks
CONTENTS = ["uniform", "near_target_clamped", "grid8", "equal_and_black", "golden"]
MASKS = ["none", "bool", "binary_float", "fractional_float"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from curl_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def note(*a):
    print("CRIT", *a)  # (pytest -s: the figures DESIGN.md tabulates)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def image_pair(content, shape, golden, seed=0):
    """pred, target [B,3,H,W] float32 on the CPU."""
    B, H, W = shape
    n = B * H * W
    g = torch.Generator().manual_seed(1000 + seed + 7 * CONTENTS.index(content) + n)
    if content == "uniform":
        pred, tgt = torch.rand(3, n, generator=g), torch.rand(3, n, generator=g)
    elif content == "near_target_clamped":
        tgt = torch.rand(3, n, generator=g)
        pred = (tgt + 0.08 * torch.randn(3, n, generator=g)).clamp(0, 1)
    elif content == "grid8":  # both on the k/255 grid, the prediction within 3 steps of the target (equal values included)
        k = torch.randint(0, 256, (3, n), generator=g)
        d = torch.randint(-3, 4, (3, n), generator=g)
        # (one nonzero step shared by all three channels moves a colour along the grey axis: chroma and hue stay, the two cones
        # differ by rounding alone and the sign of that difference is float32's to decide -- 2 % of the pixels; the third
        # channel steps one further or back instead, so that criterion_check.decidable_inputs has little left to take out)
        shared = (d[0] == d[1]) & (d[1] == d[2]) & (d[0] != 0)
        d[2] = torch.where(shared, torch.where(d[2] < 3, d[2] + 1, d[2] - 1), d[2])
        tgt = k.float() / 255.0
        pred = (k + d).clamp(0, 255).float() / 255.0
    else:
        if content == "equal_and_black":
            from test_loss import equal_and_black_case
            p, t = equal_and_black_case()[:2]
            p, t = p[0, :, 0], t[0, :, 0]
        else:  # the golden pair: values outside [0, 1]
            gl = golden("loss")
            p = torch.from_numpy(gl["pred"]).permute(1, 0, 2, 3).reshape(3, -1)
            t = torch.from_numpy(gl["target"]).permute(1, 0, 2, 3).reshape(3, -1)
        idx = (torch.arange(n) + (0 if content == "equal_and_black" else 10)) % p.shape[1]  # (golden's first ten pixels have pred == target)
        pred, tgt = p[:, idx], t[:, idx]
    to_img = lambda x: x.reshape(3, B, H, W).permute(1, 0, 2, 3).contiguous()  # noqa: E731
    return to_img(pred), to_img(tgt)


def make_mask(kind, shape, seed=0):
    B, H, W = shape
    g = torch.Generator().manual_seed(77 + seed + B * H * W)
    u = torch.rand(B, 1, H, W, generator=g)
    u[:, 0, 0, 0] = 0.9  # (every image keeps a live pixel: the terms divide by the mask's sum)
    if kind == "none":
        return None
    if kind == "bool":
        return u > 0.25
    if kind == "binary_float":
        return (u > 0.25).float()
    return torch.where(u > 0.25, 0.02 + 0.96 * u, torch.zeros(()))  # strictly inside (0, 1), with exact zeros


def to_dev(t, dev):
    return None if t is None else t.to(dev)


def offset_by_one_float(t, dev):
    """The same values at a base address 4 bytes past a 16-byte boundary: float4 loads are off, the scalar kernel must run."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# ---------------------------------------------------------------------------------------------------------------
# loss backward
# ---------------------------------------------------------------------------------------------------------------
def backward_case(content, shape, mask_kind, with_gLp, golden, w=W_TERMS):
    """-> pred, tgt, mask, w4, g_Lp, reference (its input condition asserted): all on the CPU, nothing touches the GPU."""
    pred, tgt = image_pair(content, shape, golden)
    mask = make_mask(mask_kind, shape)
    w4 = CC.sum_weights(w, mask, pred)
    g_Lp = None
    if with_gLp:  # of the Lab weight's size, both signs: what the MS-SSIM branch sends back, and no smaller than the rest
        g = torch.Generator().manual_seed(5 + pred.numel())
        g_Lp = torch.randn(shape[0], 1, shape[1], shape[2], generator=g) * float(w4[2])
    pred, g_Lp = CC.decidable_inputs(pred, tgt, mask, g_Lp)  # (a white pixel's L gate, cones 1e-8 apart: criterion_check.py)
    ref = CC.loss_gradient_reference(pred, tgt, mask, w, g_Lp, label=f"{content} {shape} mask={mask_kind} gLp={with_gLp} w={w}")
    return pred, tgt, mask, w4, g_Lp, ref


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=str)
@pytest.mark.parametrize("content", CONTENTS)
def test_loss_backward_pixel_by_pixel(ops, dev, golden, content, shape):
    """ops.loss_terms_backward against float64 autograd under criterion_check's protocol: every mask form, with and
    without a gradient on the L plane.  Measured on the device (worst |got - g64| / tol over all of these; ambiguous share):
    see DESIGN.md 'The criterion, pixel by pixel'."""
    worst, share = 0.0, 0.0
    for mask_kind in MASKS:
        for with_gLp in (False, True):
            pred, tgt, mask, w4, g_Lp, ref = backward_case(content, shape, mask_kind, with_gLp, golden)
            got = ops.loss_terms_backward(pred.to(dev), tgt.to(dev), to_dev(mask, dev), w4.to(dev), to_dev(g_Lp, dev))
            worst, share = max(worst, ref.check(got)), max(share, ref.ambiguous_share)
    note(f"loss_bwd {content} {shape}: worst/tol {worst:.3f} ambiguous {share:.3%}")


@pytest.mark.parametrize("content", CONTENTS)
def test_loss_backward_each_term_alone(ops, dev, golden, content):
    """One weight at a time, so that no term hides behind the cosine's (whose gradient at a dark prediction is the largest
    by orders of magnitude): S and every tolerance are then that term's own."""
    worst = 0.0
    for k in range(4):
        w = tuple(W_TERMS[i] if i == k else 0.0 for i in range(4))
        for mask_kind in ("none", "fractional_float"):
            pred, tgt, mask, w4, g_Lp, ref = backward_case(content, (2, 7, 9), mask_kind, False, golden, w)
            got = ops.loss_terms_backward(pred.to(dev), tgt.to(dev), to_dev(mask, dev), w4.to(dev))
            worst = max(worst, ref.check(got))
    # ... and the L plane's cotangent alone
    pred, tgt = image_pair(content, (2, 7, 9), golden)
    g_Lp = torch.randn(2, 1, 7, 9, generator=torch.Generator().manual_seed(3))
    pred, g_Lp = CC.decidable_inputs(pred, tgt, None, g_Lp)
    ref = CC.loss_gradient_reference(pred, tgt, None, (0.0, 0.0, 0.0, 0.0), g_Lp, label=f"{content} g_Lp alone")
    got = ops.loss_terms_backward(pred.to(dev), tgt.to(dev), None, torch.zeros(4, device=dev), g_Lp.to(dev))
    worst = max(worst, ref.check(got))
    note(f"loss_bwd one term at a time {content}: worst/tol {worst:.3f}")


@pytest.mark.parametrize("which", ["pred", "target", "mask", "grad_L_pred"])
def test_loss_backward_base_pointer_offset_by_one_float(ops, dev, golden, which):
    """(2, 4, 1028) is the float4 shape; with one operand's base 4 bytes off a 16-byte boundary the scalar kernel must take
    it (planes_vec4).  Same protocol, and the same bits as the aligned call: both kernels run one per-pixel function."""
    pred, tgt, mask, w4, g_Lp, ref = backward_case("near_target_clamped", (2, 4, 1028), "fractional_float", True, golden)
    args = {"pred": pred.to(dev), "target": tgt.to(dev), "mask": mask.to(dev), "grad_L_pred": g_Lp.to(dev)}
    aligned = ops.loss_terms_backward(args["pred"], args["target"], args["mask"], w4.to(dev), args["grad_L_pred"])
    args[which] = offset_by_one_float(args[which], dev)
    got = ops.loss_terms_backward(args["pred"], args["target"], args["mask"], w4.to(dev), args["grad_L_pred"])
    ref.check(got)
    ref.check(aligned)


# ---------------------------------------------------------------------------------------------------------------
# the weight domain of the L1 pullbacks
# ---------------------------------------------------------------------------------------------------------------
DOMAIN_WEIGHTS = [0.0, 1e-30, 1e-15, 1.0, 2.0 ** 27, 2.0 ** 28, 2.0 ** 30, 1e30, -1.0, -(2.0 ** 30)]


@pytest.mark.parametrize("shape", [(2, 4, 1028), (1, 37, 53)], ids=["float4", "scalar"])
@pytest.mark.parametrize("w", DOMAIN_WEIGHTS, ids=lambda w: f"{w:g}")
def test_l1_pullback_is_exact_over_the_weight_domain(ops, dev, shape, w):
    """Weights (w, 0, 0, 0) and a binary mask: the result is exactly w * sign(pred - target) * mask -- 0, not NaN, at every
    masked-out pixel and wherever pred == target (the differences there are 0, and 0 * (2^100 w) was NaN from |w| = 2^28
    when that product overflowed: curl_math_loss.h signw_of saturates it).  The weights reach the kernel on the device, so
    no host check can stand in for this.  1e30 is inside the exact range (|w| <= 2^101 for normal differences, which
    differences of multiples of 2^-24 are), so bit equality is asked there too."""
    B, H, W = shape
    g = torch.Generator().manual_seed(31 + H)
    pred, tgt = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    eq = torch.rand(B, 1, H, W, generator=g) < 0.2
    pred = torch.where(eq, tgt, pred)                    # pred == target: all three channels, ...
    pred[:, 1] = torch.where(torch.rand(B, H, W, generator=g) < 0.1, tgt[:, 1], pred[:, 1])  # ... and one channel alone
    black = torch.rand(B, 1, H, W, generator=g) < 0.05
    pred = torch.where(black, torch.zeros(()), pred)     # black predictions
    mask = torch.rand(B, 1, H, W, generator=g) > 0.3
    assert bool((~mask).any()) and bool((eq & mask).any()) and bool((black & mask).any())
    wt = torch.tensor(w, dtype=torch.float32)
    for m in (mask, mask.float()):
        mf = m.float()
        want = wt * torch.sign(pred * mf - tgt * mf) * mf
        got = ops.loss_terms_backward(pred.to(dev), tgt.to(dev), m.to(dev), torch.tensor([w, 0.0, 0.0, 0.0]).to(dev)).cpu()
        assert not bool(torch.isnan(got).any()), (w, m.dtype, int(torch.isnan(got).sum()), "NaN")
        assert bool(torch.isfinite(got).all())
        # bit for bit (adding +0.0 folds -0 into +0, which compare equal anyway and carry no gradient)
        assert torch.equal((got + 0.0).view(torch.int32), (want + 0.0).view(torch.int32)), (w, m.dtype, float((got - want).abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# loss forward
# ---------------------------------------------------------------------------------------------------------------
def tile_to(x, shape, period):
    """x [1,C,1,period] repeated along the flattened pixels of one [1,C,H,W] image (H * W a multiple of `period`)."""
    B, H, W = shape
    assert B == 1 and (H * W) % period == 0
    idx = torch.arange(H * W) % period
    return x.reshape(x.shape[1], period)[:, idx].reshape(1, x.shape[1], H, W).contiguous()


def normalised(s, n, n_zero):
    """tests/test_loss.py terms_from_sums on sums [5] -- with model.py:98's logical_not counted as such (a fractional mask's
    zeros are not n - sum) -- and the mask's mean beside the four terms."""
    unmasked = 3.0 * s[4]
    return torch.stack((s[0] / unmasked, 1.0 - s[1] / n - n_zero / n, s[2] / unmasked, s[3] / unmasked, s[4] / n))


def check_forward(sums, Lp, Lt, pred, tgt, mask, label, period=None):
    """Device sums [B,5] (float64) and L planes against the oracle in float64 ON `pred` (for the fused forward: the prediction
    the kernel itself wrote, so that the layer's own error -- held elsewhere -- is not counted against the loss terms).
    The five sums normalised as terms_from_sums does, per image (a mix-up of two images' partial sums leaves the batch totals
    alone) and over the batch: within 3e-6; the L planes within 1e-6 at every pixel -- the golden test's two figures.
    period: the image repeats every `period` pixels (tile_to): the oracle then runs on one period -- every normalised term of
    the whole image equals that of one period -- and 200 000 pixels cost it nothing."""
    B, _, H, W = pred.shape
    n = H * W
    if period is not None:
        cut = lambda x: None if x is None else x.reshape(1, x.shape[1], 1, n)[..., :period]  # noqa: E731
        for x in (pred, tgt) + (() if mask is None else (mask,)):
            assert torch.equal(x, tile_to(cut(x), (B, H, W), period)), (label, "the input does not repeat")
        ref_pred, ref_tgt, ref_mask, reps = cut(pred), cut(tgt), cut(mask), n // period
    else:
        ref_pred, ref_tgt, ref_mask, reps = pred, tgt, mask, 1
    m64 = CC.full_mask(ref_mask, ref_pred)
    want, got_sums = [], sums.cpu()
    worst_L = 0.0
    for b in range(B):
        mm = m64[b:b + 1]
        rgb, cosine, lab, hsv, Lp64, Lt64 = O.curl_loss_terms(ref_pred[b:b + 1].double(), ref_tgt[b:b + 1].double(), mm)
        k, M, n_zero = float(mm.numel()), mm.sum(), float((mm == 0).sum())
        # the float64 sums behind the oracle's normalised terms, for `reps` periods
        want.append(torch.stack((rgb * 3 * M, (1.0 - cosine) * k - n_zero, lab * 3 * M, hsv * 3 * M, M)) * reps)
        if Lp is not None:
            for plane, ref in ((Lp, Lp64), (Lt, Lt64)):
                ref = ref if period is None else tile_to(ref, (B, H, W), period)
                worst_L = max(worst_L, float((plane[b:b + 1].cpu().double() - ref).abs().max()))
            assert worst_L <= 1e-6, (label, b, worst_L)
    want = torch.stack(want)
    n_zero = (CC.full_mask(mask, pred) == 0).sum((1, 2, 3)).double()
    worst = 0.0
    for sel in [slice(b, b + 1) for b in range(B)] + ([slice(0, B)] if B > 1 else []):
        k = float(n * (sel.stop - sel.start))
        d = (normalised(got_sums[sel].sum(0), k, n_zero[sel].sum()) - normalised(want[sel].sum(0), k, n_zero[sel].sum())).abs()
        worst = max(worst, float(d.max()))
        assert float(d.max()) <= 3e-6, (label, sel, d.tolist())
    return worst, worst_L


def forward_inputs(content, mask_kind, shape, golden, period):
    if period is None:
        pred, tgt = image_pair(content, shape, golden)
        return pred, tgt, make_mask(mask_kind, shape)
    pred, tgt = image_pair(content, (1, 1, period), golden)
    mask = make_mask(mask_kind, (1, 1, period))
    return tile_to(pred, shape, period), tile_to(tgt, shape, period), None if mask is None else tile_to(mask, shape, period)


# (content, mask) pairs: every mask form on two contents, the fractional one on the rest; the two large shapes -- there for
# loss_terms_final_kernel's walk over more than 204 block partials -- repeat one period of pixels that divides H * W and
# not the block (229 against 256 pixels, 2116 against 1024)
FWD_CASES = [(c, m) for c in ("uniform", "golden") for m in MASKS] + [(c, "fractional_float") for c in ("near_target_clamped", "grid8", "equal_and_black")]
FWD_PERIOD = {(1, 229, 229): 229, (1, 460, 460): 2116}


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=str)
def test_loss_forward_against_float64(ops, dev, golden, shape):
    """ops.loss_term_sums against the float64 oracle (check_forward); want_L=False gives the same sums bit for bit."""
    period = FWD_PERIOD.get(shape)
    worst = [0.0, 0.0]
    for content, mask_kind in (FWD_CASES if period is None else [("uniform", "fractional_float"), ("golden", "bool"), ("grid8", "none")]):
        pred, tgt, mask = forward_inputs(content, mask_kind, shape, golden, period)
        sums, Lp, Lt = ops.loss_term_sums(pred.to(dev), tgt.to(dev), to_dev(mask, dev))
        t, l = check_forward(sums, Lp, Lt, pred, tgt, mask, (content, shape, mask_kind), period)
        worst = [max(worst[0], t), max(worst[1], l)]
        sums2, none_p, none_t = ops.loss_term_sums(pred.to(dev), tgt.to(dev), to_dev(mask, dev), want_L=False)
        assert none_p is None and none_t is None and torch.equal(sums, sums2)
    note(f"loss_fwd {shape}: worst term error {worst[0]:.2e} worst L error {worst[1]:.2e}")


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=str)
def test_layer_loss_forward_against_float64(ops, dev, golden, shape):
    """ops.layer_loss_forward (layer and loss terms in one kernel): its sums and L planes against the float64 oracle evaluated
    on the prediction it wrote -- not against ops.loss_term_sums, which shares its device functions."""
    B, H, W = shape
    period = FWD_PERIOD.get(shape)
    g = torch.Generator().manual_seed(11 + H)
    L, R, Hk = (torch.randn(B, k, generator=g) * 0.1 for k in (48, 48, 64))
    worst = [0.0, 0.0]
    cases = [("uniform", m) for m in MASKS] + [("grid8", "fractional_float"), ("equal_and_black", "bool")]
    for content, mask_kind in (cases if period is None else [("uniform", "bool"), ("grid8", "fractional_float")]):
        img, tgt, mask = forward_inputs(content, mask_kind, shape, golden, period)
        out, reg, sums, Lp, Lt, ws = ops.layer_loss_forward(img.to(dev), to_dev(mask, dev), L.to(dev), R.to(dev), Hk.to(dev), tgt.to(dev))
        t, l = check_forward(sums, Lp, Lt, out.cpu(), tgt, mask, (content, shape, mask_kind), period)
        worst = [max(worst[0], t), max(worst[1], l)]
        sums2 = ops.layer_loss_forward(img.to(dev), to_dev(mask, dev), L.to(dev), R.to(dev), Hk.to(dev), tgt.to(dev), want_L=False)[2]
        assert torch.equal(sums, sums2)
    note(f"layer_loss_fwd {shape}: worst term error {worst[0]:.2e} worst L error {worst[1]:.2e}")


# ---------------------------------------------------------------------------------------------------------------
# MS-SSIM statistics and their backward under independent cotangents
# ---------------------------------------------------------------------------------------------------------------
SSIM_SHAPES = [(1, 1, 32, 32),    # one tile at every level
               (1, 1, 33, 65),    # 2 x 3 tiles; odd sizes whose pooling drops a row / a column
               (2, 3, 70, 97),    # C > 1; odd at levels 1 and 2
               (1, 1, 129, 66)]   # 5 x 3 tiles
SSIM_CONTENTS = ["noise", "near_identical", "flat_saturated"]


def ssim_pair(content, shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(200 + H + W + SSIM_CONTENTS.index(content))
    a = torch.rand(*shape, generator=g)
    if content == "noise":
        b = a + 0.1 * torch.randn(*shape, generator=g)
    elif content == "near_identical":
        b = a + 0.01 * torch.randn(*shape, generator=g)
    else:
        a[:, :, H // 8:H // 2, W // 8:(5 * W) // 8] = 1.0
        a[:, :, (5 * H) // 8:, W // 16:W // 2] = 0.0
        b = (a + 0.05 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return a, b


@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=str)
@pytest.mark.parametrize("window", [1, 3, 5, 7, 9, 11])
def test_msssim_stats_and_backward_under_independent_cotangents(ops, dev, window, shape):
    """ops.msssim_stats / ops.msssim_stats_backward called directly with g_ssims, g_mcs = randn(B, 5): every level's SSIM
    AND contrast cotangent is live (through MSSSIMMetric four of the former and one of the latter are exactly 0).  Reference:
    float64 autograd through curl_oracle.ssim_and_cs level by level; bounds from the oracle's own float32 deviation r32
    (criterion_check.MsssimReference).  Measured got / r32 per window and shape: DESIGN.md."""
    B = shape[0]
    for content in SSIM_CONTENTS:
        a, b = ssim_pair(content, shape)
        ref = CC.MsssimReference(a, b, window)
        g = torch.Generator().manual_seed(window + shape[2])
        g_ssims, g_mcs = torch.randn(B, 5, generator=g), torch.randn(B, 5, generator=g)
        g64, r32, bound, scale = ref.gradient(g_ssims, g_mcs)
        ssims, mcs = ops.msssim_stats(a.to(dev), b.to(dev), window)
        d_stats = (torch.stack((ssims.cpu(), mcs.cpu())).double() - ref.stats64).abs()
        got = ops.msssim_stats_backward(a.to(dev), b.to(dev), g_ssims.to(dev), g_mcs.to(dev), window).cpu().double()
        d = (got - g64).abs()
        note(f"msssim w={window} {shape} {content}: grad err {float(d.max()):.2e} r32 {r32:.2e} got/r32 {float(d.max()) / max(r32, 1e-300):.2f} "
             f"scale {scale:.2e} | stats err {float(d_stats.max()):.2e} r32 {ref.r32_stats:.2e}")
        assert float(d_stats.max()) <= ref.stats_bound, (content, "statistics", d_stats.tolist(), ref.stats_bound)
        assert bool(torch.isfinite(got).all())
        if not float(d.max()) <= bound:
            i = [int(v) for v in (d == d.max()).nonzero()[0]]
            raise AssertionError(f"{content}: |got - g64| = {float(d.max()):.3e} at (b, c, y, x) = {i} > min(4 r32, 1e-3 scale) = {bound:.3e} "
                                 f"(r32 {r32:.3e}, scale {scale:.3e})")


def test_msssim_backward_one_cotangent_at_a_time(ops, dev):
    """One-hot cotangents per (image, level, kind): a level or image mix-up in `g_ssim[b * levels + level]` is named, and the
    other image's gradient is exactly 0."""
    shape, window = (2, 3, 70, 97), 7
    a, b = ssim_pair("noise", shape)
    ref = CC.MsssimReference(a, b, window)
    ad, bd = a.to(dev), b.to(dev)
    for kind in ("ssim", "cs"):
        for img in range(shape[0]):
            for level in range(CC.MSSSIM_LEVELS):
                hot = torch.zeros(shape[0], 5)
                hot[img, level] = 1.0
                gs, gc = (hot, torch.zeros_like(hot)) if kind == "ssim" else (torch.zeros_like(hot), hot)
                g64, r32, bound, scale = ref.gradient(gs, gc)
                got = ops.msssim_stats_backward(ad, bd, gs.to(dev), gc.to(dev), window).cpu().double()
                err = float((got - g64).abs().max())
                assert err <= bound, (kind, img, level, err, bound, r32, scale)
                assert not bool(got[1 - img].any()), (kind, img, level, "the other image's gradient is not 0")


# ---------------------------------------------------------------------------------------------------------------
# the whole criterion
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["bool", "fractional_float"])
def test_whole_criterion_pixel_by_pixel(dev, mask_kind):
    """model.CURLLoss(ssim_window_size=5) as test_curl_loss_with_msssim_vs_oracle builds it, at a size that is odd at three
    pyramid levels, value and gradient against the float64 oracle."""
    from curl_amd import model
    shape = (2, 69, 98)
    g = torch.Generator().manual_seed(21)
    tgt = torch.rand(2, 3, 69, 98, generator=g)
    pred = (tgt + 0.08 * torch.randn(2, 3, 69, 98, generator=g)).clamp(0, 1)
    mask = make_mask(mask_kind, shape)
    pred, _ = CC.decidable_inputs(pred, tgt, mask)
    ref = CC.criterion_reference(pred, tgt, mask, f"whole criterion, mask={mask_kind}")
    crit = model.CURLLoss(ssim_window_size=5).to(dev)
    p = pred.to(dev).requires_grad_(True)
    loss = crit(p, tgt.to(dev), mask.to(dev))
    loss.backward()
    p64 = pred.double()
    m64 = mask if mask.dtype == torch.bool else mask.double()
    r = O.curl_loss_terms(p64, tgt.double(), m64)
    want = O.curl_loss(p64, tgt.double(), m64, (1.0 - O.msssim(r[4], r[5], 11, 1)).mean())
    assert abs(float(loss) - float(want)) <= 5e-6, (float(loss), float(want))
    worst = ref.check(p.grad)
    note(f"whole criterion {mask_kind}: worst/tol {worst:.3f} ambiguous {ref.ambiguous_share:.3%} "
         f"(S {ref.S:.2e}, MS-SSIM allowance up to {float((ref.tol - CC.REL * ref.g64.abs().amax(1).clamp(min=ref.S)).max()):.2e})")
