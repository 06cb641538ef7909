"""GPU: the fused backward kernels (through the C ABI and through torch.autograd) against the golden
gradients (autograd through the reference's primitives) and autograd through the oracle."""
import os

import numpy as np
import pytest
import torch

import criterion_check as CC

pytestmark = pytest.mark.gpu


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


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rel(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


@pytest.mark.parametrize("sig,tol_knots,tol_img", [("s01", 5e-6, 2e-5), ("s05", 1e-3, 1e-3)])
def test_golden_gradients(ops, dev, golden, sig, tol_knots, tol_img):
    """Golden gradients = float32 autograd through the REFERENCE's primitives (tests/golden/make_golden.py).  At sigma 0.1 the
    host twin of this arithmetic is within 5.8e-7 (knots) / 4.2e-6 (image, of the gradient scale) of them; the bars are that
    with room for the hardware transcendentals (round 3 asserted 2e-4 and only the 0.999 quantile of the image gradient).
    At sigma 0.5 the golden's own distance from the float64 evaluation is 5e-5 of the scale: the precise statement there is
    test_backward_parity_is_pinned_to_float64_autograd below."""
    c = golden("chain")
    args = [T(c[k], dev) for k in ("img",)]
    mask = T(c["mask_disk"], dev)
    L, R, H = (T(c[sig + k], dev) for k in ("_L", "_R", "_H"))
    w, wr = T(c[sig + "_grad_w"], dev), T(c[sig + "_grad_wr"], dev)
    for m in (mask, mask.float()):
        gi, gL, gR, gH = ops.curl_layer_backward(args[0], m, L, R, H, w, wr)
        assert rel(gL, c[sig + "_grad_L"]) <= tol_knots and rel(gR, c[sig + "_grad_R"]) <= tol_knots
        assert rel(gH, c[sig + "_grad_H"]) <= tol_knots
        d = np.abs(gi.cpu().numpy() - c[sig + "_grad_img"])
        scale = np.abs(c[sig + "_grad_img"]).max()
        assert d.max() <= tol_img * scale, (float(d.max()), float(scale))
        assert (gi.cpu().numpy()[:, :, ~c["mask_disk"][0, 0]] == 0).all()
    gi2, gL2, _, _ = ops.curl_layer_backward(args[0], mask, L, R, H, w, wr, need_grad_img=False)
    assert gi2 is None and torch.equal(gL2, gL)


@pytest.mark.parametrize("shape", [(1, 7, 5), (2, 33, 70), (3, 64, 64), (2, 250, 301), (1, 1000, 1500)])
def test_knot_gradients_alone_agree_with_the_full_backward(ops, dev, shape):
    """grad_img = NULL (the training step: the image is data, main.py:287) picks the kernel instantiation without RGB2LAB's
    pullback and without the gradient image's stores.  The knot gradients are the same arithmetic, but NOT guaranteed the
    same bits: hipcc contracts a*b+c into an fma depending on how many uses the product has, and the dead pullback changes
    the use counts (measured over these five shapes x three masks x with / without the workspace: 88 of 90 gradient tensors
    the same bits, two with one sum one ulp off -- 1.5e-5 of 210).  Asserted: each gradient tensor within 1e-6 of its largest entry
    (the float64-pinned bound of test_backward_parity_is_pinned_to_float64_autograd, which both variants meet, is 2e-5)."""
    B, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + H)
    img = torch.rand(B, 3, H, W, generator=g).to(dev)
    w = torch.randn(B, 3, H, W, generator=g).to(dev)
    wr = torch.randn(B, generator=g).to(dev)
    L, R, Hk = ((torch.randn(B, n, generator=g) * 0.3).to(dev) for n in (48, 48, 64))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    disk = (((yy - H / 2) ** 2 / (H / 2) ** 2 + (xx - W / 2) ** 2 / (W / 2) ** 2) <= 0.8)[None, None].expand(B, 1, H, W).contiguous().to(dev)
    soft = torch.rand(B, 1, H, W, generator=g).to(dev)
    n_same = n_all = 0
    for mask in (None, disk, soft):
        ws = ops.curl_layer_forward(img, mask, L, R, Hk, return_workspace=True)[2]
        for kw in ({}, {"workspace": ws}):
            full = ops.curl_layer_backward(img, mask, L, R, Hk, w, wr, **kw)
            only = ops.curl_layer_backward(img, mask, L, R, Hk, w, wr, need_grad_img=False, **kw)
            assert only[0] is None and full[0] is not None
            for a, b in zip(full[1:], only[1:]):
                assert torch.isfinite(b).all()
                assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max()), (shape, None if mask is None else mask.dtype)
                n_same += int(torch.equal(a, b))
                n_all += 1
    print(f"knot gradients, full vs knots-only backward {shape}: {n_same} of {n_all} tensors the same bits")


@pytest.mark.parametrize("shift", [-0.7, -0.3, 0.0])
def test_black_and_the_corners_of_the_colour_cube(ops, dev, shift):
    """tests/test_twin_bwd.py's statement on the device, through both kernel instantiations' arithmetic (bool and float32
    mask): black, near-black, greys, white, primaries, secondaries -- nothing excused, every colour within 1e-5 of the
    gradient scale of the FLOAT64 autograd, as the reference's own float32 autograd is.  (Until round 4 black was off by its
    whole chain gradient: L = 1.16 fy - 0.16 as one fma is -1.6e-9 there, the reference's is exactly 0, the clamp gate differs.)
    The colours are tiled to 4 x 1024 so that float4 lanes, whole wavefronts and several workgroups see them."""
    import curl_oracle as O
    from test_twin_bwd import STRUCTURED_COLOURS, structured_case
    n = len(STRUCTURED_COLOURS)
    reps = 4 * 1024 // n + 1
    for seed in (3, 4, 5):
        img, mask, L, R, Hk, w, wr = structured_case(seed, shift)
        g64 = O.layer_gradients(img, mask, L, R, Hk, w, wr)[0]
        tol = 1e-5 * max(1.0, float(g64.abs().max()))  # (hardware log2 / exp2: the host twin holds 5e-6; black was off by 1e-1)
        tile = lambda t: t.repeat(1, 1, 1, reps)[..., :4096].reshape(1, t.shape[1], 4, 1024).contiguous()  # noqa: E731
        for m in (tile(mask).bool(), tile(mask)):
            gi = ops.curl_layer_backward(tile(img).to(dev), m.to(dev), L.to(dev), R.to(dev), Hk.to(dev), tile(w).to(dev), wr.to(dev))[0]
            d = (gi.cpu().double() - tile(g64)).abs().amax(1).flatten()
            assert float(d.max()) <= tol, (shift, seed, m.dtype, (STRUCTURED_COLOURS[int(d.argmax()) % n] * 255).tolist(), float(d.max()))


def test_loss_backward_where_prediction_equals_target_and_at_black(ops, dev):
    """tests/test_loss.py's statement on the device: torch.sign(0) = 0 where prediction and target are the same bits, and the
    Lab clamp gate passes the gradient at a black prediction (an output the layer's own clamp saturated at 0)."""
    from test_loss import equal_and_black_case, oracle_loss_gradient
    pred, tgt, mask, n_same = equal_and_black_case()
    w = (1.3, 0.0, 2.0, 0.5)  # (cosine off: its reference gradient at black is ~1e6, test_loss.py)
    n = pred.shape[-1]
    reps = 4096 // n + 1
    tile = lambda t: t.repeat(1, 1, 1, reps)[..., :4096].reshape(1, t.shape[1], 4, 1024).contiguous()  # noqa: E731
    soft = torch.full_like(mask, 0.37)  # a float mask strictly inside (0, 1): pred * m - tgt * m must not become fma(pred, m, -(tgt m))
    for m in (mask.bool(), mask, soft):
        unmasked = 3.0 * float(m.sum())
        w4 = torch.tensor([w[0] / unmasked, -w[1] / n, w[2] / unmasked, w[3] / unmasked])
        g64 = oracle_loss_gradient(pred, tgt, m.float(), w, torch.float64)
        scale = float(g64.abs().max())
        got = ops.loss_terms_backward(tile(pred).to(dev), tile(tgt).to(dev), tile(m).to(dev), w4.to(dev))
        d = (got.cpu().double() - tile(g64)).abs().amax(1).flatten()
        assert float(d.max()) <= 1e-5 * scale, (m.dtype, int(d.argmax()) % n, float(d.max()), scale)
        same = got.cpu().flatten(2)[0, :, :n][:, :n_same]
        assert float(same.abs().max()) <= 1e-6 * scale


def _mosaic_8bit():
    """24 rows of each of tools/synth8.py's eight content bands (gradients, grey ramps, flat dark patches with exact zeros,
    tie palettes, photograph-like, saturated, dark photograph, checker), 256 columns: [1,3,192,256] on the k/255 grid."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth8
    import curl_oracle as O
    u8 = synth8.coherent_8bit_frames(1, 1000, 1500, seed=1)[0]
    rows = np.concatenate([np.arange(125 * k + 50, 125 * k + 74) for k in range(8)])
    return O.u8hwc_to_f32chw(np.ascontiguousarray(u8[rows][:, 200:456]))[None]


@pytest.mark.parametrize("case", ["random_s01", "random_s03", "coherent_8bit_dim_knots", "cube_slices_8bit_dim_knots", "fullsize_random_s01",
                                  "photograph_crop_dim_knots", "photograph_dark_dim_knots"])
def test_backward_parity_is_pinned_to_float64_autograd(ops, dev, case, golden):
    """the backward's parity pinned the way the forward's is.  Yardstick: FLOAT64 autograd through the
    oracle (the reference's arithmetic).  Per pixel,
        |d img_HIP - d img_64| <= max(2e-6 * G, 2e-6 * C(pixel)),     G = max |d img_64|,
    C = the float64 gradient's own rate of change with the input (curl_oracle.gradient_curvature): a float32 chain perturbs
    its intermediates by roundings worth ~1e-6 of input.  The EXCEPTION SET is identified, not averaged away: pixels where
    the float64 gradient JUMPS within +-1e-6 of the input (h * C > 1e-3 * G: a clamp gate, a threshold select or a channel
    tie of some intermediate within rounding distance) -- there float32 may legitimately take the other side; it is reported
    and must be tiny.  Knot gradients (sums over all pixels): <= 2e-5 of their scale at sigma 0.1 (the host twin: 8e-7).
    On the 8-bit mosaic -- exact ties, exact zeros, flat dark patches -- the subgradient conventions are exercised exactly AT
    the discontinuities (torch's clamp passes the gradient at the bounds, the hue terms' masks are constants): they must match.
    Sixteen slices of the 8-bit cube (1 M colours): the exception set is 14 colours -- black among them, where the gradient does
    jump (an input below 0 closes the Lab curve's clamp gate) but the reference is NOT ambiguous: its L is exactly 0 at black
    and the gate passes.  The criterion cannot tell the two apart, so black has tests of its own that excuse nothing
    (test_black_and_the_corners_of_the_colour_cube, the photograph_dark case below)."""
    import curl_oracle as O
    g = torch.Generator().manual_seed(7)
    if case == "cube_slices_8bit_dim_knots":
        # sixteen slices of the 8-bit colour cube: every (r, g) pair at b = 0, 17, ..., 255 -- 1 048 576 colours, every exact
        # r == g tie, black, white, every colour with a channel at 0 or 255
        r8, g8, b8 = torch.meshgrid(torch.arange(256), torch.arange(256), torch.arange(0, 256, 17), indexing="ij")
        img = (torch.stack((r8, g8, b8), 0).float() / 255).reshape(1, 3, 1024, 1024).contiguous()
        B, _, H, W = img.shape
        L, R, Hk = (torch.randn(B, n, generator=g) * 0.1 - 0.7 for n in (48, 48, 64))
        mask = torch.ones(B, 1, H, W, dtype=torch.bool)
        tol_knots = 2e-5
    elif case.startswith("photograph"):
        # the reference's own photographs (tests/golden/real8.npz: configs[0]'s 256x256 crop, and the dark 512x341 frame whose
        # forward needs the conditioned bound on 2 pixels), the unsaturated knots B, the crop under its disk mask
        real = golden("real8")
        key = "crop" if "crop" in case else "dark"
        img = O.u8hwc_to_f32chw(real[key + "_u8"])[None]
        B, _, H, W = img.shape
        L, R, Hk = (torch.from_numpy(real["B_" + k]) for k in "LRH")
        mask = torch.from_numpy(real["crop_disk"]) if key == "crop" else torch.ones(B, 1, H, W, dtype=torch.bool)
        tol_knots = 2e-5
    elif case == "coherent_8bit_dim_knots":
        img = _mosaic_8bit()
        B, _, H, W = img.shape
        # curves that halve their channel: model.py:170's clamp(img + residual) does not saturate, every pixel carries gradient
        L, R, Hk = (torch.randn(B, n, generator=g) * 0.1 - 0.7 for n in (48, 48, 64))
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        mask = ((((yy - H / 2) / (H / 2)) ** 2 + ((xx - W / 2) / (W / 2)) ** 2) < 0.9)[None, None]
        tol_knots = 2e-5
    else:
        # the full-size frame is where the exception set shows: ~15 gates per pixel x 1.5 M pixels within 1e-6 of one of them
        B, H, W = (1, 1000, 1500) if case == "fullsize_random_s01" else (2, 96, 128)
        sigma = 0.3 if case == "random_s03" else 0.1
        img = torch.rand(B, 3, H, W, generator=g)
        L, R, Hk = (torch.randn(B, n, generator=g) * sigma for n in (48, 48, 64))
        mask = torch.rand(B, 1, H, W, generator=g) > 0.1
        tol_knots = 2e-5 if sigma == 0.1 else 2e-4
    w = torch.randn(B, 3, H, W, generator=g)
    wr = torch.rand(B, generator=g)
    mf = mask.float()
    g64, gL64, gR64, gH64 = O.layer_gradients(img, mf, L, R, Hk, w, wr)
    assert float(g64.abs().max()) > 0.5 and float((g64.abs().amax(1) > 0).double().mean()) > 0.3   # not a saturated frame
    C = O.gradient_curvature(img, mf, L, R, Hk, w, g64=g64, h=1e-6)
    G = float(g64.abs().max())
    jump = 1e-6 * C > 1e-3 * G                       # a discontinuity of the float64 gradient within +-1e-6 of the input
    # Knot gradients are sums over all pixels, and one gate taken on the other side moves them by that pixel's whole
    # contribution (on the cube slices: (79, 238, 34) alone moves d L by 1e-2 of its scale; on the full-size frame the
    # reference's OWN float32 autograd flips one of the 17).  The statement that does not depend on which side of a kink a
    # rounding falls: with the exception set masked out of both evaluations, the knot gradients agree to tol_knots.
    mask_ex, want_knots, g32 = mask, (gL64, gR64, gH64), None
    if bool(jump.any()):
        mask_ex = mask & ~jump[:, None]
        want_knots = O.layer_gradients(img, mask_ex.float(), L, R, Hk, w, wr)[1:]
    for m in (mask, mf):
        gi, gL, gR, gH = ops.curl_layer_backward(img.to(dev), m.to(dev), L.to(dev), R.to(dev), Hk.to(dev), w.to(dev), wr.to(dev))
        kn = (gL, gR, gH)
        if bool(jump.any()):
            mx = mask_ex if m.dtype == torch.bool else mask_ex.float()
            kn = ops.curl_layer_backward(img.to(dev), mx.to(dev), L.to(dev), R.to(dev), Hk.to(dev), w.to(dev), wr.to(dev),
                                         need_grad_img=False)[1:]
        else:  # ... and the kernel instantiation that computes the knot gradients alone, against the same float64 figures
            kn = kn + tuple(ops.curl_layer_backward(img.to(dev), m.to(dev), L.to(dev), R.to(dev), Hk.to(dev), w.to(dev), wr.to(dev),
                                                    need_grad_img=False)[1:])
        for got, want in zip(kn, tuple(want_knots) * 2):
            assert rel(got, want) <= tol_knots, (case, rel(got, want), tol_knots)
        d = (gi.cpu().double() - g64).abs().amax(1)
        bound = torch.clamp(2e-6 * C, min=2e-6 * G)
        over = (d > bound) & ~jump
        print(f"backward parity {case} mask={m.dtype}: max |err| {float(d.max()):.2e} of G {G:.2f}; max err/bound "
              f"{float((d / bound)[~jump].max()):.2f}; exception set (gradient jump within 1e-6): {int(jump.sum())} of {jump.numel()} px")
        assert int(over.sum()) == 0, (case, int(over.sum()), float((d / bound)[~jump].max()))
        if case == "photograph_dark_dim_knots":
            # 2 194 of this frame's pixels are pure black, and black IS a discontinuity of the reference's gradient (the
            # docstring's L = 116 * (4/29) - 16): the exception set is exactly black pixels, nothing else
            assert bool((img.permute(0, 2, 3, 1)[jump] == 0).all()) and int(jump.sum()) <= int((img.amax(1) == 0).sum())
            # ... and the kernel is on the reference's side of it on every one (float32 and float64 autograd agree there:
            # L is exactly 0 resp. >= 0 and torch.clamp's gate passes; test_black_and_the_corners_of_the_colour_cube)
            assert float(d[jump].max()) <= 5e-6 * G, float(d[jump].max())
        else:
            assert int(jump.sum()) <= 1e-3 * jump.numel()
        assert float(d[jump].max() if bool(jump.any()) else 0.0) <= 2.0 * G    # even there: a gate flipped, nothing worse
        # The exception set excuses a pixel only while the REFERENCE is of two minds about it.  Where its float32 and its
        # float64 autograd agree (the gate is not a coin toss of its arithmetic: black is the example, L is exactly 0 there) a
        # gate-sized error of the kernel is a flip of its own; a true knife edge may produce one now and then (the cube slices:
        # (79, 238, 34)), a systematic one produces thousands (the `dark` photograph's 2 169 black pixels, round 4).
        if bool(jump.any()):
            if g32 is None:
                g32 = O.layer_gradients(img, mf, L, R, Hk, w, wr, dtype=torch.float32)[0].double()
            unambiguous = (g32 - g64).abs().amax(1) <= 1e-4 * G
            lone = (d > 1e-3 * G) & unambiguous
            print(f"   exception pixels where the reference's float32 and float64 agree and the kernel alone is off: {int(lone.sum())}")
            assert int(lone.sum()) <= max(3, int(1e-5 * lone.numel())), int(lone.sum())
        assert (gi.cpu()[:, :, ~mask[0, 0]] == 0).all() if case == "coherent_8bit_dim_knots" else True


@pytest.mark.parametrize("shape", [(2, 24, 32), (1, 7, 9), (3, 33, 65)])
def test_autograd_matches_oracle(dev, shape):
    import curl_oracle as O
    from curl_amd import model
    B, H, W = shape
    g = torch.Generator().manual_seed(B * 100 + H)
    img = torch.rand(B, 3, H, W, generator=g)
    mask = torch.rand(B, 1, H, W, generator=g) > 0.2
    knots = torch.randn(B, 170, generator=g) * 0.1  # a wider head than the layer consumes
    w = torch.randn(B, 3, H, W, generator=g)
    wr = torch.rand(B, generator=g)

    def run(layer_fn, device, mask_t):
        x = img.detach().clone().to(device).requires_grad_(True)
        k = knots.detach().clone().to(device).requires_grad_(True)
        L, R, Hk = k[:, :48], k[:, 50:98], k[:, 100:164]
        out, reg = layer_fn(x, mask_t.to(device), L, R, Hk)
        ((out * w.to(device)).sum() + (reg * wr.to(device)).sum()).backward()
        return x.grad, k.grad

    gx_ref, gk_ref = run(lambda x, m, L, R, Hk: O.curl_layer(x, m, L, R, Hk), torch.device("cpu"), mask.float())
    layer = model.CURLLayer().to(dev)
    gx, gk = run(layer, dev, mask)
    assert rel(gk, gk_ref) <= 1e-3
    d = (gx.cpu() - gx_ref).abs()
    assert float(torch.quantile(d.flatten(), 0.995)) <= 3e-4 * float(gx_ref.abs().max())
    assert (gk.cpu()[:, 48:50] == 0).all() and (gk.cpu()[:, 164:] == 0).all()  # unused head outputs get zero grad


def test_backward_is_reproducible_and_batch_independent(ops, dev):
    g = torch.Generator().manual_seed(9)
    B, H, W = 3, 64, 128
    img = torch.rand(B, 3, H, W, generator=g).to(dev)
    L, R, Hk = ((torch.randn(B, n, generator=g) * 0.1).to(dev) for n in (48, 48, 64))
    w = torch.randn(B, 3, H, W, generator=g).to(dev)
    a = ops.curl_layer_backward(img, None, L, R, Hk, w, None)
    b = ops.curl_layer_backward(img, None, L, R, Hk, w, None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)  # fixed-order reduction, no float atomics
    one = ops.curl_layer_backward(img[1:2], None, L[1:2], R[1:2], Hk[1:2], w[1:2], None)
    assert torch.equal(one[0][0], a[0][1]) and torch.equal(one[1][0], a[1][1]) and torch.equal(one[3][0], a[3][1])


def test_train_step_gcurlnet(dev):
    """Config-5 shape in miniature: encoder fwd/bwd on PyTorch-ROCm + fused HIP curve fwd/bwd, one Adam step."""
    from curl_amd import model
    torch.manual_seed(0)
    net = model.GCURLNet(backbone=model.CurveEncoder(160, width=0.25, num_features=128)).to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    img = torch.rand(4, 3, 64, 64, device=dev)
    gt = torch.rand(4, 3, 64, 64, device=dev)
    mask = torch.rand(4, 1, 64, 64, device=dev) > 0.1
    losses = []
    for _ in range(3):
        out, reg = net(img, mask)
        loss = ((out - gt).abs() * mask).mean() + 1e-6 * reg.mean()
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.backbone.classifier.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))


def test_curl_loss_terms_golden(dev, golden):
    """CURLLoss pointwise terms + gradient (model.py:89-109) vs values computed with the reference's colors.py."""
    from curl_amd import model
    g = golden("loss")
    tgt = T(g["target"], dev)
    wl = T(g["wl"], dev)
    w = g["weights"]
    for mk, m in (("bool", T(g["mask"], dev)), ("f32", T(g["mask"], dev).float())):
        pred = T(g["pred"], dev).requires_grad_(True)
        rgb, cosv, lab, hsv, Lp, Lt = model._LossTermsFn.apply(pred, tgt, m)
        for name, v in (("rgb", rgb), ("cos", cosv), ("lab", lab), ("hsv", hsv)):
            assert abs(float(v.detach()) - float(g[f"{mk}_{name}"])) <= 3e-6, (mk, name)
        assert (Lp.detach().cpu().numpy() - g[f"{mk}_Lp"]).__abs__().max() <= 1e-6
        assert (Lt.cpu().numpy() - g[f"{mk}_Lt"]).__abs__().max() <= 1e-6
        total = float(w[0]) * rgb + float(w[1]) * cosv + float(w[2]) * lab + float(w[3]) * hsv + (Lp * wl).sum() * 1e-3
        total.backward()
        # pixel by pixel against float64 autograd (criterion_check.py): the golden gradient's max, 4.05e4, is the cosine term at 106
        # black predictions; relative to it (as here until now) a gradient that is zero at every other pixel passed
        CC.loss_gradient_reference(torch.from_numpy(g["pred"]), torch.from_numpy(g["target"]), m.cpu(), [float(v) for v in w],
                                   torch.from_numpy(g["wl"]) * 1e-3, label=f"golden, {mk} mask").check(pred.grad)


def test_curl_loss_module_vs_oracle(dev):
    import curl_oracle as O
    from curl_amd import model
    g = torch.Generator().manual_seed(8)
    pred, tgt = torch.rand(3, 3, 40, 56, generator=g), torch.rand(3, 3, 40, 56, generator=g)
    mask = torch.rand(3, 1, 40, 56, generator=g) > 0.3
    pred, _ = CC.decidable_inputs(pred, tgt, mask)  # (2 to 7 pixels whose sign float32 cannot decide: criterion_check.py)
    want = O.curl_loss(pred, tgt, mask, torch.tensor(0.0))
    got = model.CURLLoss(msssim_layer=None)(pred.to(dev), tgt.to(dev), mask.to(dev))
    assert abs(float(got) - float(want)) <= 2e-6
    fake_ssim = lambda a, b: 1.0 - (a - b).abs().mean(dim=(1, 2, 3))  # noqa: E731  (stands in for MS-SSIM)
    p = pred.to(dev).requires_grad_(True)
    loss = model.CURLLoss(msssim_layer=fake_ssim)(p, tgt.to(dev), mask.to(dev))
    loss.backward()
    pc = pred.clone().requires_grad_(True)
    r = O.curl_loss_terms(pc, tgt, mask)
    ref = (r[0] + r[1] + r[2] + r[3] + 10 * (1.0 - fake_ssim(r[4], r[5])).mean()) / 5
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 2e-6
    extra = lambda Lp, Lt: 2.0 * (1.0 - fake_ssim(Lp, Lt)).mean()  # noqa: E731
    CC.loss_gradient_reference(pred, tgt, mask, (0.2, 0.2, 0.2, 0.2), extra=extra, label="module, stand-in MS-SSIM").check(p.grad)


def test_curl_loss_float_mask_strictly_inside_the_unit_interval(dev):
    """model.py:98's torch.logical_not(mask) counts the pixels whose mask is EXACTLY 0; under a float mask with fractional
    values that is not n - mask.sum() (round 4: the cosine term was off by the mask's mean)."""
    import curl_oracle as O
    from curl_amd import model
    g = torch.Generator().manual_seed(18)
    pred, tgt = torch.rand(2, 3, 40, 56, generator=g), torch.rand(2, 3, 40, 56, generator=g)
    soft = torch.rand(2, 1, 40, 56, generator=g) * 0.8 + 0.1
    soft[:, :, :5] = 0.0  # ... and some exact zeros
    pred, _ = CC.decidable_inputs(pred, tgt, soft)  # (2 to 7 pixels whose sign float32 cannot decide: criterion_check.py)
    p = pred.to(dev).requires_grad_(True)
    got = model.CURLLoss(msssim_layer=None)(p, tgt.to(dev), soft.to(dev))
    got.backward()
    pc = pred.clone().double().requires_grad_(True)
    want = O.curl_loss(pc, tgt.double(), soft.double(), torch.tensor(0.0, dtype=torch.float64))
    want.backward()
    assert abs(float(got) - float(want)) <= 2e-6, (float(got), float(want))
    CC.loss_gradient_reference(pred, tgt, soft, (0.2, 0.2, 0.2, 0.2), label="fractional mask").check(p.grad)


@pytest.mark.parametrize("kind", ["bool", "binary_float", "fractional_float"])
def test_curl_loss_one_image_mask_broadcast_over_the_batch(dev, kind):
    """a [1,1,H,W] mask at B > 1 (ops._mask expands it for the kernel).  model.py:90 sums the mask AS GIVEN (one
    image's worth) while model.py:98's mean counts its zeros once per image: value and gradient against the oracle, which
    broadcasts as the reference does."""
    import curl_oracle as O
    from curl_amd import model
    g = torch.Generator().manual_seed(28)
    B = 3
    pred, tgt = torch.rand(B, 3, 24, 40, generator=g), torch.rand(B, 3, 24, 40, generator=g)
    m = torch.rand(1, 1, 24, 40, generator=g)
    mask = {"bool": m > 0.3, "binary_float": (m > 0.3).float(), "fractional_float": torch.where(m > 0.3, m, torch.zeros(()))}[kind]
    pred, _ = CC.decidable_inputs(pred, tgt, mask)
    p = pred.to(dev).requires_grad_(True)
    got = model.CURLLoss(msssim_layer=None)(p, tgt.to(dev), mask.to(dev))
    got.backward()
    md = mask if kind == "bool" else mask.double()
    pc = pred.clone().double().requires_grad_(True)
    want = O.curl_loss(pc, tgt.double(), md, torch.tensor(0.0, dtype=torch.float64))
    want.backward()
    assert abs(float(got) - float(want)) <= 3e-6 * max(1.0, abs(float(want))), (float(got), float(want))
    CC.loss_gradient_reference(pred, tgt, mask, (0.2, 0.2, 0.2, 0.2), label=f"one-image mask, {kind}").check(p.grad)
    # and the same mask given per image: the L1 terms are then B times smaller, the cosine term the same
    full = model.CURLLoss(msssim_layer=None)(pred.to(dev), tgt.to(dev), mask.expand(B, 1, 24, 40).contiguous().to(dev))
    want_full = O.curl_loss(pred.double(), tgt.double(), md.expand(B, 1, 24, 40), torch.tensor(0.0, dtype=torch.float64))
    assert abs(float(full) - float(want_full)) <= 3e-6 and abs(float(full) - float(got)) > 1e-3


def test_curl_loss_with_msssim_vs_oracle(dev):
    """The module as the reference builds it (model.py:48: MS-SSIM of the clamped L planes, window 11), value and
    gradient against the oracle's restatement (pinned by the reference's own class, golden msssim.npz)."""
    import curl_oracle as O
    from curl_amd import model
    g = torch.Generator().manual_seed(9)
    tgt = torch.rand(2, 3, 96, 128, generator=g)
    pred = (tgt + 0.08 * torch.randn(2, 3, 96, 128, generator=g)).clamp(0, 1)
    mask = torch.rand(2, 1, 96, 128, generator=g) > 0.2
    pred, _ = CC.decidable_inputs(pred, tgt, mask)  # (2 to 7 pixels whose sign float32 cannot decide: criterion_check.py)
    crit = model.CURLLoss(ssim_window_size=5).to(dev)
    p = pred.to(dev).requires_grad_(True)
    loss = crit(p, tgt.to(dev), mask.to(dev))
    loss.backward()
    pc = pred.clone().requires_grad_(True)
    r = O.curl_loss_terms(pc, tgt, mask)
    ref = O.curl_loss(pc, tgt, mask, (1.0 - O.msssim(r[4], r[5], 11, 1)).mean())
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 5e-6
    # (the gradient's max, 603, is ONE black prediction against 4.5e-4 elsewhere: 5e-4 of it was an absolute 0.3)
    CC.criterion_reference(pred, tgt, mask, "criterion with MS-SSIM").check(p.grad)


@pytest.mark.parametrize("nc,residual_only,shape", [(126, False, (2, 12, 20)), (126, True, (1, 70, 131)),
                                                      (35, False, (3, 33, 65)), (126, False, (1, 130, 257)),
                                                      (126, False, (1, 40, 128)), (126, True, (2, 37, 256)),
                                                      (126, False, (1, 9, 600))])
def test_trispace_backward_vs_oracle_autograd(ops, dev, nc, residual_only, shape):
    """d loss / d coeffs of the fused polynomial path (C ABI) vs autograd through the oracle; sizes straddle the
    accumulation tiles: the 4096-pixel tile of the non-spatial form; for the spatial form's column strips 64-, 128- and
    256-column blocks (widths 20 / 131 / 257 / 600, 128, 256), one to five column blocks, one to three row tiles, ragged."""
    from oracle import curl_oracle as O
    g = torch.Generator().manual_seed(nc + residual_only + shape[1])
    B, H, W = shape
    img = torch.rand(B, 3, H, W, generator=g)
    coeffs = (torch.randn(B, 3, 3, nc, generator=g) * 0.3).requires_grad_(True)
    w = torch.randn(B, 3, H, W, generator=g)
    res = O.trispace_residual(img, coeffs[:, 0], coeffs[:, 1], coeffs[:, 2], spatial=(nc == 126))
    out = res if residual_only else O.generate_image(img, res)
    (out * w).sum().backward()
    got = ops.trispace_backward(img.to(dev), coeffs.detach().to(dev), w.to(dev), residual_only=residual_only)
    assert rel(got, coeffs.grad) <= 2e-4
    again = ops.trispace_backward(img.to(dev), coeffs.detach().to(dev), w.to(dev), residual_only=residual_only)
    assert torch.equal(got, again)  # fixed-order reduction: bit-reproducible


@pytest.mark.parametrize("residual_only", [False, True])
def test_trispace_backward_on_8bit_content(ops, dev, residual_only, golden):
    """tests/test_poly.py's statement on the device: the polynomial path's coefficient gradient on a whole photograph of the
    reference (bytes / 255: exact ties, the pixels generate_image's clamp pins) with black, white, grey and primary pixels
    written into it, against autograd through the oracle in FLOAT64."""
    import curl_oracle as O
    real = golden("real8")
    u8 = real["crop_u8"].copy()
    u8[0, :6] = [[0, 0, 0], [255, 255, 255], [128, 128, 128], [255, 0, 0], [0, 255, 0], [0, 0, 255]]
    img = O.u8hwc_to_f32chw(u8)[None].repeat(2, 1, 1, 1)
    g = torch.Generator().manual_seed(5 + residual_only)
    coeffs = torch.randn(2, 3, 3, 126, generator=g) * 0.3
    w = torch.randn(2, 3, 256, 256, generator=g)
    c64 = coeffs.double().requires_grad_(True)
    res = O.trispace_residual(img.double(), c64[:, 0], c64[:, 1], c64[:, 2], spatial=True)
    out = res if residual_only else O.generate_image(img.double(), res)
    (out * w.double()).sum().backward()
    got = ops.trispace_backward(img.to(dev), coeffs.to(dev), w.to(dev), residual_only=residual_only)
    assert rel(got, c64.grad) <= 1e-4, rel(got, c64.grad)


def test_trispace_backward_batch_geometry_consistent(ops, dev):
    """The training crop batch (32 x 256 x 256: 24 rows per thread, 11 row tiles) against the same images one at a time
    (16 rows per thread, 16 row tiles): the same sums in another order."""
    g = torch.Generator().manual_seed(11)
    B, H, W = 32, 256, 256
    img = torch.rand(B, 3, H, W, generator=g).to(dev)
    coeffs = (torch.randn(B, 3, 3, 126, generator=g) * 0.3).to(dev)
    w = torch.randn(B, 3, H, W, generator=g).to(dev)
    got = ops.trispace_backward(img, coeffs, w)
    for b in (0, 13, 31):
        one = ops.trispace_backward(img[b:b + 1].contiguous(), coeffs[b:b + 1].contiguous(), w[b:b + 1].contiguous())
        assert rel(got[b:b + 1], one) <= 2e-5


def test_trispace_regnet_train_step(dev):
    """TriSpaceRegNet.forward under autograd: the backbone's parameters receive the same gradients as with the
    oracle's differentiable polynomial ops downstream of the same backbone."""
    from curl_amd import model as M
    from oracle import curl_oracle as O
    torch.manual_seed(3)
    net = M.TriSpaceRegNet(spatial=True).to(dev)
    net.eval()  # batch-norm in inference mode so both passes see the same statistics
    img = torch.rand(2, 3, 48, 64, device=dev)
    mask = torch.ones(2, 1, 48, 64, device=dev)
    tgt = torch.rand(2, 3, 48, 64, device=dev)
    out = net(img, mask)
    assert out.requires_grad
    ((out - tgt) ** 2).mean().backward()
    got = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    assert got, "no parameter received a gradient"
    net.zero_grad()
    R, L, H = net.generate_coefficients(img, mask)
    ref_out = O.generate_image(img.cpu(), O.trispace_residual(img.cpu(), R.cpu(), L.cpu(), H.cpu()))  # autograd
    ((ref_out - tgt.cpu()) ** 2).mean().backward()
    worst = 0.0
    for k, p in net.named_parameters():
        if p.grad is not None and float(p.grad.abs().max()) > 0:
            worst = max(worst, rel(got[k], p.grad))
    assert worst <= 2e-3, worst


def _run_train(args, nproc=1, port=29541, timeout=600):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable]
    if nproc > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
                "--master-port", str(port)]
    cmd += ["-m", "curl_amd.train"] + args
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


SMALL = ["--crop", "64", "--train_items", "16", "--valid_items", "8", "--batch_size", "4", "--width", "0.25",
         "--valid_every", "1"]


@pytest.mark.parametrize("arch", ["trispace", "curl"])
def test_train_driver_two_rank_ddp(dev, arch):
    """BASELINE configs[4] shape, rehearsed with two processes sharing this one GPU (gloo carries DDP's gradient
    all-reduce; on the 8-GPU node the same code runs with nccl = RCCL): the replicas end with identical weights,
    the gathered loss and the all-reduced validation PSNR are finite."""
    res = _run_train(SMALL + ["--num_epoch", "2", "--parallel_mode", "ddp", "--backend", "gloo", "--arch", arch], nproc=2)
    assert res["world_size"] == 2 and res["replicas_identical"], res
    assert len(res["epochs"]) == 2
    for e in res["epochs"]:
        assert np.isfinite(e["train_loss"]) and np.isfinite(e["valid_loss"]) and np.isfinite(e["valid_psnr"])


def test_train_driver_checkpoint_resume(dev, tmp_path):
    """main.py:241-250 / 332-338: the checkpoint holds the reference's keys and a resumed run continues at its epoch."""
    res = _run_train(SMALL + ["--num_epoch", "2", "--log_dirpath", str(tmp_path), "--save_images"])
    ckpt = res["epochs"][0]["checkpoint"]
    # the Evaluator's image dump (evaluate.py:49-66): <log>/valid/<epoch>/<name>, uint8 RGB files
    from PIL import Image
    dumped = sorted((tmp_path / "valid" / "1").glob("*.png"))
    assert len(dumped) == 8
    im = np.asarray(Image.open(dumped[0]))
    assert im.shape == (64, 64, 3) and im.dtype == np.uint8
    assert all(np.isfinite(res["epochs"][i]["valid_msssim"]) for i in range(2))
    state = torch.load(ckpt, map_location="cpu")
    assert set(state) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "loss"}
    assert state["epoch"] == 1
    res2 = _run_train(SMALL + ["--num_epoch", "2", "--checkpoint_filepath", ckpt])
    assert [e["epoch"] for e in res2["epochs"]] == [2]
    assert np.isfinite(res2["epochs"][0]["train_loss"])
    assert abs(res2["epochs"][0]["lr"] - res["epochs"][1]["lr"]) <= 1e-12  # the scheduler state came back too


def test_autograd_nodes_under_autocast(dev):
    """torch.autocast around the encoder: the HIP nodes cast their inputs back to float32 (custom_fwd) and the
    parameter gradients arrive finite in the parameters' own dtype."""
    from curl_amd import model as M
    torch.manual_seed(5)
    img = torch.rand(2, 3, 64, 64, device=dev)
    mask = torch.rand(2, 1, 64, 64, device=dev) > 0.2
    tgt = torch.rand(2, 3, 64, 64, device=dev)
    crit = M.CURLLoss().to(dev)
    for net in (M.TriSpaceRegNet(spatial=True, backbone=M.CurveEncoder(1, width=0.25, num_features=1024)),
                M.GCURLNet(backbone=M.CurveEncoder(160, width=0.25))):
        net = net.to(dev).to(memory_format=torch.channels_last).train()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(img, mask)
            out = out[0] if isinstance(out, tuple) else out
        assert out.dtype == torch.float32
        loss = crit(out, tgt, mask)
        loss.backward()
        grads = [p.grad for p in net.parameters() if p.grad is not None]
        assert grads and all(g.dtype == torch.float32 and torch.isfinite(g).all() for g in grads)


def test_entry_points_are_reentrant_across_threads_and_streams(ops, dev):
    """nn.DataParallel-style callers drive forward from several host threads at once.  Four threads,
    each on its own stream and its own inputs, must get what a serial call gets."""
    import threading
    g = torch.Generator().manual_seed(17)
    jobs = []
    for t in range(4):
        img = torch.rand(2, 3, 40 + t, 64, generator=g).to(dev)
        L, R, H = (torch.randn(2, n, generator=g).mul(0.1).to(dev) for n in (48, 48, 64))
        jobs.append((img, L, R, H, ops.curl_layer_forward(img, None, L, R, H)[0].clone()))
    torch.cuda.synchronize()
    results, errors = [None] * 4, []

    def work(i):
        try:
            s = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(s):
                for _ in range(20):
                    out, _ = ops.curl_layer_forward(*jobs[i][:1], None, *jobs[i][1:4])
                s.synchronize()
            results[i] = out
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i in range(4):
        assert torch.equal(results[i], jobs[i][4])


@pytest.mark.parametrize("tag", ["loss", "rgb", "w5"])
def test_msssim_hip_vs_reference_golden(dev, golden, tag):
    """The fused MS-SSIM kernels (through curl_amd.metric.MSSSIMMetric on the device) against outputs and gradients of
    the reference's own class (tests/golden/make_golden_msssim.py), and against the stock-torch route of the mirror."""
    from curl_amd import metric, ops
    g = golden("msssim")
    ws, ch = (int(v) for v in g[tag + "_cfg"])
    m = metric.MSSSIMMetric(window_size=ws, num_channel=ch).to(dev)
    a = torch.from_numpy(g[tag + "_a"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(g[tag + "_b"]).to(dev)
    ssims, mcs = ops.msssim_stats(a.detach(), b, ws)
    assert np.abs(ssims[:, 0].cpu().numpy() - g[tag + "_ssim"]).max() <= 2e-6
    assert np.abs(mcs[:, 0].cpu().numpy() - g[tag + "_cs"]).max() <= 2e-6
    out = m(a, b)
    assert np.abs(out.detach().cpu().numpy() - g[tag + "_out"]).max() <= 3e-6
    (out * torch.from_numpy(g[tag + "_w"]).to(dev)).sum().backward()
    ref = g[tag + "_grad_a"]
    assert np.abs(a.grad.cpu().numpy() - ref).max() <= 1e-3 * np.abs(ref).max()
    again = ops.msssim_stats(a.detach(), b, ws)
    assert torch.equal(again[0], ssims) and torch.equal(again[1], mcs)  # fixed-order reductions


@pytest.mark.parametrize("shape", [(2, 1, 256, 256), (1, 3, 97, 131), (3, 1, 32, 35)])
def test_msssim_hip_odd_shapes_vs_torch_route(dev, shape):
    """Sizes that are not multiples of the 32x32 tile or of 2 (avg_pool2d floors), down to the 32-pixel minimum (below it the
    reference's fifth pooling raises; so does this path)."""
    from curl_amd import metric
    torch.manual_seed(sum(shape))
    a = torch.rand(*shape, device=dev)
    b = (a + 0.1 * torch.randn(*shape, device=dev)).clamp(0, 1)
    m = metric.MSSSIMMetric(window_size=11, num_channel=shape[1]).to(dev)
    a1 = a.clone().requires_grad_(True)
    out = m(a1, b)
    out.sum().backward()
    a2 = a.clone().requires_grad_(True)
    b2 = b.clone().requires_grad_(True)  # a gradient for the second image forces the stock-torch route
    ref = m(a2, b2)
    ref.sum().backward()
    assert float((out - ref).abs().max()) <= 3e-6
    assert float((a1.grad - a2.grad).abs().max()) <= 1e-3 * float(a2.grad.abs().max())


@pytest.mark.parametrize("case", ["identical", "constant", "black_vs_black", "black_vs_image", "saturated_patches"])
def test_msssim_hip_special_images_vs_torch_route(dev, case):
    """What evaluation meets and noise never produces (metric.py:120-211): identical images (every SSIM map is 1), constant
    images (all variances 0: the ratio of the stabilising constants), black planes (masked-out regions), flat saturated
    patches inside a photograph-like plane.  The fused statistics kernels against the stock-torch route of the same module
    (forced by asking for a gradient of the second image), values and gradients, nothing NaN that is not NaN there."""
    from curl_amd import metric
    torch.manual_seed(4)
    shape = (2, 1, 96, 80)
    a = torch.rand(*shape, device=dev)
    if case == "identical":
        b = a.clone()
    elif case == "constant":
        a = torch.full(shape, 0.5, device=dev)
        b = torch.full(shape, 0.25, device=dev)
    elif case == "black_vs_black":
        a = torch.zeros(shape, device=dev)
        b = torch.zeros(shape, device=dev)
    elif case == "black_vs_image":
        b = torch.zeros(shape, device=dev)
    else:
        a[:, :, 10:50, 10:60] = 1.0
        a[:, :, 60:90, 5:40] = 0.0
        b = (a + 0.05 * torch.randn(*shape, device=dev)).clamp(0, 1)
    m = metric.MSSSIMMetric(window_size=11, num_channel=1).to(dev)
    a1 = a.clone().requires_grad_(True)
    out = m(a1, b)
    out.sum().backward()
    a2, b2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = m(a2, b2)
    ref.sum().backward()
    assert torch.equal(torch.isnan(out), torch.isnan(ref)), (out, ref)
    ok = ~torch.isnan(ref)
    assert float((out - ref)[ok].abs().max() if bool(ok.any()) else 0.0) <= 3e-6, (out, ref)
    gn = torch.isnan(a2.grad)
    assert torch.equal(torch.isnan(a1.grad), gn)
    scale = float(a2.grad[~gn].abs().max()) if bool((~gn).any()) else 0.0
    assert float((a1.grad - a2.grad)[~gn].abs().max() if bool((~gn).any()) else 0.0) <= 1e-3 * scale + 1e-9, scale


def test_train_driver_reads_the_reference_folder_layout(dev, tmp_path):
    """--training_img_dirpath <dir>: main.py:196-210's layout (input / output / mask folders, images_train.txt,
    images_valid.txt) through curl_amd.data, one epoch with validation."""
    import os
    from PIL import Image
    rng = np.random.default_rng(1)
    for d in ("curl_example_input", "curl_example_output", "masks"):
        os.makedirs(tmp_path / d)
    for i in range(12):
        h, w = int(rng.integers(70, 100)), int(rng.integers(70, 100))
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(tmp_path / "curl_example_input" / f"{i}.png")
        Image.fromarray((rgb.astype(np.float32) ** 0.9).clip(0, 255).astype(np.uint8)).save(tmp_path / "curl_example_output" / f"{i}.png")
        m = np.full((h, w), 255, np.uint8)
        m[: h // 5] = 0
        Image.fromarray(m).save(tmp_path / "masks" / f"{i}.png")
    (tmp_path / "images_train.txt").write_text("\n".join(str(i) for i in range(8)) + "\n")
    (tmp_path / "images_valid.txt").write_text("\n".join(str(i) for i in range(8, 12)) + "\n")
    res = _run_train(["--training_img_dirpath", str(tmp_path), "--crop", "64", "--batch_size", "4", "--width", "0.25",
                      "--num_epoch", "1", "--valid_every", "1"])
    e = res["epochs"][0]
    assert np.isfinite(e["train_loss"]) and np.isfinite(e["valid_loss"]) and np.isfinite(e["valid_psnr"])
    assert 0.0 < e["valid_msssim"] <= 1.0
    # main.py:147-193: the same driver evaluates a checkpoint on a folder (images_inference.txt) and dumps the outputs
    res = _run_train(["--training_img_dirpath", str(tmp_path), "--crop", "64", "--batch_size", "4", "--width", "0.25",
                      "--num_epoch", "1", "--valid_every", "1", "--log_dirpath", str(tmp_path / "log")])
    (tmp_path / "images_inference.txt").write_text("9\n10\n11\n")
    inf = _run_train(["--checkpoint_filepath", res["epochs"][0]["checkpoint"], "--inference_img_dirpath", str(tmp_path),
                      "--crop", "64", "--batch_size", "2", "--width", "0.25", "--log_dirpath", str(tmp_path / "inf")])
    assert inf["mode"] == "inference" and inf["images"] == 3 and np.isfinite(inf["test_psnr"])
    assert sorted(p.name for p in (tmp_path / "inf" / "test" / "1").glob("*.png")) == ["10.png", "11.png", "9.png"]


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 70), (2, 3, 64), (1, 17, 65), (1, 5, 129), (1, 33, 300), (1, 100, 7),
                                   (1, 2, 1025)])
def test_trispace_backward_edge_geometries_vs_twin(ops, dev, twin, shape):
    """The spatial backward's column strips at the edges of their geometry -- one pixel, one row, one column block exactly
    full / one lane over, 64- / 128- / 256-column blocks with ragged tails, more row phases than rows, five column blocks --
    against the host twin of the same arithmetic (which is checked against the oracle's autograd in tests/test_poly.py)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = torch.rand(B, 3, H, W, generator=g)
    coeffs = torch.randn(B, 3, 3, 126, generator=g) * 0.3
    w = torch.randn(B, 3, H, W, generator=g)
    want = twin.trispace_bwd(img.numpy(), coeffs.numpy(), w.numpy(), False)
    got = ops.trispace_backward(img.to(dev), coeffs.to(dev), w.to(dev))
    assert rel(got, want) <= 2e-5
    want35 = twin.trispace_bwd(img.numpy(), coeffs[..., :35].contiguous().numpy(), w.numpy(), False)
    got35 = ops.trispace_backward(img.to(dev), coeffs[..., :35].contiguous().to(dev), w.to(dev))
    assert rel(got35, want35) <= 2e-5


def test_backward_reuses_the_forward_workspace(ops, dev):
    """CURL_F_WS_READY: the autograd node keeps the knot workspace the forward filled and the backward skips its prep
    launch -- identical gradients, through ops and through CURLLayer; a workspace of the wrong size is refused."""
    from curl_amd import model
    g = torch.Generator().manual_seed(77)
    B, H, W = 3, 40, 52
    img = torch.rand(B, 3, H, W, generator=g).to(dev)
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.2).to(dev)
    L, R, Hk = ((torch.randn(B, n, generator=g) * 0.1).to(dev) for n in (48, 48, 64))
    w = torch.randn(B, 3, H, W, generator=g).to(dev)
    wr = torch.rand(B, generator=g).to(dev)
    out, reg, ws = ops.curl_layer_forward(img, mask, L, R, Hk, return_workspace=True)
    a = ops.curl_layer_backward(img, mask, L, R, Hk, w, wr)
    b = ops.curl_layer_backward(img, mask, L, R, Hk, w, wr, workspace=ws)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        ops.curl_layer_backward(img, mask, L, R, Hk, w, wr, workspace=ws[:8])
    layer = model.CURLLayer().to(dev)
    x = img.clone().requires_grad_(True)
    Lg, Rg, Hg = (t.clone().requires_grad_(True) for t in (L, R, Hk))
    o, r = layer(x, mask, Lg, Rg, Hg)
    ((o * w).sum() + (r * wr).sum()).backward()
    assert torch.equal(x.grad, a[0]) and torch.equal(Lg.grad, a[1]) and torch.equal(Rg.grad, a[2]) and torch.equal(Hg.grad, a[3])


def test_foreground_masks_skip_masked_out_wavefronts(ops, dev):
    """Segmentation masks (data.py:186-190) leave whole wavefronts (256 consecutive pixels) masked out.  The backward skips
    their arithmetic (every gradient there is an exact zero); with CURL_F_MASK_FIRST forward and backward also wait for
    the mask and never read those pixels.  Same numbers either way -- against the flag-less call, against the float-mask
    path (which has neither shortcut), against autograd through the oracle, and through CURLLayer(foreground_masks=True)."""
    import curl_oracle as O
    from curl_amd import model
    g = torch.Generator().manual_seed(190)
    B, H, W = 2, 24, 1024
    img = torch.rand(B, 3, H, W, generator=g)
    mask = torch.rand(B, 1, H, W, generator=g) > 0.3
    mask[:, :, 5:14] = False          # nine rows of four wavefronts each: fully masked out
    mask[0, :, 14, :512] = False      # ... and half a row
    mask[1, :, :3] = True             # fully inside the foreground
    L, R, Hk = (torch.randn(B, n, generator=g) * 0.1 for n in (48, 48, 64))
    w = torch.randn(B, 3, H, W, generator=g)
    wr = torch.rand(B, generator=g)
    d = [t.to(dev) for t in (img, mask, L, R, Hk, w, wr)]
    F = ops.F_MASK_FIRST
    out0, reg0 = ops.curl_layer_forward(*d[:5])
    out1, reg1 = ops.curl_layer_forward(*d[:5], flags=F)
    assert torch.equal(out0, out1) and torch.equal(reg0, reg1)
    assert torch.equal(ops.lab_stage(d[0], d[1], d[2])[0], ops.lab_stage(d[0], d[1], d[2], flags=F)[0])
    assert torch.equal(ops.hsv_stage(d[0], d[1], d[4])[0], ops.hsv_stage(d[0], d[1], d[4], flags=F)[0])
    ref, _ = O.curl_layer(img, mask.float(), L, R, Hk)
    assert float((out1.cpu() - ref).abs().max()) <= 1e-5
    slab = torch.zeros_like(out0)   # the row-slab entry (split-pixels layout): rows 4..20 in place, mask-first
    ops.curl_layer_forward_rows(*d[:5], (4, 20), slab, flags=F)
    assert torch.equal(slab[:, :, 4:20], out0[:, :, 4:20]) and not slab[:, :, :4].any() and not slab[:, :, 20:].any()
    a = ops.curl_layer_backward(*d[:5], d[5], d[6])
    b = ops.curl_layer_backward(*d[:5], d[5], d[6], flags=F)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not a[0][:, :, 5:14].any()
    f = ops.curl_layer_backward(d[0], d[1].float(), *d[2:5], d[5], d[6])   # general path: no shortcut of either kind
    assert float((a[0] - f[0]).abs().max()) <= 2e-6 * float(f[0].abs().max())
    for x, y in zip(a[1:], f[1:]):
        assert rel(x, y) <= 1e-5
    # autograd through the oracle
    x = img.clone().requires_grad_(True)
    Lg, Rg, Hg = (t.clone().requires_grad_(True) for t in (L, R, Hk))
    o, r = O.curl_layer(x, mask.float(), Lg, Rg, Hg)
    ((o * w).sum() + (r * wr).sum()).backward()
    for got, want in zip(a[1:], (Lg.grad, Rg.grad, Hg.grad)):
        assert rel(got, want) <= 1e-3
    dd = (a[0].cpu() - x.grad).abs()
    assert float(torch.quantile(dd.flatten(), 0.995)) <= 3e-4 * float(x.grad.abs().max())
    # the module route
    layer = model.CURLLayer(foreground_masks=True).to(dev)
    xs = d[0].clone().requires_grad_(True)
    Ld, Rd, Hd = (t.clone().requires_grad_(True) for t in d[2:5])
    o, r = layer(xs, d[1], Ld, Rd, Hd)
    ((o * d[5]).sum() + (r * d[6]).sum()).backward()
    assert torch.equal(o, out0) and torch.equal(xs.grad, a[0]) and torch.equal(Ld.grad, a[1]) and torch.equal(Hd.grad, a[3])


# ------------------------------------------------------------------ one launch per call
PREP_SEPARATE, PREP_IN_KERNEL = 1 << 23, 2 << 23


@pytest.mark.parametrize("shape", [(2, 40, 64), (3, 7, 9), (1, 256, 256), (32, 32, 32)])
def test_curve_collapse_placement_is_bit_identical(ops, dev, shape):
    """CURL_F_TUNE_PREP: the image's curves collapsed in a launch of their own (knots_prep_kernel, one workgroup per image) or
    inside the streaming kernel by every workgroup (stream_selfprep_kernel; the library's choice for small launches).  The
    same device code runs either way: images, regularisers and the workspace row are BIT-identical, for every mask kind, on
    the float4 and the scalar paths, and the backward computes the same gradients from either row."""
    B, H, W = shape
    g = torch.Generator().manual_seed(B * H + W)
    img = torch.rand(B, 3, H, W, generator=g).to(dev)
    gout = torch.rand(B, 3, H, W, generator=g).to(dev)
    greg = torch.rand(B, generator=g).to(dev)
    L, R, Hk = ((torch.randn(B, n, generator=g) * 0.2).to(dev) for n in (48, 48, 64))
    holes = (torch.rand(B, 1, H, W, generator=g) > 0.3).to(dev)
    for mask in (None, holes, holes.float() * 0.7):
        o1, r1, w1 = ops.curl_layer_forward(img, mask, L, R, Hk, flags=PREP_SEPARATE, return_workspace=True)
        o2, r2, w2 = ops.curl_layer_forward(img, mask, L, R, Hk, flags=PREP_IN_KERNEL, return_workspace=True)
        o0, r0 = ops.curl_layer_forward(img, mask, L, R, Hk)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(o0, o1) and torch.equal(r0, r1)
        # every slot of the row a prep pass writes: (a, b) pairs, regularisers, masked-out colour, stamp, knots
        cols = list(range(0, 27)) + [29] + list(range(32, 32 + 160))
        assert torch.equal(w1.view(torch.int32).view(B, -1)[:, cols], w2.view(torch.int32).view(B, -1)[:, cols])
        for fn, k in ((ops.lab_stage, L), (ops.hsv_stage, Hk)):
            a, ra = fn(img, mask, k, flags=PREP_SEPARATE)
            b, rb = fn(img, mask, k, flags=PREP_IN_KERNEL)
            assert torch.equal(a, b) and torch.equal(ra, rb)
        # the backward takes the workspace row of either form (CURL_F_WS_READY): the same gradients, bit for bit
        want = ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg, workspace=w1)
        got = ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg, workspace=w2)
        none = ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg)  # no workspace: the backward's own prep launch
        for x, y, z in zip(got, want, none):
            assert torch.equal(x, y) and torch.equal(z, y)
    for fn, k in ((ops.adjust_rgb, R), (ops.adjust_lab, L), (ops.adjust_hsv, Hk)):
        a, ra = fn(img, k, flags=PREP_SEPARATE)
        b, rb = fn(img, k, flags=PREP_IN_KERNEL)
        assert torch.equal(a, b) and torch.equal(ra, rb)


def test_backward_refuses_a_workspace_nobody_filled(ops, dev):
    """CURL_F_WS_READY trusts the caller.  A workspace row that no prep pass filled for these knot counts (zeros, or
    the row of a call with other K) is answered with NaN knot gradients, not with plausible numbers."""
    B, H, W = 2, 16, 16
    g = torch.Generator().manual_seed(3)
    img, gout = (torch.rand(B, 3, H, W, generator=g).to(dev) for _ in range(2))
    L, R, Hk = ((torch.randn(B, n, generator=g) * 0.1).to(dev) for n in (48, 48, 64))
    _, _, ws = ops.curl_layer_forward(img, None, L, R, Hk, return_workspace=True)
    ok = ops.curl_layer_backward(img, None, L, R, Hk, gout, workspace=ws)
    assert all(torch.isfinite(t).all() for t in ok[1:])
    assert torch.isfinite(ok[0]).all()
    bad = ops.curl_layer_backward(img, None, L, R, Hk, gout, workspace=torch.zeros_like(ws))
    assert all(torch.isnan(t).all() for t in bad[1:])
    assert torch.isnan(bad[0]).all()  # the gradient IMAGE of such a row is NaN too, not silent garbage
    # one image's row bad, the other's good: the good image's gradients are untouched
    half = ws.clone()
    half.view(B, -1)[1].zero_()
    mixed = ops.curl_layer_backward(img, None, L, R, Hk, gout, workspace=half)
    assert torch.equal(mixed[0][0], ok[0][0]) and torch.isnan(mixed[0][1]).all()
    assert all(torch.equal(m[0], o[0]) and torch.isnan(m[1]).all() for m, o in zip(mixed[1:], ok[1:]))
    # (the scalar path -- H*W not a multiple of 4 -- takes the same check)
    i3, g3 = img[..., :15].contiguous(), gout[..., :15].contiguous()
    _, _, ws3 = ops.curl_layer_forward(i3, None, L, R, Hk, return_workspace=True)
    assert torch.isnan(ops.curl_layer_backward(i3, None, L, R, Hk, g3, workspace=torch.zeros_like(ws3))[0]).all()
    # the row of a forward with other knot counts (K = 8): same size class, another stamp
    L8, R8, H8 = ((torch.randn(B, n, generator=g) * 0.1).to(dev) for n in (24, 24, 32))
    _, _, ws8 = ops.curl_layer_forward(img, None, L8, R8, H8, return_workspace=True)
    big = torch.zeros_like(ws)
    big[:ws8.numel()] = ws8
    bad = ops.curl_layer_backward(img, None, L, R, Hk, gout, workspace=big)
    assert all(torch.isnan(t).all() for t in bad) 

@pytest.mark.parametrize("shape,mask_kind", [((3, 40, 56), "bool"), ((2, 37, 53), "bool"), ((2, 40, 56), "f32"), ((2, 40, 56), "none"),
                                             ((2, 96, 128), "broadcast_bool")])
def test_layer_and_loss_terms_in_one_forward_pass(dev, shape, mask_kind):
    """curl_layer_loss_fwd_f32 (the train step's forward as one kernel: main.py:283-285): `out`, `reg`, the five sums, both L
    planes and the workspace row are the bits of curl_layer_fwd_f32 followed by curl_loss_terms_f32 -- the float4 path, the
    scalar path (37x53), every mask kind, the in-kernel curve collapse (these sizes) -- and against the oracle."""
    import curl_oracle as O
    from curl_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(31)
    img, tgt = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    L, R, Hk = (torch.randn(B, n, generator=g) * 0.1 for n in (48, 48, 64))
    mb = torch.rand(B, 1, H, W, generator=g) > 0.25
    mask = {"bool": mb, "f32": mb.float() * 0.8, "none": None, "broadcast_bool": mb[:1]}[mask_kind]
    md = None if mask is None else mask.to(dev)
    out, reg, sums, Lp, Lt, ws = ops.layer_loss_forward(img.to(dev), md, L.to(dev), R.to(dev), Hk.to(dev), tgt.to(dev))
    out2, reg2, ws2 = ops.curl_layer_forward(img.to(dev), md, L.to(dev), R.to(dev), Hk.to(dev), return_workspace=True)
    sums2, Lp2, Lt2 = ops.loss_term_sums(out2, tgt.to(dev), md)
    assert torch.equal(out, out2) and torch.equal(reg, reg2)
    assert torch.equal(Lp, Lp2) and torch.equal(Lt, Lt2)
    assert torch.equal(sums, sums2), (sums - sums2).abs().max()
    a, b = ws.view(torch.int32).view(B, -1), ws2.view(torch.int32).view(B, -1)
    assert all(torch.equal(a[:, sl], b[:, sl]) for sl in (slice(0, 24), slice(29, 30), slice(32, 192)))
    # the workspace it filled serves the backward as the layer's own does
    gout = torch.rand(B, 3, H, W, generator=g).to(dev)
    g1 = ops.curl_layer_backward(img.to(dev), md, L.to(dev), R.to(dev), Hk.to(dev), gout, workspace=ws)
    g2 = ops.curl_layer_backward(img.to(dev), md, L.to(dev), R.to(dev), Hk.to(dev), gout, workspace=ws2)
    assert all(torch.equal(x, y) for x, y in zip(g1, g2))
    # and the oracle
    mo = torch.ones(B, 1, H, W) if mask is None else mask.float().expand(B, 1, H, W)
    ref, _ = O.curl_layer(img, mo, L, R, Hk)
    assert float((out.cpu() - ref).abs().max()) <= 1e-4


def test_layer_with_loss_module_equals_the_two_modules(dev):
    """model.CURLLayerWithLoss (one forward kernel) against model.CURLLayer + model.CURLLoss (two): the same loss, the same
    output, the same gradients w.r.t. the knots and the image -- with a stand-in for MS-SSIM that uses both L planes."""
    from curl_amd import model
    g = torch.Generator().manual_seed(32)
    B, H, W = 3, 48, 64
    img, tgt = torch.rand(B, 3, H, W, generator=g).to(dev), torch.rand(B, 3, H, W, generator=g).to(dev)
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.2).to(dev)
    fake_ssim = lambda a, b: 1.0 - (a - b).abs().mean(dim=(1, 2, 3))  # noqa: E731
    grads = []
    for fused in (True, False):
        L, R, Hk = ((torch.randn(B, n, generator=torch.Generator().manual_seed(5 + n)) * 0.1).to(dev).requires_grad_(True) for n in (48, 48, 64))
        x = img.clone().requires_grad_(True)
        if fused:
            out, reg, loss = model.CURLLayerWithLoss(msssim_layer=fake_ssim)(x, mask, L, R, Hk, tgt)
        else:
            out, reg = model.CURLLayer()(x, mask, L, R, Hk)
            loss = model.CURLLoss(msssim_layer=fake_ssim)(out, tgt, mask)
        total = loss + 1e-6 * reg.mean() + 1e-3 * out.mean()  # `out` is used downstream too (its own gradient adds)
        total.backward()
        grads.append((float(loss.detach()), out.detach(), x.grad, L.grad, R.grad, Hk.grad))
    assert grads[0][0] == grads[1][0] and torch.equal(grads[0][1], grads[1][1])
    for a, b in zip(grads[0][2:], grads[1][2:]):
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_gcurlnet_fused_train_forward_equals_the_two_calls(dev):
    """GCURLNet(img, mask, target=gt, criterion=CURLLoss) -- the train step with one forward kernel for the layer and the loss'
    pointwise terms (curl_amd.train --fused_forward) -- against criterion(net(img, mask)[0], gt, mask): loss, output and every
    parameter gradient of the encoder's head."""
    from curl_amd import model
    torch.manual_seed(11)
    net = model.GCURLNet(backbone=model.CurveEncoder(num_outputs=160, width=0.25, num_features=256), encoder_size=64).to(dev).train()
    crit = model.CURLLoss(msssim_layer=lambda a, b: 1.0 - (a - b).abs().mean(dim=(1, 2, 3))).to(dev)
    g = torch.Generator().manual_seed(12)
    img, gt = torch.rand(4, 3, 64, 64, generator=g).to(dev), torch.rand(4, 3, 64, 64, generator=g).to(dev)
    mask = (torch.rand(4, 1, 64, 64, generator=g) > 0.2).to(dev)
    res = []
    for fused in (True, False):
        net.zero_grad()
        if fused:
            out, reg, loss = net(img, mask, target=gt, criterion=crit)
        else:
            out, reg = net(img, mask)
            loss = crit(out, gt, mask)
        (loss + 1e-6 * reg.mean()).backward()
        res.append((float(loss.detach()), out.detach().clone(), [p.grad.clone() for p in net.backbone.classifier.parameters()]))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_layer_with_loss_when_only_the_loss_is_used(dev):
    """The usual training step uses the loss alone: `out` and `reg` receive no gradient (None, not a zero image to be added)."""
    from curl_amd import model
    g = torch.Generator().manual_seed(1)
    img, tgt = torch.rand(2, 3, 32, 32, generator=g).to(dev), torch.rand(2, 3, 32, 32, generator=g).to(dev)
    grads = []
    for fused in (True, False):
        L, R, H = ((torch.randn(2, n, generator=torch.Generator().manual_seed(n)) * 0.1).to(dev).requires_grad_(True) for n in (48, 48, 64))
        if fused:
            _, _, loss = model.CURLLayerWithLoss(msssim_layer=None)(img, None, L, R, H, tgt)
        else:
            out, _ = model.CURLLayer()(img, None, L, R, H)
            loss = model.CURLLoss(msssim_layer=None)(out, tgt, None)
        loss.backward()
        grads.append((float(loss.detach()), L.grad, R.grad, H.grad))
    assert grads[0][0] == grads[1][0]
    for a, b in zip(grads[0][1:], grads[1][1:]):
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
