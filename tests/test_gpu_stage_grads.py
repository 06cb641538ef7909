"""Autograd through the stand-alone curve ops, converters and fused stages (curves.*, colors.*, ops.*) on the device:
gradients against float64 autograd through the oracle, the reference's CURLLayer.forward written out of the drop-in
pieces against model.CURLLayer's fused backward, the forward under grad bit-equal to the no-grad call, reproducible
backward calls, and the forward-only forms refusing to run under grad."""
import pytest
import torch

import curl_oracle as O
import jacobian_check as JC
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]
TOL = 2e-4  # tests/test_twin_bwd.py's
SMALLEST = (2, 7, 9)
JC_KIND = {"random": "random", "grid8": "grid8", "saturated": "wide"}  # jacobian_check's content for a case here
# ... drawn with a seed at which every operator's 126 pixels meet the input conditions (one pixel is 0.8 % there; 8-bit hues of
# exactly 85 / 255 and 170 / 255 are near kinks of hsv2rgb, and the default draw holds two of them)
JC_SEED = 4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from curl_amd import _lib, ops
    _lib.load()
    return ops


def check_image_grad(got, want, what, want32=None):
    """0.999-quantile within TOL of the gradient scale, max within 20 TOL.  want32: the reference's gradient once more, in
    float32 or at inputs moved by 1e-6: pixels where it differs from `want` sit on one of the reference's kinks (a clamp
    reached exactly, a hue on a ramp's end) and are left out (at most 1 %)."""
    got, want = got.detach().double().cpu().flatten(), want.detach().double().cpu().flatten()
    d = (got - want).abs()
    scale = max(want.abs().max().item(), 1e-30)
    if want32 is not None:
        alts = want32 if isinstance(want32, (list, tuple)) else [want32]
        kink = torch.zeros_like(want, dtype=torch.bool)
        for alt in alts:
            kink |= (alt.detach().double().cpu().flatten() - want).abs() > TOL * scale
        assert kink.double().mean().item() <= 0.01, what
        d = d[~kink]
    if d.numel() == 0:
        return
    assert torch.quantile(d, 0.999).item() <= TOL * scale and d.max().item() <= 20 * TOL * scale, (what, d.max().item() / scale)


def check_knot_grad(got, want, what, tol=TOL):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    r = (got - want).abs().max().item() / max(1e-12, want.abs().max().item())
    assert r <= tol, (what, r, tol)


def knot_conditioning(op, img, mask, raw, w, wr, want):
    """How far the float64 oracle's own knot gradient moves when the image moves by float32 rounding (1e-7): on 8-bit content
    many pixels share a colour, and where that colour sits on a kink of the reference (a clamp reached exactly) the knot
    gradient jumps by that pixel group's share -- either side is the reference's answer."""
    worst = 0.0
    for seed in range(3):
        g = torch.Generator().manual_seed(seed)
        _, moved = oracle_grads(op, img + 1e-7 * torch.randn(img.shape, generator=g, dtype=img.dtype), mask, raw, w, wr)
        worst = max(worst, (moved - want).abs().max().item() / max(1e-12, want.abs().max().item()))
    return worst


CURVE_OPS = {"adjust_rgb": 3, "adjust_lab": 3, "adjust_hsv": 4, "lab_stage": 3, "hsv_stage": 4}


def make_inputs(op, B, H, W, case, seed, n=None):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g)
    if case == "grid8":
        img = torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255
        img[:, 1, : H // 3] = img[:, 0, : H // 3]
    if case == "saturated":
        img = img * 1.6 - 0.3
    nc = CURVE_OPS.get(op, 3)
    n = n or (48 if nc == 3 else 64)
    raw = torch.randn(B, n, generator=g) * 0.3
    w = torch.randn(B, 3, H, W, generator=g)
    wr = torch.rand(B, generator=g)
    holes = torch.rand(B, 1, H, W, generator=g) > 0.3
    soft = torch.rand(B, 1, H, W, generator=g)
    return img, raw, w, wr, holes, soft


def oracle_grads(op, img, mask, raw, w, wr, dtype=torch.float64, use_reg=True):
    x = img.to(dtype).clone().requires_grad_(True)
    k = raw.to(dtype).clone().requires_grad_(True)
    if op in ("lab_stage", "hsv_stage"):
        m = torch.ones_like(x[:, :1]) if mask is None else mask.to(dtype)
        out, reg = getattr(O, op)(x, m, k, k.shape[1])
    else:
        out, reg = getattr(O, op)(x, k)
    loss = (out * w.to(dtype)).sum() + ((reg * wr.to(dtype)).sum() if use_reg else 0)
    loss.backward()
    return x.grad, k.grad


def ours(ops, op, img, mask, raw, w, wr, dev, flags=0, use_reg=True, img_grad=True, knot_grad=True):
    x = img.to(dev).clone().requires_grad_(img_grad)
    k = raw.to(dev).clone().requires_grad_(knot_grad)
    if op in ("lab_stage", "hsv_stage"):
        out, reg = getattr(ops, op)(x, None if mask is None else mask.to(dev), k, flags=flags)
    else:
        out, reg = getattr(ops, op)(x, k)
    loss = (out * w.to(dev)).sum() + ((reg * wr.to(dev)).sum() if use_reg else 0)
    loss.backward()
    return x.grad, k.grad


@pytest.mark.parametrize("shape", [(1, 33, 65), (2, 7, 9), (2, 64, 256)])
@pytest.mark.parametrize("case", ["random", "grid8", "saturated"])
@pytest.mark.parametrize("op", list(CURVE_OPS))
def test_curve_ops_vs_oracle(ops, dev, op, case, shape):
    img, raw, w, wr, _, _ = make_inputs(op, *shape, case, seed=100 * list(CURVE_OPS).index(op) + 10 * len(case) + shape[1])
    gi, gk = ours(ops, op, img, None, raw, w, wr, dev)
    wi, wk = oracle_grads(op, img, None, raw, w, wr)
    wi32, _ = oracle_grads(op, img, None, raw, w, wr, dtype=torch.float32)
    check_image_grad(gi, wi, (op, case, shape), wi32)
    try:
        check_knot_grad(gk, wk, (op, case, shape))
    except AssertionError:
        if case != "grid8":
            raise
        check_knot_grad(gk, wk, (op, case, shape), 2 * knot_conditioning(op, img, None, raw, w, wr, wk))
    if shape == SMALLEST:
        # the autograd node (_curve_op_grad) under tests/jacobian_check.py's per-pixel bar: one-hot w, the smallest shape
        # (input conditions asserted by JC.case_references before the kernel runs)
        ref, = JC.case_references(op, JC_KIND[case], "s03", shape, seed=JC_SEED)

        def rows(go):
            gi, gk = ours(ops, op, ref.x, None, ref.raw, go, wr, dev, use_reg=False)
            return gi.cpu(), gk.cpu()
        J, K = JC.one_hot_jacobian(rows, shape)
        ref.check(J)
        ref.check_knots(K)


@pytest.mark.parametrize("mask_first", [False, True])
@pytest.mark.parametrize("kind", ["none", "bool", "uint8", "float32"])
@pytest.mark.parametrize("op", ["lab_stage", "hsv_stage"])
def test_stage_masks(ops, dev, op, kind, mask_first):
    img, raw, w, wr, holes, soft = make_inputs(op, 2, 64, 256, "random", seed=5)
    holes[:, :, :32] = False  # whole wavefronts masked out: the skipped-wave path
    mask = {"none": None, "bool": holes, "uint8": holes.to(torch.uint8), "float32": soft}[kind]
    flags = ops.F_MASK_FIRST if mask_first else 0
    gi, gk = ours(ops, op, img, mask, raw, w, wr, dev, flags=flags)
    om = None if mask is None else mask.double()
    wi, wk = oracle_grads(op, img, om, raw, w, wr)
    check_image_grad(gi, wi, (op, kind, mask_first))
    check_knot_grad(gk, wk, (op, kind, mask_first))


@pytest.mark.parametrize("case", ["random", "grid8", "saturated"])
@pytest.mark.parametrize("name,cls", [("rgb2lab", "RGB2LAB"), ("lab2rgb", "LAB2RGB"), ("rgb2hsv", "RGB2HSV"), ("hsv2rgb", "HSV2RGB")])
def test_converters_vs_oracle(dev, name, cls, case):
    from curl_amd import colors
    mod = getattr(colors, cls)().to(dev)
    for shape in ((1, 33, 65), (2, 7, 9), (2, 64, 256)):
        img, _, w, _, _, _ = make_inputs("adjust_rgb", *shape, case, seed=len(name) + len(case))
        x = img.to(dev).requires_grad_(True)
        (mod(x) * w.to(dev)).sum().backward()
        want = {}
        for dt in (torch.float64, torch.float32):
            y = img.to(dt).requires_grad_(True)
            (getattr(O, name)(y) * w.to(dt)).sum().backward()
            want[dt] = y.grad
        check_image_grad(x.grad, want[torch.float64], (name, case, shape), want[torch.float32])
    # the autograd node (_ConvertFn) under tests/jacobian_check.py's per-pixel bar: one-hot w, the smallest shape (input
    # conditions asserted by JC.case_references before the kernel runs)
    ref, = JC.case_references(name, JC_KIND[case], None, SMALLEST, seed=JC_SEED)

    def rows(go):
        x = ref.x.to(dev).requires_grad_(True)
        (mod(x) * go.to(dev)).sum().backward()
        return x.grad.cpu()
    ref.check(JC.one_hot_jacobian(rows, SMALLEST))


@pytest.mark.parametrize("op", ["adjust_rgb", "adjust_lab", "adjust_hsv"])
def test_curves_module_and_uneven_knots(dev, op):
    """curves.* inherit the autograd path; torch.chunk's shorter last curve (47 = 16 + 16 + 15, 61 = 16 x 3 + 13)."""
    from curl_amd import curves
    n = 47 if CURVE_OPS[op] == 3 else 61
    img, raw, w, wr, _, _ = make_inputs(op, 2, 33, 65, "random", seed=9, n=n)
    x, k = img.to(dev).requires_grad_(True), raw.to(dev).requires_grad_(True)
    out, reg = getattr(curves, op)(x, k)
    ((out * w.to(dev)).sum() + (reg * wr.to(dev)).sum()).backward()
    wi, wk = oracle_grads(op, img, None, raw, w, wr)
    check_image_grad(x.grad, wi, op)
    check_knot_grad(k.grad, wk, op)


@pytest.mark.parametrize("op", list(CURVE_OPS))
def test_misaligned_view_reg_unused_and_partial_grads(ops, dev, op):
    """A view one float into its storage (the scalar kernels), grad_reg unused, gradient w.r.t. the knots only / the image only."""
    B, H, W = 2, 16, 24
    img, raw, w, wr, holes, _ = make_inputs(op, B, H, W, "random", seed=13)
    mask = holes if op.endswith("stage") else None
    base = torch.zeros(1 + img.numel(), device=dev)
    x = base[1:].view(B, 3, H, W)  # contiguous, one float off the float4 grid: the scalar kernels, forward and backward
    x.copy_(img.to(dev))
    assert x.data_ptr() % 16 != 0
    x.requires_grad_(True)
    k = raw.to(dev).requires_grad_(True)
    out, _ = getattr(ops, op)(x, mask.to(dev), k) if mask is not None else getattr(ops, op)(x, k)
    (out * w.to(dev)).sum().backward()  # grad_reg unused
    om = None if mask is None else mask.double()
    wi, wk = oracle_grads(op, img, om, raw, w, wr, use_reg=False)
    check_image_grad(x.grad, wi, (op, "misaligned"))
    check_knot_grad(k.grad, wk, (op, "misaligned"))
    # knots only: no image gradient computed; image only: no knot gradient
    gi, gk = ours(ops, op, img, mask, raw, w, wr, dev, img_grad=False)
    assert gi is None
    check_knot_grad(gk, oracle_grads(op, img, om, raw, w, wr)[1], (op, "knots only"))
    gi, gk = ours(ops, op, img, mask, raw, w, wr, dev, knot_grad=False)
    assert gk is None
    check_image_grad(gi, oracle_grads(op, img, om, raw, w, wr)[0], (op, "image only"))


@pytest.mark.parametrize("op", list(CURVE_OPS))
def test_empty_image(ops, dev, op):
    """An empty image: an empty image gradient, and the knots still receive the regulariser's gradient."""
    raw = (torch.randn(2, 48 if CURVE_OPS[op] == 3 else 64) * 0.3).to(dev).requires_grad_(True)
    x = torch.empty(2, 3, 0, 5, device=dev, requires_grad=True)
    out, reg = getattr(ops, op)(x, None, raw) if op.endswith("stage") else getattr(ops, op)(x, raw)
    (out.sum() + reg.sum()).backward()
    assert x.grad.shape == x.shape
    _, wk = oracle_grads(op, torch.rand(2, 3, 1, 1), None, raw.detach().cpu(), torch.zeros(2, 3, 1, 1), torch.ones(2))
    check_knot_grad(raw.grad, wk, (op, "empty"))


def test_one_full_frame(ops, dev):
    """2 x 3 x 1500 x 1000 against the float64 oracle (on the host: the oracle builds its constants there)."""
    g = torch.Generator(device=dev).manual_seed(3)
    B, H, W = 2, 1500, 1000
    img = torch.rand(B, 3, H, W, device=dev, generator=g)
    mask = torch.rand(B, 1, H, W, device=dev, generator=g) > 0.3
    w = torch.randn(B, 3, H, W, device=dev, generator=g)
    wr = torch.rand(B, device=dev, generator=g)
    for op in CURVE_OPS:
        raw = torch.randn(B, 48 if CURVE_OPS[op] == 3 else 64, device=dev, generator=g) * 0.3
        m = mask if op.endswith("stage") else None
        gi, gk = ours(ops, op, img, m, raw, w, wr, dev)
        om = None if m is None else m.double().cpu()
        wi, wk = oracle_grads(op, img.cpu(), om, raw.cpu(), w.cpu(), wr.cpu())
        noise = 1e-6 * torch.randn(img.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        moved = [oracle_grads(op, img.cpu().double() + sgn * noise, om, raw.cpu(), w.cpu(), wr.cpu()) for sgn in (1, -1)]
        check_image_grad(gi, wi, (op, "frame"), [mv[0] for mv in moved])
        # the knot sums see the kink pixels too: the tolerance grows by what moving the inputs does to the reference's own
        kink_share = max((mv[1] - wk).abs().max().item() for mv in moved) / wk.abs().max().item()
        check_knot_grad(gk, wk, (op, "frame"), max(TOL, 2 * kink_share))
        del gi, gk, wi, wk, moved
    from curl_amd import colors
    for cls, name in (("RGB2LAB", "rgb2lab"), ("RGB2HSV", "rgb2hsv")):
        x = img[:1].clone().requires_grad_(True)
        (getattr(colors, cls)()(x) * w[:1]).sum().backward()
        y = img[:1].double().cpu().requires_grad_(True)
        (getattr(O, name)(y) * w[:1].double().cpu()).sum().backward()
        check_image_grad(x.grad, y.grad, (name, "frame"))


def test_drop_in_model_matches_fused_layer(dev):
    """The reference's CURLLayer.forward (model.py:151-176) written out of the drop-in pieces: its autograd gradients equal
    model.CURLLayer's fused backward and the oracle's."""
    from curl_amd import colors, curves, model
    rgb2lab, lab2rgb, rgb2hsv, hsv2rgb = colors.RGB2LAB(), colors.LAB2RGB(), colors.RGB2HSV(), colors.HSV2RGB()

    def piecewise(img, mask, L, R, H):  # model.py:151-176 without the dead `feat` lines
        img_lab = rgb2lab(img)
        img_lab, gradient_regulariser_lab = curves.adjust_lab(img_lab, L[:, :48])
        img_lab = img_lab * mask
        img_rgb = lab2rgb(img_lab)
        img_rgb, gradient_regulariser_rgb = curves.adjust_rgb(img_rgb, R[:, :48])
        img_rgb = img_rgb * mask
        img_hsv = rgb2hsv(img_rgb)
        img_hsv, gradient_regulariser_hsv = curves.adjust_hsv(img_hsv, H[:, :64])
        img_hsv = img_hsv * mask
        img_residual = hsv2rgb(img_hsv)
        img = torch.clamp(img + img_residual, 0.0, 1.0) * mask
        return img, gradient_regulariser_rgb + gradient_regulariser_lab + gradient_regulariser_hsv

    B, H, W = 2, 40, 64
    g = torch.Generator().manual_seed(21)
    img = torch.rand(B, 3, H, W, generator=g)
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.2).float()
    L, R, Hk = (torch.randn(B, n, generator=g) * 0.1 for n in (48, 48, 64))
    w = torch.randn(B, 3, H, W, generator=g)
    wr = torch.rand(B, generator=g)
    res = []
    for fn in (piecewise, model.CURLLayer().to(dev)):
        x = img.to(dev).requires_grad_(True)
        ks = [t.to(dev).requires_grad_(True) for t in (L, R, Hk)]
        out, reg = fn(x, mask.to(dev), *ks)
        ((out * w.to(dev)).sum() + (reg * wr.to(dev)).sum()).backward()
        res.append([x.grad] + [k.grad for k in ks])
    ref = O.layer_gradients(img, mask, L, R, Hk, w, wr)
    for i, name in enumerate(("img", "L", "R", "H")):
        if name == "img":
            check_image_grad(res[0][i], res[1][i], ("piecewise vs fused", name))
            check_image_grad(res[0][i], ref[i], ("piecewise vs oracle", name))
        else:
            check_knot_grad(res[0][i], res[1][i], ("piecewise vs fused", name))
            check_knot_grad(res[0][i], ref[i], ("piecewise vs oracle", name))


def test_forward_unchanged_and_backward_reproducible(ops, dev):
    img, raw, w, wr, holes, soft = make_inputs("lab_stage", 2, 64, 256, "random", seed=31)
    img, w, wr, holes = img.to(dev), w.to(dev), wr.to(dev), holes.to(dev)
    from curl_amd import colors
    for op in CURVE_OPS:
        k = (raw if CURVE_OPS[op] == 3 else torch.randn(2, 64) * 0.3).to(dev)
        args = (holes,) if op.endswith("stage") else ()
        with torch.no_grad():
            o0, r0 = getattr(ops, op)(img, *args, k)
        x, kg = img.clone().requires_grad_(True), k.clone().requires_grad_(True)
        o1, r1 = getattr(ops, op)(x, *args, kg)
        assert o1.grad_fn is not None and torch.equal(o0, o1) and torch.equal(r0, r1), op
        grads = []
        for _ in range(2):
            x.grad = kg.grad = None
            o, r = getattr(ops, op)(x, *args, kg)
            ((o * w).sum() + (r * wr).sum()).backward()
            grads.append((x.grad.clone(), kg.grad.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*grads)), op
    for cls in ("RGB2LAB", "LAB2RGB", "RGB2HSV", "HSV2RGB"):
        mod = getattr(colors, cls)()
        with torch.no_grad():
            o0 = mod(img)
        x = img.clone().requires_grad_(True)
        o1 = mod(x)
        assert o1.grad_fn is not None and torch.equal(o0, o1), cls


def test_forward_only_forms_refuse_grad(ops, dev):
    from curl_amd import curves
    img = torch.rand(1, 3, 8, 8, device=dev, requires_grad=True)
    C = torch.rand(1, 16, device=dev) + 0.5
    with pytest.raises(NotImplementedError):
        curves.apply_curve(img, C, torch.zeros(1, device=dev), 0, 0)
    with pytest.raises(NotImplementedError):
        ops.apply_curve(img.detach(), C.requires_grad_(True), None, 0, 0)
    k = torch.randn(1, 48, device=dev, requires_grad=True)
    for fn in (lambda: ops.adjust_rgb(img, k, flags=ops.F_PWL), lambda: ops.lab_stage(img, None, k, flags=ops.F_PWL)):
        with pytest.raises(NotImplementedError):
            fn()
    with torch.no_grad():  # the same calls without grad still run
        ops.adjust_rgb(img, k, flags=ops.F_PWL)
        curves.apply_curve(img, C, None, 0, 0)
