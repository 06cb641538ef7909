"""GPU tests of polynomial orders 1-3: the per-order forward kernels behind curl_trispace_fwd_f32 / _slab_f32 / _u8hwc and
curl_poly_layer_f32, the gradients that reach them through the order-4 backward kernels, and the module surface.

References: the order-d model composed from the oracle's pieces (tests/poly_orders_ref.py), outputs of the reference's own
classes (tests/golden/poly_orders.npz), and the order-4 kernels -- unchanged code -- on the zero-padded table.
Bounds are the ones the degree-4 tests of the same quantities use: tests/test_gpu_parity.py's 1e-5 at coefficient scale 0.2
and 2e-5 at scale 1 for the fused forward, 3e-6 for the stand-alone layer, the byte test's "one grey level on < 1 % of the
bytes"; the gradient yardsticks and ceilings are imported from tests/trispace_img_grad_ref.py and tests/poly_layer_bwd_ref.py.
A lower order evaluates a shorter chain of the same operations: it rounds no more often than degree 4."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import poly_orders_ref as R
import trispace_img_grad_ref as IG
from conftest import max_err
from guard_arena import IN, OUT, Buf, run_both
from poly_layer_bwd_ref import CEILING, rel

pytestmark = pytest.mark.gpu

NEW = pytest.mark.parametrize("d,V,nc", R.NEW_COUNTS, ids=R.COUNT_IDS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from curl_amd import _lib
    from curl_amd import ops as _ops
    _lib.load()  # fail loudly if the HIP library is missing
    return _ops


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _misaligned(t):
    """The same values in a tensor whose storage starts 4 bytes past an allocation boundary: contiguous, not 16-byte aligned."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ------------------------------------------------------------------ fused forward, f32
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@NEW
def test_forward_vs_composed_oracle_and_order_4_kernel(ops, dev, d, V, nc, shape):
    """Image and residual against the composed oracle and against the order-4 kernel on the zero-padded table, both within the
    1e-5 the degree-4 kernels are held to at this coefficient scale (0.2); an unaligned image takes the scalar kernel to the
    same bits."""
    img, c, _ = R.inputs(nc, shape)
    x, cd = img.to(dev), c.to(dev)
    for residual_only in (True, False):
        got = ops.trispace_forward(x, cd, residual_only=residual_only)
        want = R.trispace(img, c, residual_only)
        e_ref = max_err(N(got), want.numpy())
        e_pad = max_err(N(got), N(ops.trispace_forward(x, R.pad4(c).to(dev), residual_only=residual_only)))
        print(f"\nd={d} V={V} {shape} residual_only={residual_only}: vs oracle {e_ref:.3g}, vs padded order 4 {e_pad:.3g}")
        assert e_ref <= 1e-5 and e_pad <= 1e-5
        if (shape[1] * shape[2]) % 4 == 0:
            assert torch.equal(ops.trispace_forward(_misaligned(x), cd, residual_only=residual_only), got)
        # a table that starts at an odd float of its storage is read as it stands (no 8-byte rule for these widths)
        assert torch.equal(ops.trispace_forward(x, _misaligned(cd), residual_only=residual_only), got)


@pytest.mark.parametrize("s,tol", [("s02", 1e-5), ("s1", 2e-5)])
@NEW
def test_forward_golden(ops, dev, golden, d, V, nc, s, tol):
    """Against TriSpaceRegNet.generate_residual / generate_image of the reference with ChannelPolyLayer(d)."""
    g, go = golden("poly"), golden("poly_orders")
    c = T(g[s + ("_coeffs" if V == 5 else "_coeffs35")][..., :nc], dev)
    for nm in (("img", "img8") if (s == "s02" and V == 5) else ("img",)):
        x = T(g[nm], dev)
        assert max_err(N(ops.trispace_forward(x, c, residual_only=True)), go[f"{s}_{nm}_residual_d{d}v{V}"]) <= tol, nm
        key = f"{s}_{nm}_image_d{d}v{V}"
        if key in go.files:
            assert max_err(N(ops.trispace_forward(x, c)), go[key]) <= tol, nm


@pytest.mark.parametrize("shape,rows", [((2, 30, 52), (7, 19)), ((1, 9, 7), (3, 9)), ((2, 16, 1500), (8, 16))])
@NEW
def test_rows_keep_the_full_image_coordinates(ops, dev, d, V, nc, shape, rows):
    """The slab entry equals the rows of the whole-image call bit for bit and leaves the other rows alone (shapes and slabs of
    tests/test_gpu_parity.py's order-4 test); three ranks of shard.apply_row_slab_trispace tile the image."""
    B, H, W = shape
    img, c, _ = (t.to(dev) for t in R.inputs(nc, shape, seed=1))
    full = ops.trispace_forward(img, c)
    out = torch.full_like(img, -7.0)
    ops.trispace_forward_rows(img, c, rows, out)
    r0, r1 = rows
    assert torch.equal(out[:, :, r0:r1], full[:, :, r0:r1])
    assert (out[:, :, :r0] == -7.0).all() and (out[:, :, r1:] == -7.0).all()
    if V == 5 and r0 > 0:
        assert not torch.equal(ops.trispace_forward(img[:, :, r0:r1].contiguous(), c), full[:, :, r0:r1])
    from curl_amd import shard
    both = torch.zeros_like(img)
    for rank in range(3):
        o, (a, b) = shard.apply_row_slab_trispace(img, c, rank, 3)
        both[:, :, a:b] = o[:, :, a:b]
    assert torch.equal(both, full)


# ------------------------------------------------------------------ bytes
def _u8_case(nc, shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(H * W + nc)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    white = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=g)
    white[:, : H // 3] = 0
    white[:, -H // 3:] = 255
    return img, white, torch.randn(B, 3, 3, nc, generator=g) * 0.2


def _u8_oracle(img, c, wm, dtype):
    import curl_oracle as O
    xo = torch.stack([O.u8hwc_to_f32chw(img[b].numpy()) for b in range(img.shape[0])]).to(dtype)
    yo = R.trispace(xo, c.to(dtype))
    if wm is not None:
        yo = O.white_background(yo, (wm.to(dtype) / 255).unsqueeze(1))
    return np.stack([O.f32chw_to_u8hwc(yo[b]) for b in range(img.shape[0])])


@pytest.mark.parametrize("shape", [(2, 36, 52), (1, 33, 65), (2, 7, 9)], ids=lambda s: "x".join(map(str, s)))
@NEW
def test_u8hwc_fused_file_edge(ops, dev, d, V, nc, shape):
    """The byte entry == ingest, trispace, white background, truncating egress through the f32 entry points, byte for byte; and
    within one grey level of the composed oracle on < 1 % of the bytes -- the rule and cap of the order-4 byte test, on its
    inputs (same generator, same seeds).
    Checked first, on the CPU: without compositing the oracle's own float32 chain keeps that cap against its float64 chain on
    these inputs.  With the white mask no choice of inputs can: wherever the image clamps to 0, (1 - m) * 255 with m = byte/255
    is an exact integer in real arithmetic, float32 lands on either side of it and the truncation turns that into a grey level
    -- 3 ... 12 % of the bytes here at every order, 5.5 % and 9.1 % on the order-4 test's own (1, 33, 65) inputs.  float64 is
    no yardstick at those ties; the float32 oracle, which rounds as the reference does, is the one the existing test uses."""
    img, white, c = _u8_case(nc, shape)
    for wm in (None, white):
        want = _u8_oracle(img, c, wm, torch.float32)
        if wm is None:
            own = np.abs(want.astype(int) - _u8_oracle(img, c, wm, torch.float64).astype(int))
            assert own.max() <= 1 and (own > 0).mean() < 0.01, "the oracle's own float32 noise exceeds the cap on these inputs"
        got = ops.trispace_forward_u8hwc(img.to(dev), c.to(dev), None if wm is None else wm.to(dev))
        y = ops.trispace_forward(ops.u8hwc_to_f32chw(img.to(dev)), c.to(dev))
        if wm is not None:
            m = (wm.float() / 255).unsqueeze(1).to(dev)  # divided on the CPU: torch's GPU div-by-scalar multiplies by 1/255
            y = y * m + (1 - m)
        assert torch.equal(got, ops.f32chw_to_u8hwc(y))
        dlt = np.abs(N(got).astype(int) - want.astype(int))
        assert dlt.max() <= 1 and (dlt > 0).mean() < 0.01


# ------------------------------------------------------------------ the stand-alone layer
@pytest.mark.parametrize("shape", [(2, 36, 40), (1, 37, 41), (2, 20, 64), (1, 1, 1), (1, 3, 1030)], ids=lambda s: "x".join(map(str, s)))
@NEW
def test_poly_layer_vs_oracle(ops, dev, golden, d, V, nc, shape):
    """ChannelPolyLayer(d, V, 3) through curl_poly_layer_f32 with the degree packed into num_variables: against
    O.channel_poly_layer in float64 (3e-6, the degree-4 layer's bound), the float4 and scalar kernels to the same bits, and
    against the reference's own layer on the golden inputs."""
    import curl_oracle as O
    B, H, W = shape
    g = torch.Generator().manual_seed(V * 100 + d * 10 + H + W)
    x = torch.rand(B, V, H, W, generator=g)
    c = torch.randn(B, 3, nc, generator=g) * 0.3
    got = ops.poly_layer(x.to(dev), c.to(dev))
    assert max_err(N(got), O.channel_poly_layer(x.double(), c.double(), d).numpy()) <= 3e-6
    if (H * W) % 4 == 0:
        assert torch.equal(ops.poly_layer(_misaligned(x.to(dev)), c.to(dev)), got)
    if shape == (2, 36, 40):
        gp, go = golden("poly"), golden("poly_orders")
        out = ops.poly_layer(T(gp[f"x{V}"], dev), T(gp[f"c{V}"][..., :nc], dev))
        assert max_err(N(out), go[f"channel_poly_d{d}v{V}"]) <= 3e-6


# ------------------------------------------------------------------ gradients (through the order-4 backward kernels)
def _oracle_grads(img, c, w, residual_only, dtype=torch.float64):
    """d ((residual or image) * w).sum() / d (img, coeffs) by autograd through the composed oracle, in `dtype`."""
    i = img.detach().clone().to(dtype).requires_grad_()
    k = c.detach().clone().to(dtype).requires_grad_()
    (R.trispace(i, k, residual_only) * w.to(dtype)).sum().backward()
    return i.grad, k.grad


def _exception_set(img, c, w, residual_only, g64):
    """tests/trispace_img_grad_ref.py's exception set (its constants, its sign patterns), through the composed oracle."""
    g = torch.Generator().manual_seed(4242)
    G = g64.abs().max()
    exc = torch.zeros(g64.shape[0], g64.shape[2], g64.shape[3], dtype=torch.bool)
    for _ in range(3):
        s = (torch.randint(0, 2, img.shape, generator=g) * 2 - 1).double()
        for sign in (1.0, -1.0):
            moved = _oracle_grads(img.double() + sign * IG.EXC_STEP * s, c, w, residual_only)[0]
            exc |= (moved - g64).abs().amax(1) > IG.EXC_MOVE * G
    return exc


@pytest.mark.parametrize("shape,residual_only", [((2, 36, 40), False), ((1, 37, 41), True), ((2, 7, 9), False)],
                         ids=["2x36x40-image", "1x37x41-residual", "2x7x9-image"])
@NEW
def test_gradients_through_the_autograd_node(ops, dev, d, V, nc, shape, residual_only):
    """A TriSpaceRegNet-style loss through _TriSpaceFn with image and coefficients requiring grad, against float64 autograd
    through the composed oracle: the image gradient by the yardstick, exception set and ceiling of trispace_img_grad_ref, the
    coefficient gradient by the polynomial-backward ceiling of poly_layer_bwd_ref.  The forward under grad is the no-grad
    forward's bits; the coefficient gradient has the table's own width."""
    from curl_amd import model as M
    img, c, w = R.inputs(nc, shape, scale=0.3, seed=2)
    x, k = img.to(dev).requires_grad_(), c.to(dev).requires_grad_()
    out = M._TriSpaceFn.apply(x, k, residual_only)
    assert torch.equal(out.detach(), ops.trispace_forward(img.to(dev), c.to(dev), residual_only=residual_only))
    (out * w.to(dev)).sum().backward()
    assert k.grad.shape == c.shape
    gi64, gc64 = _oracle_grads(img, c, w, residual_only)
    gi32, _ = _oracle_grads(img, c, w, residual_only, torch.float32)
    exc = _exception_set(img, c, w, residual_only, gi64)
    r32 = IG.rel_px(gi32, gi64)
    yard = float(r32[~exc].max()) if bool((~exc).any()) else 0.0
    IG.check(x.grad, gi64, yard, exc, f"d={d} V={V} {shape} residual_only={residual_only}")
    e = rel(k.grad, gc64)
    print(f"coefficient gradient: {e:.3g} (ceiling {CEILING:.3g})")
    assert bool(torch.isfinite(k.grad).all()) and e <= CEILING


@pytest.mark.parametrize("shape", [(2, 36, 40), (1, 37, 41)], ids=["2x36x40", "1x37x41"])
@NEW
def test_layer_gradients_through_the_autograd_node(ops, dev, d, V, nc, shape):
    """ChannelPolyLayer(d) through _PolyLayerFn, image and coefficients, against float64 autograd through
    O.channel_poly_layer(., ., d): tests/test_gpu_poly_layer_bwd.py's rule -- K = 32 yardsticks (the oracle's own float32
    autograd, floored at 2^-24), never more than the ceiling."""
    import curl_oracle as O
    from curl_amd import model as M
    B, H, W = shape
    g = torch.Generator().manual_seed(100 * V + 10 * d + B + 7 * H + 13 * W)
    img, c, w = torch.rand(B, V, H, W, generator=g), torch.randn(B, 3, nc, generator=g) * 0.3, torch.randn(B, 3, H, W, generator=g)

    def oracle(dtype):
        i, k = img.clone().to(dtype).requires_grad_(), c.clone().to(dtype).requires_grad_()
        (O.channel_poly_layer(i, k, d) * w.to(dtype)).sum().backward()
        return i.grad, k.grad
    ref, f32 = oracle(torch.float64), oracle(torch.float32)
    x, k = img.to(dev).requires_grad_(), c.to(dev).requires_grad_()
    lay = M.ChannelPolyLayer(d, V, 3).to(dev)
    out = lay(x, k)
    with torch.no_grad():
        assert torch.equal(out.detach(), lay(img.to(dev), c.to(dev)))
    (out * w.to(dev)).sum().backward()
    assert k.grad.shape == c.shape
    for name, got, r, y in (("image", x.grad, ref[0], f32[0]), ("coeffs", k.grad, ref[1], f32[1])):
        yard = max(rel(y, r), 2.0 ** -24)
        e = rel(got, r)
        print(f"\nd={d} V={V} {shape} {name}: {e:.3g} / {yard:.3g} = {e / yard:.2f}")
        assert e <= min(32 * yard, CEILING), name


# ------------------------------------------------------------------ guard bands
def _slab_keep(B, C, H, W, r0, n, itemsize=4):
    """The byte ranges of a [B,C,H,W] output outside rows [r0, r0 + n)."""
    keep = []
    for p in range(B * C):
        base = p * H * W * itemsize
        keep += [(base, base + r0 * W * itemsize), (base + (r0 + n) * W * itemsize, base + H * W * itemsize)]
    return keep


@pytest.mark.parametrize("cls", ["16", "16+4"])
@pytest.mark.parametrize("shape", [(2, 7, 9), (2, 36, 40)], ids=["2x7x9", "2x36x40"])
@NEW
def test_guard_bands(ops, dev, d, V, nc, shape, cls):
    """`out` of the f32, slab and byte entries and of the layer, each between poisoned bands (tests/guard_arena.py), on and 4
    bytes off the 16-byte grid: bands untouched, inputs untouched, rows outside the slab untouched, every element assigned,
    nothing depending on the poison."""
    from curl_amd import _lib
    lib = _lib.load()
    B, H, W = shape
    g = torch.Generator().manual_seed(nc * 1000 + H * W)
    img, c = torch.rand(B, 3, H, W, generator=g), torch.randn(B, 3, 3, nc, generator=g) * 0.1
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    wm = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.int32).to(torch.uint8)
    xv, cv = torch.rand(B, V, H, W, generator=g), torch.randn(B, 3, nc, generator=g) * 0.1
    s = torch.cuda.current_stream().cuda_stream
    r0, n = max(1, H // 3), max(1, H // 2)

    def ok(rc):
        assert rc == 0, (rc, lib.curl_last_error().decode("utf-8", "replace"))
    f32 = [Buf("img", IN, img), Buf("coeffs", IN, c), Buf("out", OUT, shape=(B, 3, H, W), dtype=torch.float32)]
    for flags in (0, _lib.F_RESIDUAL_ONLY):
        A = run_both(f32, cls, dev, lambda A: ok(lib.curl_trispace_fwd_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("out"), B, H, W, _lib.poly_coeffs(nc, d), flags, s)))
        assert torch.equal(A.read("out"), ops.trispace_forward(img.to(dev), c.to(dev), residual_only=bool(flags)))
    slab = f32[:2] + [Buf("out", OUT, shape=(B, 3, H, W), dtype=torch.float32, keep=_slab_keep(B, 3, H, W, r0, n))]
    A = run_both(slab, cls, dev, lambda A: ok(lib.curl_trispace_fwd_slab_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("out"), B, H, W, r0, n, _lib.poly_coeffs(nc, d), 0, s)))
    assert torch.equal(A.read("out")[:, :, r0:r0 + n], ops.trispace_forward(img.to(dev), c.to(dev))[:, :, r0:r0 + n])
    for white in (True, False):
        b8 = [Buf("img", IN, u8), Buf("coeffs", IN, c)] + ([Buf("white_mask", IN, wm)] if white else []) + \
            [Buf("out", OUT, shape=(B, H, W, 3), dtype=torch.uint8)]
        A = run_both(b8, cls, dev, lambda A: ok(lib.curl_trispace_fwd_u8hwc(A.ptr("img"), A.ptr("coeffs"), A.ptr("white_mask"), A.ptr("out"), B, H, W, _lib.poly_coeffs(nc, d), 0, s)))
        assert torch.equal(A.read("out"), ops.trispace_forward_u8hwc(u8.to(dev), c.to(dev), wm.to(dev) if white else None))
    lay = [Buf("img", IN, xv), Buf("coeffs", IN, cv), Buf("out", OUT, shape=(B, 3, H, W), dtype=torch.float32)]
    A = run_both(lay, cls, dev, lambda A: ok(lib.curl_poly_layer_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("out"), B, H, W, _lib.poly_vars(V, d), s)))
    assert torch.equal(A.read("out"), ops.poly_layer(xv.to(dev), cv.to(dev)))


# ------------------------------------------------------------------ the module surface
class _TinyBackbone(nn.Module):
    """A pooled-feature encoder with the `.classifier` slot TriSpaceRegNet fills."""

    def __init__(self, width=16):
        super().__init__()
        self.conv = nn.Conv2d(3, width, 3, stride=2, padding=1)
        self.classifier = nn.Identity()

    def forward(self, x):
        return self.classifier(torch.tanh(self.conv(x)).mean((2, 3)))


@pytest.mark.parametrize("spatial", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_trispace_regnet_module(dev, d, spatial):
    """TriSpaceRegNet(polynomial_order=d) with is_train True and False and a full-resolution target_img, and PolyRegNet(d),
    against the composed oracle on the coefficients the module's own head produced."""
    import curl_oracle as O
    from curl_amd import model as M
    torch.manual_seed(d + 10 * spatial)
    img = torch.rand(2, 3, 24, 40, device=dev)
    mask = (torch.rand(2, 1, 24, 40, device=dev) > 0.2).float()
    big = torch.rand(2, 3, 50, 70, device=dev)
    for is_train in (True, False):
        net = M.TriSpaceRegNet(polynomial_order=d, spatial=spatial, is_train=is_train, backbone=_TinyBackbone(),
                               feature_width=16).to(dev).eval()
        with torch.no_grad():
            out = net(img, mask, big)
            Rc, L, H = net.generate_coefficients(img, mask)
            res = net.generate_residual(big, Rc, L, H)
        assert Rc.shape == (2, 3, net.num_coeffs)
        ref = R.trispace_residual(big.cpu(), Rc.cpu(), L.cpu(), H.cpu(), d, spatial)
        assert max_err(N(res), ref.numpy()) <= 2e-5
        assert max_err(N(out), (O.generate_image(big.cpu(), ref) if is_train else ref).numpy()) <= 2e-5
    if not spatial:
        p = M.PolyRegNet(polynomial_order=d, backbone=_TinyBackbone(), feature_width=16).to(dev).eval()
        with torch.no_grad():
            y = p(img, mask)
            c = p.backbone(img).reshape(2, 3, p.num_coeffs)
        want = torch.sigmoid(O.channel_poly_layer(img.cpu().double(), c.cpu().double(), d)) * mask.cpu().double()
        assert max_err(N(y), want.numpy()) <= 3e-6


def test_infer_byte_path_at_order_2(dev):
    """infer.enhance hands the byte kernel whatever the model's head produces: an order-2 model end to end."""
    from curl_amd import infer, model as M, ops as _ops
    torch.manual_seed(5)
    net = M.TriSpaceRegNet(polynomial_order=2, spatial=True, is_train=False, backbone=_TinyBackbone(), feature_width=16).to(dev).eval()
    g = torch.Generator().manual_seed(6)
    img = torch.randint(0, 256, (40, 56, 3), generator=g, dtype=torch.int32).to(torch.uint8).numpy()
    mask = torch.randint(0, 256, (40, 56), generator=g, dtype=torch.int32).to(torch.uint8).numpy()
    out = infer.enhance(net, img, mask, dev)
    assert out.shape == img.shape and out.dtype == np.uint8
    x = _ops.u8hwc_to_f32chw(torch.from_numpy(img).to(dev)[None])
    tm = torch.from_numpy(mask).to(dev)[None, None].float() / 255.0
    small, msmall = infer.encoder_view(x, tm)
    with torch.no_grad():
        c = torch.stack(net.generate_coefficients(small, msmall), 1)
    assert c.shape[-1] == 21
    want = _ops.trispace_forward_u8hwc(torch.from_numpy(img).to(dev)[None], c, torch.from_numpy(mask).to(dev)[None])[0]
    assert np.array_equal(out, N(want))


def test_training_step_end_to_end_order_3(dev):
    """TriSpaceRegNet(polynomial_order=3, spatial=True) + CURLLoss, one backward on a 2x3x32x32 crop: every parameter gradient
    finite and equal to the float64 gradient of the same model composed from the oracle's pieces, within the
    polynomial-backward ceiling (relative to each tensor's largest element)."""
    import curl_oracle as O
    from curl_amd import model as M
    torch.manual_seed(11)
    net = M.TriSpaceRegNet(polynomial_order=3, spatial=True, backbone=_TinyBackbone(), feature_width=16).to(dev).train()
    g = torch.Generator().manual_seed(12)
    img, tgt = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g)
    mask = torch.rand(2, 1, 32, 32, generator=g) > 0.2
    ref_net = copy.deepcopy(net).cpu().double()
    crit = M.CURLLoss(msssim_layer=None).to(dev)  # the four pointwise terms: MS-SSIM's five scales need more than 32 pixels
    loss = crit(net(img.to(dev), mask.to(dev)), tgt.to(dev), mask.to(dev))
    loss.backward()
    c64 = ref_net.backbone(img.double() * mask.double()).reshape(2, 3, 3, 56)
    ref = O.curl_loss(R.trispace(img.double(), c64), tgt.double(), mask, 0.0)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 5e-6
    for (name, p), q in zip(net.named_parameters(), ref_net.parameters()):
        if not p.requires_grad:
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        e = rel(p.grad, q.grad)
        print(f"{name}: {e:.3g}")
        assert e <= CEILING, (name, e)
