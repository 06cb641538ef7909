"""The encoder's view from image bytes on the GPU (curl_encoder_view_u8hwc, ops.encoder_view_u8hwc, infer.enhance(view="pil"))
against Pillow's own output (tests/golden/encoder_view.npz; cases and what each exercises: tests/encoder_view_cases.py).
Equality is exact everywhere -- torch.equal -- because the arithmetic is integer and byte / 255 is correctly rounded."""
import numpy as np
import pytest
import torch
from torch import nn

import encoder_view_cases as cases
from guard_arena import IN, OUT, Buf, CLASSES, run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope="module")
def data(golden):
    """name -> (img u8 [B,H,W,C], mask u8 [B,H,W], want view f32 [B,3,S,S], want mask view f32 [B,1,S,S]); CPU tensors, made once"""
    out = {}
    for name in cases.CASES:
        img, mask = cases.inputs(name, golden)
        want = torch.from_numpy(golden[f"{name}/view"].astype(np.float32) / np.float32(255.0))
        want_m = torch.from_numpy((golden[f"{name}/mask_view"] > 0).astype(np.float32))[:, None]
        out[name] = (torch.from_numpy(img), torch.from_numpy(mask), want, want_m)
    return out


def _skewed(t, skew):
    """The same bytes in a tensor that starts `skew` bytes past an allocation boundary."""
    flat = torch.empty(t.numel() + skew, dtype=t.dtype, device=t.device)
    v = flat[skew:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("name", list(cases.CASES))
def test_view_is_pillows(dev, data, name):
    from curl_amd import ops
    img, mask, want, want_m = data[name]
    size = cases.CASES[name][2]
    view, mview = ops.encoder_view_u8hwc(img.to(dev), mask.to(dev), size=size)
    assert view.dtype == mview.dtype == torch.float32 and view.shape == want.shape and mview.shape == want_m.shape
    assert torch.equal(view.cpu(), want), (view.cpu() != want).nonzero()[:4]
    assert torch.equal(mview.cpu(), want_m), (mview.cpu() != want_m).nonzero()[:4]
    # from every byte alignment of the two inputs: the same bits
    for skew in (1, 2, 3):
        v2, m2 = ops.encoder_view_u8hwc(_skewed(img.to(dev), skew), _skewed(mask.to(dev), 4 - skew), size=size)
        assert torch.equal(v2, view) and torch.equal(m2, mview), skew
    # without a mask: the same view, no mask view
    v3, m3 = ops.encoder_view_u8hwc(img.to(dev), None, size=size)
    assert m3 is None and torch.equal(v3, view)


@pytest.mark.parametrize("shape", [(40, 56, 32), (641, 481, 32), (20, 27, 32), (97, 1003, 16)], ids=lambda s: "x".join(map(str, s)))
def test_constant_images_are_exact(dev, shape):
    """All 0 and all 255: the clip, and byte / 255 -- exactly 0.0 and exactly 1.0."""
    from curl_amd import ops
    H, W, size = shape
    for byte in (0, 255):
        img = torch.full((1, H, W, 3), byte, dtype=torch.uint8, device=dev)
        view, mview = ops.encoder_view_u8hwc(img, img[..., 0].contiguous(), size=size)
        assert torch.equal(view, torch.full_like(view, byte // 255)) and torch.equal(mview, torch.full_like(mview, byte // 255))


def test_repeatable_batch_independent_and_on_any_stream(dev, data):
    from curl_amd import ops
    img, mask, want, want_m = data["37x37_b2"]
    img3 = torch.cat([img, img.flip(1)[:1]]).to(dev)       # three different images
    mask3 = torch.cat([mask, mask.flip(1)[:1]]).to(dev)
    v, m = ops.encoder_view_u8hwc(img3, mask3, size=32)
    assert torch.equal(v[:2].cpu(), want) and torch.equal(m[:2].cpu(), want_m)
    v2, m2 = ops.encoder_view_u8hwc(img3, mask3, size=32)   # a repeated call
    assert torch.equal(v2, v) and torch.equal(m2, m)
    for b in range(3):                                       # an image alone
        vb, mb = ops.encoder_view_u8hwc(img3[b:b + 1], mask3[b:b + 1], size=32)
        assert torch.equal(vb[0], v[b]) and torch.equal(mb[0], m[b]), b
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        vs, ms = ops.encoder_view_u8hwc(img3, mask3, size=32)
    s.synchronize()
    assert torch.equal(vs, v) and torch.equal(ms, m)


def _host_plan(lib, H, W, size):
    n = lib.curl_encoder_view_plan_bytes(H, W, size)
    plan = torch.empty(n // 4, dtype=torch.int32)
    assert n > 0 and lib.curl_encoder_view_plan(H, W, size, plan.data_ptr(), n) == 0
    return plan


def _arena_call(lib, shape, C):
    B, H, W, size = shape

    def call(A):
        rc = lib.curl_encoder_view_u8hwc(A.ptr("img"), C, A.ptr("mask"), A.ptr("plan"), A.nbytes("plan"), A.ptr("view"), A.ptr("mview"),
                                         B, H, W, size, 0, torch.cuda.current_stream(A.device).cuda_stream)
        assert rc == 0, lib.curl_last_error()
    return call


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ["37x37_b2", "rgba_40x56", "641x481"])
def test_guard_bands(dev, data, name, cls):
    """Every buffer of the call exactly as long as the header says between poisoned bands, at both alignment classes: guards
    intact, inputs untouched, every output element assigned and independent of the poison around the inputs -- and Pillow's."""
    from curl_amd import _lib
    lib = _lib.load()
    img, mask, want, want_m = data[name]
    H, W, size, B, C = cases.CASES[name]
    bufs = [Buf("img", IN, img), Buf("mask", IN, mask), Buf("plan", IN, _host_plan(lib, H, W, size)),
            Buf("view", OUT, dtype=torch.float32, shape=(B, 3, size, size)), Buf("mview", OUT, dtype=torch.float32, shape=(B, 1, size, size))]
    A = run_both(bufs, cls, dev, _arena_call(lib, (B, H, W, size), C))
    assert torch.equal(A.read("view").cpu(), want) and torch.equal(A.read("mview").cpu(), want_m)


@pytest.mark.parametrize("cls", CLASSES)
def test_a_plan_for_another_shape_gives_nan_and_stays_inside(dev, data, cls):
    """The plan of 56x40, of 40x40 and of 640x900 handed to a 40x56 call: a NaN in every value of both outputs, and nothing
    written outside them (guard bands) or read from outside the inputs into a result (poison)."""
    from curl_amd import _lib
    lib = _lib.load()
    img, mask, _, _ = data["40x56"]
    need = lib.curl_encoder_view_plan_bytes(40, 56, 32)
    for other in ((56, 40, 32), (40, 40, 32), (640, 900, 32)):
        plan = _host_plan(lib, *other)
        if plan.numel() * 4 < need:  # the call checks the length it is told: a shorter plan padded to it
            plan = torch.cat([plan, torch.zeros(need // 4 - plan.numel(), dtype=torch.int32)])
        bufs = [Buf("img", IN, img), Buf("mask", IN, mask), Buf("plan", IN, plan),
                Buf("view", OUT, dtype=torch.float32, shape=(1, 3, 32, 32)), Buf("mview", OUT, dtype=torch.float32, shape=(1, 1, 32, 32))]
        A = run_both(bufs, cls, dev, _arena_call(lib, (1, 40, 56, 32), 3))
        assert bool(torch.isnan(A.read("view")).all()) and bool(torch.isnan(A.read("mview")).all()), other


@pytest.mark.parametrize("cls", CLASSES)
def test_a_stale_plan_under_the_calls_header_stays_inside(dev, data, cls):
    """The tables of 640x900 under the header of 40x56 (a plan that went stale in place): wrong values at worst -- every index
    is clamped by the call's own H and W -- never an access outside the tensors."""
    from curl_amd import _lib
    lib = _lib.load()
    img, mask, _, _ = data["40x56"]
    plan = _host_plan(lib, 40, 56, 32)
    plan[16:] = _host_plan(lib, 640, 900, 32)[16:plan.numel()]
    bufs = [Buf("img", IN, img), Buf("mask", IN, mask), Buf("plan", IN, plan),
            Buf("view", OUT, dtype=torch.float32, shape=(1, 3, 32, 32)), Buf("mview", OUT, dtype=torch.float32, shape=(1, 1, 32, 32))]
    A = run_both(bufs, cls, dev, _arena_call(lib, (1, 40, 56, 32), 3))
    v = A.read("view")
    assert bool(((v >= 0) & (v <= 1)).all())  # bytes / 255, whatever the tables say


# ------------------------------------------------------------------ infer.enhance
class _TinyBackbone(nn.Module):
    """A pooled-feature encoder with a `.classifier` slot (the heads of TriSpaceRegNet and GCURLNet go there)."""

    def __init__(self, width=16, n_out=None):
        super().__init__()
        self.conv = nn.Conv2d(3, width, 3, stride=2, padding=1)
        self.classifier = nn.Identity() if n_out is None else nn.Linear(width, n_out)

    def forward(self, x):
        return self.classifier(torch.tanh(self.conv(x)).mean((2, 3)))


BIG = "1000x1500_s320"


def test_enhance_pil_view_polynomial_model(dev, data):
    """infer.enhance(view="pil") is the byte kernel fed the coefficients of Pillow's view, byte for byte."""
    from curl_amd import infer, model as M, ops
    img, mask, want, want_m = data[BIG]
    torch.manual_seed(5)
    net = M.TriSpaceRegNet(polynomial_order=4, spatial=True, is_train=False, backbone=_TinyBackbone(), feature_width=16).to(dev).eval()
    out = infer.enhance(net, img[0].numpy(), mask[0].numpy(), dev, view="pil")
    with torch.no_grad():
        c = torch.stack(net.generate_coefficients(want.to(dev), want_m.to(dev)), 1)
    ref = ops.trispace_forward_u8hwc(img.to(dev), c, mask.to(dev))[0]
    assert out.dtype == np.uint8 and np.array_equal(out, ref.cpu().numpy())
    rgba = np.concatenate([img[0].numpy(), np.full((1000, 1500, 1), 7, np.uint8)], axis=2)  # alpha is dropped
    assert np.array_equal(infer.enhance(net, rgba, mask[0].numpy(), dev, view="pil"), out)


def test_enhance_pil_view_curve_model(dev, data):
    from curl_amd import infer, model as M, ops
    img, mask, want, want_m = data[BIG]
    torch.manual_seed(7)
    net = M.GCURLNet(backbone=_TinyBackbone(n_out=160), encoder_size=320).to(dev).eval()
    out = infer.enhance(net, img[0].numpy(), mask[0].numpy(), dev, view="pil")
    with torch.no_grad():
        knots = net.predict_knots(want.to(dev) * want_m.to(dev))
    L, R, H = knots[:, :48].contiguous(), knots[:, 48:96].contiguous(), knots[:, 96:].contiguous()
    ref, _ = ops.curl_layer_forward_u8hwc(img.to(dev), None, L, R, H, mask.to(dev))
    assert np.array_equal(out, ref[0].cpu().numpy())


def test_enhance_float_view_is_todays_route(dev):
    """view="float" (the default) is what enhance did before it had the argument."""
    from curl_amd import infer, model as M, ops
    torch.manual_seed(5)
    net = M.TriSpaceRegNet(polynomial_order=2, spatial=True, is_train=False, backbone=_TinyBackbone(), feature_width=16).to(dev).eval()
    g = torch.Generator().manual_seed(6)
    img = torch.randint(0, 256, (40, 56, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    mask = torch.randint(0, 256, (40, 56), generator=g, dtype=torch.int32).to(torch.uint8)
    out = infer.enhance(net, img.numpy(), mask.numpy(), dev)
    assert np.array_equal(out, infer.enhance(net, img.numpy(), mask.numpy(), dev, view="float"))
    x = ops.u8hwc_to_f32chw(img.to(dev)[None])
    small, msmall = infer.encoder_view(x, mask.to(dev)[None, None].float() / 255.0)
    with torch.no_grad():
        c = torch.stack(net.generate_coefficients(small, msmall), 1)
    assert np.array_equal(out, ops.trispace_forward_u8hwc(img.to(dev)[None], c, mask.to(dev)[None])[0].cpu().numpy())
    with pytest.raises(ValueError):
        infer.enhance(net, img.numpy(), mask.numpy(), dev, view="bicubic")
