"""GPU tests of the stand-alone polynomial layers' backward: ops.poly_layer_backward (curl_poly_layer_bwd_f32) and the autograd
surface over it (ChannelPolyLayer, Deg4MobilePolyLayer, PolyRegNet).

Inputs: img = rand, coeffs = randn * 0.3, w = randn as grad_out, from a seeded CPU generator.  Reference: autograd of
(O.channel_poly_layer(img64, c64, 4) * w64).sum() in float64.  rel(a, b) = max|a - b| / max|b|.

Bound.  The yardstick is the oracle's own float32 autograd on the same inputs against float64, computed here per case
(0.9e-7 .. 2.4e-7; floored at 2^-24, half an ulp of the largest element).  The kernel may be K times that, and never more
than the project's polynomial-backward ceiling of 2e-4.  The margin is for the kernel's order of operations, not for a wrong
term (a wrong or missing term is an error of 1e-2 and more on these inputs).
K is meant to be twice the largest kernel / yardstick ratio observed on an MI355X over the parity cases, rounded up to a power
of two.  NOT MEASURED YET: no GPU run was possible when this file was written, so K = 32 is counted from the roundings the
kernels add over torch's handful per term instead -- image gradient: three Horner chains of <= 55 sequential FMAs and three
combining ones per value; coefficient gradient: a lane's float32 chain over <= 64 pixels and an 8-step tree over the block
(the tile rows are summed in float64), (64 + 8) / ~3 -> 32.  The host twin of the same arithmetic, whose block sum is a
256-term chain instead of the tree, is at 0.7 .. 1.0 (image) and 3.4 .. 4.4 (coefficients) yardsticks.  The parity test prints
every ratio (`pytest -s`): replace K by the rule above once they are on record.
"""
import pytest
import torch

from poly_layer_bwd_ref import CEILING, case, inputs, rel

pytestmark = pytest.mark.gpu

K = 32
FLOOR = 2.0 ** -24


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


def _bound(yard):
    return min(K * max(yard, FLOOR), CEILING)


def _tile():
    from curl_amd import ops as _ops
    return _ops.poly_layer_bwd_tile(1, 1, 8192)  # pixels per tile of the coefficient pass at these sizes


T = _tile()
PARITY = [(3, (1, 1, 1)), (3, (2, 20, 64)), (3, (1, 130, 257)),
          (5, (2, 36, 40)), (5, (1, 37, 41)), (5, (1, 3, 1030)),      # (1,37,41): H*W odd -> the scalar path
          (5, (1, 1, T)), (3, (1, 1, T + 1)), (5, (1, 1, 2 * T + 3)),  # exactly one tile, one pixel more, two tiles and a tail
          (3, (1, 1, T)), (5, (1, 1, T + 1)), (3, (1, 1, 2 * T + 3))]


def _misaligned(t):
    """The same values in a tensor whose storage starts 4 bytes past an allocation boundary: contiguous, not 16-byte aligned."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@pytest.mark.parametrize("V,shape", PARITY, ids=[f"v{v}-{'x'.join(map(str, s))}" for v, s in PARITY])
def test_parity(ops, dev, V, shape):
    assert ops.poly_layer_bwd_tile(*shape) == T
    img, c, w, ref, yard = case(V, shape)
    g_img, g_c = ops.poly_layer_backward(img.to(dev), c.to(dev), w.to(dev))
    e_img, e_c = rel(g_img, ref[0]), rel(g_c, ref[1])
    print(f"\nRATIO V={V} {shape}: image {e_img:.3g} / {yard[0]:.3g} = {e_img / max(yard[0], FLOOR):.2f}, "
          f"coeffs {e_c:.3g} / {yard[1]:.3g} = {e_c / max(yard[1], FLOOR):.2f}")
    assert g_img.shape == img.shape and g_c.shape == c.shape
    assert e_img <= _bound(yard[0])
    assert e_c <= _bound(yard[1])


def test_misaligned_base_gives_the_same_values(ops, dev):
    img, c, w, _, _ = case(5, (2, 36, 40))
    img, c, w = img.to(dev), c.to(dev), w.to(dev)
    want = ops.poly_layer_backward(img, c, w)
    for a, b in ((_misaligned(img), w), (img, _misaligned(w)), (_misaligned(img), _misaligned(w))):
        got = ops.poly_layer_backward(a, c, b)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("V,shape", [(3, (2, 20, 64)), (5, (1, 37, 41))])
def test_variants(ops, dev, V, shape):
    img, c, w = (t.to(dev) for t in inputs(V, shape))
    g_img, g_c = ops.poly_layer_backward(img, c, w)
    only_c = ops.poly_layer_backward(img, c, w, need_img_grad=False)
    only_i = ops.poly_layer_backward(img, c, w, need_coeffs_grad=False)
    assert only_c[0] is None and torch.equal(only_c[1], g_c)
    assert only_i[1] is None and torch.equal(only_i[0], g_img)
    assert ops.poly_layer_backward(img, c, w, need_img_grad=False, need_coeffs_grad=False) == (None, None)


def test_reproducible(ops, dev):
    img, c, w = (t.to(dev) for t in inputs(5, (2, 36, 40)))
    a, b = ops.poly_layer_backward(img, c, w), ops.poly_layer_backward(img, c, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    img, c, w = (t.to(dev) for t in inputs(3, (32, 64, 64)))
    g_img, g_c = ops.poly_layer_backward(img, c, w)
    for i in (0, 13, 31):
        one = ops.poly_layer_backward(img[i:i + 1], c[i:i + 1], w[i:i + 1])
        assert rel(g_img[i:i + 1], one[0]) <= 2e-5 and rel(g_c[i:i + 1], one[1]) <= 2e-5


def test_rejects_bad_tensors(ops, dev):
    img, c, w = (t.to(dev) for t in inputs(3, (1, 4, 4)))
    with pytest.raises(ValueError):
        ops.poly_layer_backward(img, c, w[:, :2])
    with pytest.raises(ValueError):
        ops.poly_layer_backward(img, c[:, :, :34], w)
    with pytest.raises(ValueError):
        ops.poly_layer_backward(img.double(), c, w)
    with pytest.raises(RuntimeError):
        ops.poly_layer_backward(img, c, w.cpu())


def _layer(kind, dev):
    from curl_amd import model
    if kind == "channel5":
        return model.ChannelPolyLayer(4, 5, 3).to(dev), 5
    if kind == "channel3":
        return model.ChannelPolyLayer(4, 3, 3).to(dev), 3
    return model.Deg4MobilePolyLayer().to(dev), 5


@pytest.mark.parametrize("kind", ["channel5", "channel3", "deg4mobile"])
def test_autograd_surface(ops, dev, kind):
    layer, V = _layer(kind, dev)
    img, c, w = (t.to(dev) for t in inputs(V, (2, 20, 24)))
    with torch.no_grad():
        plain = layer(img, c)
    i, k = img.clone().requires_grad_(), c.clone().requires_grad_()
    out = layer(i, k)
    assert out.requires_grad and torch.equal(out, plain)  # the forward under grad: the same bits
    (out * w).sum().backward()
    want = ops.poly_layer_backward(img, c, w)
    assert torch.equal(i.grad, want[0]) and torch.equal(k.grad, want[1])
    # only the coefficients ask: no image gradient is formed
    i, k = img.clone(), c.clone().requires_grad_()
    (layer(i, k) * w).sum().backward()
    assert i.grad is None and torch.equal(k.grad, want[1])
    # only the image asks
    i, k = img.clone().requires_grad_(), c.clone()
    (layer(i, k) * w).sum().backward()
    assert k.grad is None and torch.equal(i.grad, want[0])


def test_autocast_gradients_arrive_in_the_inputs_dtypes(ops, dev):
    layer, V = _layer("channel3", dev)
    img, c, w = (t.to(dev) for t in inputs(V, (2, 20, 24)))
    i, k = img.clone().requires_grad_(), c.to(torch.bfloat16).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(i, k)
    assert out.dtype == torch.float32
    (out * w).sum().backward()
    assert i.grad.dtype == torch.float32 and k.grad.dtype == torch.bfloat16
    want = ops.poly_layer_backward(img, k.detach().float(), w)
    assert torch.equal(i.grad, want[0])
    assert rel(k.grad.float(), want[1]) <= 2.0 ** -8  # one rounding to bfloat16


def test_two_layers_in_sequence(dev):
    """The image gradient as a chain link: d loss / d (first layer's coefficients) through a second, 3-variable layer."""
    import curl_oracle as O
    from curl_amd import model
    img, c1, w = inputs(5, (2, 20, 24))
    c2 = inputs(3, (2, 20, 24), seed=1)[1]

    def chain(dtype):
        a, b = c1.clone().to(dtype).requires_grad_(), c2.clone().to(dtype).requires_grad_()
        mid = O.channel_poly_layer(img.to(dtype), a, 4)
        (O.channel_poly_layer(mid, b, 4) * w.to(dtype)).sum().backward()
        return a.grad, b.grad
    ref, f32 = chain(torch.float64), chain(torch.float32)
    a, b = c1.to(dev).requires_grad_(), c2.to(dev).requires_grad_()
    mid = model.ChannelPolyLayer(4, 5, 3)(img.to(dev), a)
    (model.ChannelPolyLayer(4, 3, 3)(mid, b) * w.to(dev)).sum().backward()
    for got, want, y in ((a.grad, ref[0], rel(f32[0], ref[0])), (b.grad, ref[1], rel(f32[1], ref[1]))):
        print(f"\nchain: {rel(got, want):.3g} (yardstick {y:.3g})")
        assert rel(got, want) <= _bound(y)


def test_polyregnet_trains(dev):
    """PolyRegNet under grad: d loss / d coeffs (captured by hook) against the oracle's sigmoid(channel_poly_layer) * mask in
    float64, and a finite, non-zero gradient on every backbone parameter."""
    import curl_oracle as O
    from curl_amd import model
    torch.manual_seed(4)
    net = model.PolyRegNet(backbone=model.CurveEncoder(1, width=0.25, num_features=128), feature_width=128).to(dev).eval()
    g = torch.Generator().manual_seed(11)
    img = torch.rand(2, 3, 32, 32, generator=g)
    mask = torch.rand(2, 1, 32, 32, generator=g) > 0.2
    w = torch.randn(2, 3, 32, 32, generator=g)
    seen = {}

    def hook(_, __, out):
        seen["coeffs"] = out.detach()
        out.register_hook(lambda grad: seen.__setitem__("grad", grad.detach()))
    handle = net.backbone.register_forward_hook(hook)
    out = net(img.to(dev), mask.to(dev))
    handle.remove()
    (out * w.to(dev)).sum().backward()
    coeffs = seen["coeffs"].cpu().reshape(2, 3, 35)

    def oracle(dtype):
        c = coeffs.to(dtype).requires_grad_()
        (torch.sigmoid(O.channel_poly_layer(img.to(dtype), c, 4)) * mask.to(dtype) * w.to(dtype)).sum().backward()
        return c.grad
    ref = oracle(torch.float64)
    yard = rel(oracle(torch.float32), ref)
    got = seen["grad"].cpu().reshape(2, 3, 35)
    print(f"\npolyregnet: {rel(got, ref):.3g} (yardstick {yard:.3g})")
    assert rel(got, ref) <= _bound(yard)
    for name, p in net.backbone.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
