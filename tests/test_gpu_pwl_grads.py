"""The fused layer's backward with the paper's piecewise-linear curves on the device (ops.curl_layer_backward(..., flags=F_PWL),
curl_layer_pwl_bwd_f32): gradients against float64 autograd through the PWL restatement of tests/test_twin_pwl_bwd.py (whose
forward is pinned to the GPU PWL forward here), every mask kind with CURL_F_MASK_FIRST on and off, the float4 and scalar paths,
with and without the image gradient and the forward's workspace, K = 16 and 64; reproducible, batch-independent results; an
empty image and a full frame; CURLLayer(paper_pwl=True) under grad (same forward bits, a grad_fn, it trains)."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from test_twin_pwl_bwd import kinks, make_case, oracle_grads, smooth_knots

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from curl_amd import _lib, ops
    _lib.load()
    return ops


def check_knots(got, want, want32, what):
    """tests/test_gpu_backward.py's 1e-3 of the largest, or three times the float32 restatement's own error if larger."""
    want, want32, got = (np.asarray(a, np.float64) for a in (want, want32, got))
    scale = max(np.abs(want).max(), 1e-12)
    tol = max(1e-3, 3 * np.abs(want32 - want).max() / scale)
    r = np.abs(got - want).max() / scale
    assert r <= tol, (what, r, tol)


def check_image(got, want, want32, what):
    """99.5 % quantile within 3e-4 of the largest (tests/test_gpu_backward.py), pixels on a float32 / float64 kink left out."""
    want = np.asarray(want, np.float64)
    scale = max(np.abs(want).max(), 1e-30)
    kink = np.broadcast_to(kinks(want32, want, scale), want.shape)
    assert kink.mean() <= 0.01, (what, float(kink.mean()))
    d = np.abs(np.asarray(got, np.float64) - want)[~kink]
    assert np.quantile(d, 0.995) <= 3e-4 * scale, (what, float(np.quantile(d, 0.995) / scale))


def _case(case, K, seed, W=20):
    img, mask, binary, L, R, Hk, gout, greg = make_case(case, K, seed, B=2, H=12, W=W)
    return img, mask, L, R, Hk, gout, greg


def _gpu_mask(mask, kind, dev):
    if mask is None:
        return None
    m = torch.from_numpy(mask).to(dev)
    return m > 0.5 if kind == "bool" else (m > 0.5).to(torch.uint8) if kind == "u8" else m


def _run(ops, dev, img, m, L, R, Hk, gout, greg, need_img=True, ws_ready=False, flags=0):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ws = None
    if ws_ready:
        _, _, ws = ops.curl_layer_forward(T(img), m, T(L), T(R), T(Hk), flags=ops.F_PWL | flags, return_workspace=True)
    gi, gL, gR, gH = ops.curl_layer_backward(T(img), m, T(L), T(R), T(Hk), T(gout), T(greg), need_img, workspace=ws,
                                             flags=ops.F_PWL | flags)
    return (None if gi is None else gi.cpu().numpy()), gL.cpu().numpy(), gR.cpu().numpy(), gH.cpu().numpy()


MASKS = ["none", "bool", "u8", "f32"]


@pytest.mark.parametrize("K", [16, 64])
@pytest.mark.parametrize("mask_kind,mask_first", [(k, False) for k in MASKS] + [("bool", True), ("u8", True)])
@pytest.mark.parametrize("W", [20, 21])  # float4 path, scalar path (odd W)
def test_pwl_backward_vs_oracle(ops, dev, K, mask_kind, mask_first, W):
    backward_vs_oracle(ops, dev, K, mask_kind, mask_first, W, 40 + K + W + MASKS.index(mask_kind))


def backward_vs_oracle(ops, dev, K, mask_kind, mask_first, W, seed):
    """K: knots per curve, one count or (Kl, Kr, Kh) (tests/test_gpu_knot_paths.py runs this body off K = 16 and 64)."""
    case = {"none": "random", "bool": "boolmask", "u8": "boolmask", "f32": "softmask"}[mask_kind]
    img, mask, L, R, Hk, gout, greg = _case(case, K, seed, W)
    if mask is not None and mask_kind in ("bool", "u8"):
        mask[0] = 0  # a whole image masked out: every wavefront of it takes the dead-wave skip
    m = _gpu_mask(mask, mask_kind, dev)
    flags = ops.F_MASK_FIRST if mask_first else 0
    out, wi, wL, wR, wH = oracle_grads(img, mask, L, R, Hk, gout, greg)
    _, wi32, *w32 = oracle_grads(img, mask, L, R, Hk, gout, greg, torch.float32)
    # the restatement is the GPU PWL forward's function (2e-5: the kernels' hardware log2 / exp2 / rcp)
    fwd, _ = ops.curl_layer_forward(torch.from_numpy(img).to(dev), m, *(torch.from_numpy(a).to(dev) for a in (L, R, Hk)),
                                    flags=ops.F_PWL)
    assert np.abs(fwd.cpu().numpy() - out).max() <= 2e-5
    for need_img in (True, False):
        for ws_ready in (False, True):
            what = (K, mask_kind, mask_first, W, need_img, ws_ready)
            gi, gL, gR, gH = _run(ops, dev, img, m, L, R, Hk, gout, greg, need_img, ws_ready, flags)
            if need_img:
                check_image(gi, wi, wi32, what)
            else:
                assert gi is None
            for got, want, want32 in ((gL, wL, w32[0]), (gR, wR, w32[1]), (gH, wH, w32[2])):
                check_knots(got, want, want32, what)


def test_pwl_backward_is_reproducible_and_batch_independent(ops, dev):
    img, mask, L, R, Hk, gout, greg = _case("random", 16, 5)
    a = _run(ops, dev, img, None, L, R, Hk, gout, greg)
    b = _run(ops, dev, img, None, L, R, Hk, gout, greg)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    one = _run(ops, dev, img[1:], None, L[1:], R[1:], Hk[1:], gout[1:], greg[1:])
    for x, y in zip(a, one):
        assert np.array_equal(x[1:], y)


def test_pwl_backward_empty_image_and_full_frame(ops, dev):
    g = torch.Generator().manual_seed(3)
    L, R, Hk = (smooth_knots(2, n, 16, g).to(dev) for n in (3, 3, 4))
    greg = torch.rand(2, generator=g).to(dev)
    empty = torch.zeros(2, 3, 0, 5, device=dev)
    gi, gL, gR, gH = ops.curl_layer_backward(empty, None, L, R, Hk, empty, greg, flags=ops.F_PWL)
    assert gi.shape == empty.shape
    # the regulariser's share alone: what a zero output gradient gives on any image
    z = torch.rand(2, 3, 4, 4, device=dev)
    _, zL, zR, zH = ops.curl_layer_backward(z, None, L, R, Hk, torch.zeros_like(z), greg, flags=ops.F_PWL)
    for a, b in ((gL, zL), (gR, zR), (gH, zH)):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9)
    # a full 1500 x 1000 frame, against float64 autograd
    img = torch.rand(1, 3, 1000, 1500, generator=g)
    L1, R1, H1 = (smooth_knots(1, n, 16, g) for n in (3, 3, 4))
    gout = torch.randn(1, 3, 1000, 1500, generator=g)
    gi, gL, gR, gH = ops.curl_layer_backward(img.to(dev), None, L1.to(dev), R1.to(dev), H1.to(dev), gout.to(dev),
                                             flags=ops.F_PWL)
    out, wi, wL, wR, wH = oracle_grads(img.numpy(), None, L1.numpy(), R1.numpy(), H1.numpy(), gout.numpy(), np.zeros(1))
    _, wi32, *w32 = oracle_grads(img.numpy(), None, L1.numpy(), R1.numpy(), H1.numpy(), gout.numpy(), np.zeros(1),
                                 torch.float32)
    check_image(gi.cpu().numpy(), wi, wi32, "frame")
    for got, want, want32 in ((gL, wL, w32[0]), (gR, wR, w32[1]), (gH, wH, w32[2])):
        check_knots(got.cpu().numpy(), want, want32, "frame")


def test_curl_layer_paper_pwl_trains(dev):
    from curl_amd import model
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(8)
    B, H, W = 4, 64, 96
    img = torch.rand(B, 3, H, W, generator=g).to(dev)
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.1).to(dev)
    layer = model.CURLLayer(paper_pwl=True).to(dev)
    k_true = [smooth_knots(B, n, 16, g, amp=0.4).to(dev) for n in (3, 3, 4)]
    with torch.no_grad():
        target, _ = layer(img, mask, *k_true)
    k = [torch.nn.Parameter(torch.zeros(B, n * 16, device=dev)) for n in (3, 3, 4)]
    # under grad: a grad_fn, and the forward's bits are the no-grad call's
    out, reg = layer(img, mask, *k)
    assert out.grad_fn is not None and reg.grad_fn is not None
    with torch.no_grad():
        out0, reg0 = layer(img, mask, *k)
    assert torch.equal(out, out0) and torch.equal(reg, reg0)
    opt = torch.optim.Adam(k, lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        out, reg = layer(img, mask, *k)
        loss = ((out - target) ** 2).mean() + 1e-6 * reg.mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] <= 0.5 * losses[0], losses


def test_gcurlnet_paper_pwl_with_target_is_refused(dev):
    from curl_amd import model
    torch.manual_seed(1)
    net = model.GCURLNet(backbone=model.CurveEncoder(num_outputs=160, width=0.25, num_features=64), paper_pwl=True).to(dev)
    img = torch.rand(2, 3, 32, 32, device=dev)
    with pytest.raises(ValueError, match="paper_pwl"):
        net(img, None, target=img, criterion=model.CURLLoss(ssim_window_size=5).to(dev))
    out, reg = net(img, None)  # without target: the PWL layer, under grad
    out.mean().backward()
    assert out.grad_fn is not None and any(p.grad is not None for p in net.backbone.parameters())
