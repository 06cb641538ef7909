"""The knot-driven kernels off 16 knots per curve, on the device, against float64 on the rounded knots (tests/knot_paths.py:
the cases, the yardstick and the bounds; tests/test_knot_paths.py holds the host twins to the same bounds on the CPU).

What changes with the knot count and is compared here value by value: prep_image's 256-thread walk and 16-lane collapse
(forward out and reg, under every CURL_F_TUNE_PREP choice), knots_bwd_kernel's KNOT_OF decoding, knot_bwd5's clamped window, its
tail loop and its per-image row offset, stage_knots_bwd_kernel<NC>'s walk, and layer_pwl_knots_bwd_kernel with the PWL partial
rows.  The regulariser-only cotangent pins every knot gradient to its own knot, curve and image within 1e-6; the full cotangent
adds the pixel sums.  Run with -s for the worst error / bound ratio of every case."""
import pytest
import torch

import knot_paths as KP
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from curl_amd import _lib, ops
    _lib.load()
    return ops


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


LAYER_ROWS = [r for r in KP.case_table() if r[0] == "layer"]
STAGE_ROWS = [r for r in KP.case_table() if r[0] != "layer"]


@pytest.mark.parametrize("row", LAYER_ROWS, ids=KP.case_id)
def test_layer_vs_rounded_float64(ops, dev, row):
    from curl_amd import _lib
    ref, what = KP.reference(*row), KP.case_id(row)
    Y = ref.Y
    KP.check_conditions(Y, what)
    T = lambda t: None if t is None else t.to(dev)  # noqa: E731
    img, mask, raws = T(ref.img), T(ref.mask), [T(r) for r in ref.raws]
    # forward: curves collapsed where the launch size says, in a launch of their own, inside the streaming kernel -- the same bits
    fwd = [ops.curl_layer_forward(img, mask, *raws, flags=sel << _lib.F_TUNE_PREP_SHIFT, return_workspace=True)
           for sel in (0, 1, 2)]
    for other in fwd[1:]:
        assert torch.equal(other[0], fwd[0][0]) and torch.equal(other[1], fwd[0][1]), what
    out, reg, ws = fwd[0]
    r_fwd = KP.check_forward(Y, out, reg, what)
    # backward, with and without the image gradient, with the forward's workspace (CURL_F_WS_READY) and with its own knot prep
    zeros = torch.zeros_like(img)
    r_img = r_reg = r_full = 0.0
    for need_img in (True, False):
        for cotangent in ("regulariser", "full"):
            w, wr = (zeros, T(Y.greg.float())) if cotangent == "regulariser" else (T(ref.w), T(ref.wr))
            own = ops.curl_layer_backward(img, mask, *raws, w, wr, need_grad_img=need_img)
            ready = ops.curl_layer_backward(img, mask, *raws, w, wr, need_grad_img=need_img, workspace=ws)
            assert _same(own, ready), (what, cotangent, need_img)
            assert (own[0] is None) == (not need_img)
            if cotangent == "regulariser":
                r_reg = max(r_reg, KP.check_reg_knots(Y, own[1:], (what, need_img)))
                assert not need_img or float(own[0].abs().max()) == 0.0
                continue
            if need_img:
                r_img = KP.check_image_grad(Y, own[0], what)
            kn = own[1:]
            if bool(Y.jump.any()):  # both sides once more with the exception set masked out
                kn = ops.curl_layer_backward(img, T(Y.mask_ex), *raws, T(Y.w_ex), wr, need_grad_img=False)[1:]
            r_full = max(r_full, KP.check_full_knots(Y, kn, (what, need_img)))
    print(f"\n  gpu {what:28s} forward {r_fwd:.2f}  image gradient {r_img:.2f}  regulariser knots {r_reg / 1e-6:.3f}  "
          f"knots {r_full:.2f}  (delta {max(Y.delta):.1e}, exception set {int(Y.jump.sum())} px)")


def _stage(ops, op, img, mask, raw, w, wr):
    """Forward and backward of a stand-alone curve op or stage through the Python surface (its autograd node)."""
    x, k = img.clone().requires_grad_(True), raw.clone().requires_grad_(True)
    out, reg = getattr(ops, op)(x, mask, k) if op.endswith("stage") else getattr(ops, op)(x, k)
    ((out * w).sum() + (reg * wr).sum()).backward()
    return out.detach(), reg.detach(), x.grad, k.grad


@pytest.mark.parametrize("row", STAGE_ROWS, ids=KP.case_id)
def test_stage_operators_vs_rounded_float64(ops, dev, row):
    ref, what = KP.reference(*row), KP.case_id(row)
    Y, op = ref.Y, ref.op
    KP.check_conditions(Y, what)
    T = lambda t: None if t is None else t.to(dev)  # noqa: E731
    img, mask, raw, w, wr = T(ref.img), T(ref.mask), T(ref.raws[0]), T(ref.w), T(ref.wr)
    out, reg, g_img, g_raw = _stage(ops, op, img, mask, raw, w, wr)
    r_fwd = KP.check_forward(Y, out, reg, what)
    r_img = KP.check_image_grad(Y, g_img, what)
    if bool(Y.jump.any()):
        g_raw = _stage(ops, op, img, T(Y.mask_ex), raw, T(Y.w_ex), wr)[3]
    r_full = KP.check_full_knots(Y, [g_raw], what)
    _, _, z_img, z_raw = _stage(ops, op, img, mask, raw, torch.zeros_like(img), T(Y.greg.float()))
    r_reg = KP.check_reg_knots(Y, [z_raw], what)
    assert float(z_img.abs().max()) == 0.0
    print(f"\n  gpu {what:28s} forward {r_fwd:.2f}  image gradient {r_img:.2f}  regulariser knots {r_reg / 1e-6:.3f}  "
          f"knots {r_full:.2f}  (delta {max(Y.delta):.1e}, exception set {int(Y.jump.sum())} px)")


PWL_KNOTS = [(2, 2, 2), (3, 3, 3), (103, 103, 103), (256, 256, 256), (2, 256, 5)]


@pytest.mark.parametrize("K", PWL_KNOTS, ids=lambda K: "-".join(map(str, K)))
@pytest.mark.parametrize("mask_kind", ["none", "bool"])
@pytest.mark.parametrize("W", [20, 21])  # float4 path, scalar path (odd W)
def test_pwl_backward_vs_oracle_off_16_knots(ops, dev, K, mask_kind, W):
    """tests/test_gpu_pwl_grads.py's test_pwl_backward_vs_oracle, its checks unchanged, where layer_pwl_knots_bwd_kernel's
    window is clamped (2, 3), its partial rows are wider than a wavefront (103) and as wide as they get (256), and where the
    three segments' rows differ in width (2, 256, 5)."""
    from test_gpu_pwl_grads import MASKS, backward_vs_oracle
    backward_vs_oracle(ops, dev, K, mask_kind, False, W, 40 + sum(K) + W + MASKS.index(mask_kind))
