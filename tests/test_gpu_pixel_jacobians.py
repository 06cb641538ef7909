"""The nine stand-alone backward entry points (kernels/stage_bwd.inc, curl_math_bwd.h) on the device, held to float64
Jacobian by pixel: tests/jacobian_check.py's protocol through ops.*_backward directly, three calls per case with one-hot
grad_out.  The inputs are the host-twin tests' (jacobian_check.case_references: built once, shared, left unchanged), and their
conditions are asserted from the oracle alone before a kernel is called: a content has at most 1 % of its pixels replaced and
no near-kink pixel left; an atlas is finite, holds >= 100 smooth and (where the operator has convention points) >= 100
decided-kink pixels and is less than half near-kink; knot Jacobians are judged on inputs without near-kink pixels."""
import pytest
import torch

import jacobian_check as JC
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


def shapes_of(kind):
    return (None,) if kind == "atlas" else tuple(JC.SHAPES.values())


def off_by_one_float(t, dev):
    """t on the device as a contiguous view one float into its storage: off the float4 grid, the scalar kernels."""
    base = torch.zeros(1 + t.numel(), device=dev)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def device_jacobian(ops, dev, ref, x=None, flags=0, need_grad_img=True):
    """The Jacobian (and the knot Jacobian) of ref.op at ref.x from three one-hot calls of ops.<op>_backward."""
    B, _, H, W = ref.x.shape
    x = ref.x.to(dev) if x is None else x
    fn = getattr(ops, ref.op + "_backward")
    if ref.op in JC.CONVERTERS:
        return JC.one_hot_jacobian(lambda go: fn(x, go.to(dev)).cpu(), (B, H, W))
    raw = ref.raw.to(dev)
    head = (x, None if ref.mask is None else ref.mask.to(dev), raw) if ref.op in JC.STAGES else (x, raw)
    kw = {"flags": flags} if ref.op in JC.STAGES else {}

    def call(go):
        gi, gk = fn(*head, go.to(dev), None, need_grad_img, **kw)
        return (None if gi is None else gi.cpu()), gk.cpu()
    return JC.one_hot_jacobian(call, (B, H, W))


def misaligned_is_the_same_bits(ops, dev, ref, J, flags=0):
    """HW a multiple of 4 takes the float4 kernels; the same image through a view offset by one float takes the scalar ones:
    the image Jacobian must be the same bits, and the scalar kernels' knot Jacobian at this shape is held to the knot bound
    (on the input the knots are judged on: JC.knot_reference)."""
    if (ref.x.shape[2] * ref.x.shape[3]) % 4:
        return
    got = device_jacobian(ops, dev, ref, off_by_one_float(ref.x, dev), flags)
    Jm, Km = got if isinstance(got, tuple) else (got, None)
    assert torch.equal(Jm, J), (ref.label, "scalar path vs float4 path", float((Jm - J).abs().max()))
    if Km is not None:
        kref = JC.knot_reference(ref)
        if kref is not ref:
            Km = device_jacobian(ops, dev, kref, off_by_one_float(kref.x, dev), flags)[1]
        kref.check_knots(Km)


@pytest.mark.parametrize("kind", JC.CONTENTS)
@pytest.mark.parametrize("op", JC.CONVERTERS)
def test_converters(ops, dev, op, kind):
    """All four converters on random, wide, grid8 (tied rows) and the atlas; float4 shape (2, 4, 293), scalar shape
    (1, 37, 53), and the float4 shape through a view offset by one float (bit for bit the aligned result).  Input conditions:
    the module's, asserted by JC.case_references before the kernel runs."""
    for shape in shapes_of(kind):
        for ref in JC.case_references(op, kind, None, shape):
            J = device_jacobian(ops, dev, ref)
            print(JC.report(ref, ref.check(J), "gpu"))
            misaligned_is_the_same_bits(ops, dev, ref, J)


@pytest.mark.parametrize("kind", JC.CONTENTS)
@pytest.mark.parametrize("op", ["adjust_rgb", "adjust_lab", "adjust_hsv"])
def test_curve_ops(ops, dev, op, kind):
    """adjust_rgb / adjust_lab / adjust_hsv (the general, input-clamped form of adjust_hsv runs only from here): the same
    shapes and contents, knots at sigma 0.1, sigma 0.3 and the saturating shift (48 / 64 parameters), image and knot
    Jacobians, need_grad_img=False the same knot bits.  Input conditions: the module's, asserted before the kernel runs."""
    for kk in JC.knot_kinds(op, kind):
        for shape in shapes_of(kind):
            for ref in JC.case_references(op, kind, kk, shape):
                J, K = device_jacobian(ops, dev, ref)
                line = JC.report(ref, ref.check(J), "gpu")
                misaligned_is_the_same_bits(ops, dev, ref, J)
                _, K_only = device_jacobian(ops, dev, ref, need_grad_img=False)
                assert torch.equal(K_only, K), (ref.label, "need_grad_img=False moved the knot gradient")
                kref = JC.knot_reference(ref)  # (an atlas part: its near-kink pixels replaced, for the knot sums)
                if kref is not ref:
                    K = device_jacobian(ops, dev, kref)[1]
                print(line + f" | knots {kref.check_knots(K):.1e} of {kref.knot_bound()[0]:.1e}")


@pytest.mark.parametrize("op", list(JC.CURVE_OPS))
def test_uneven_chunk_split(ops, dev, op):
    """torch.chunk's shorter last curve (47 = 16 + 16 + 15, 61 = 16 x 3 + 13) on random content, both shapes: image and knot
    Jacobians.  Input conditions: the module's, asserted before the kernel runs."""
    n = 47 if JC.CURVE_OPS[op] == 3 else 61
    for shape in JC.SHAPES.values():
        for ref in JC.case_references(op, "random", "s03", shape, "none", n):
            J, K = device_jacobian(ops, dev, ref)
            print(JC.report(ref, ref.check(J), "gpu") + f" | knots {ref.check_knots(K):.1e} of {ref.knot_bound()[0]:.1e}")


@pytest.mark.parametrize("kind", JC.CONTENTS)
@pytest.mark.parametrize("mask_kind", JC.MASKS)
@pytest.mark.parametrize("op", JC.STAGES)
def test_stages(ops, dev, op, mask_kind, kind):
    """lab_stage / hsv_stage under no mask, a bool mask with the first 256 pixels of an image off (whole waves dead), the same
    as uint8, a soft float mask (no masked-out-is-zero claim; decided kinks judged as everywhere) and the bool mask with
    F_MASK_FIRST: shapes, contents and knots as for the curve ops, image and knot Jacobians, need_grad_img=False the same knot
    bits.  A masked-out pixel of a bool / uint8 mask must be exactly 0 (Reference.check).  Input conditions: the module's,
    asserted before the kernel runs."""
    flags = ops.F_MASK_FIRST if mask_kind == "bool_mask_first" else 0
    for kk in JC.knot_kinds(op, kind):
        for shape in shapes_of(kind):
            for ref in JC.case_references(op, kind, kk, shape, mask_kind):
                J, K = device_jacobian(ops, dev, ref, flags=flags)
                line = JC.report(ref, ref.check(J), "gpu")
                misaligned_is_the_same_bits(ops, dev, ref, J, flags)
                _, K_only = device_jacobian(ops, dev, ref, flags=flags, need_grad_img=False)
                assert torch.equal(K_only, K), (ref.label, "need_grad_img=False moved the knot gradient")
                kref = JC.knot_reference(ref)
                if kref is not ref:
                    K = device_jacobian(ops, dev, kref, flags=flags)[1]
                print(line + f" | knots {kref.check_knots(K):.1e} of {kref.knot_bound()[0]:.1e}")


@pytest.mark.parametrize("op", list(JC.CURVE_OPS))
def test_grad_reg_alone(ops, dev, op):
    """grad_out = 0 and a one-hot grad_reg, one call per image: the image gradient is exactly 0, the knot gradient is the
    regulariser's (float64 through the oracle) under the knot bound max(2e-5, 4 |K32 - K64| / max |K64|).  Input conditions:
    the random-content case's (the module's), asserted by JC.case_references before the kernel runs; the regulariser itself
    sees the knots alone."""
    shape = JC.SHAPES["float4"]
    ref = JC.case_references(op, "random", "s03", shape)[0]
    K64, K32 = JC.reg_knot_reference(op, ref.raw)
    scale = float(K64.abs().max())
    bound = max(JC.KNOT_FLOOR, JC.FACTOR32 * float((K32 - K64).abs().max()) / scale)
    fn = getattr(ops, op + "_backward")
    x, raw = ref.x.to(dev), ref.raw.to(dev)
    head = (x, None, raw) if op in JC.STAGES else (x, raw)
    for b in range(shape[0]):
        greg = torch.zeros(shape[0], device=dev)
        greg[b] = 1
        gi, gk = fn(*head, torch.zeros_like(x), greg)
        assert not bool(gi.any()), (op, "image gradient under grad_out = 0")
        want = torch.zeros_like(K64)
        want[b] = K64[b]
        r = float((gk.cpu().double() - want).abs().max()) / scale
        print(f"jacobian | {op} grad_reg e_{b} | knots {r:.1e} of {bound:.1e}")
        assert r <= bound, (op, b, r, bound)
