"""tests/jacobian_check.py on the CPU: the protocol against the host twin of the nine stand-alone backward entry points
(tests/twin/stage_twin.cpp, both flavours), the protocol refusing subtly wrong Jacobians made in Python from J64, and the
conditions on its own inputs (the replaced share of the contents, the class counts of the atlases)."""
import ctypes

import numpy as np
import pytest
import torch

import jacobian_check as JC
from test_twin_stage_bwd import CONVERTERS, _f32, _p, twin_stage
from test_twin_stage_bwd import check_image_grad as old_check_image_grad
from twin_build import FLAVOURS, twin_library

SHAPE = (2, 12, 41)  # the mutants' content: 984 pixels
ALL_OPS = list(JC.CONVERTERS) + list(JC.CURVE_OPS)


@pytest.fixture(scope="module", params=FLAVOURS)
def stage_twin(request):
    return twin_library("stage_twin.cpp", request.param)


def twin_jacobian(lib, op, x, raw=None, mask=None, binary=True):
    """The twin's Jacobian (and knot Jacobian) from three one-hot gout, greg = 0."""
    B, _, H, W = x.shape
    img = x.numpy()

    def call(go):
        go = go.numpy()
        if op in CONVERTERS:
            gi = np.zeros_like(img)
            lib.twin_convert_bwd(CONVERTERS[op], _p(_f32(img)), _p(_f32(go)), _p(gi), B, ctypes.c_long(H * W))
            return gi
        m = None if mask is None else mask.float().expand(B, 1, H, W).numpy()
        return twin_stage(lib, op, img, m, binary, raw.numpy(), go, np.zeros(B, np.float32))
    return JC.one_hot_jacobian(call, (B, H, W))


def case_list(op, mask_kind="none", n=None, contents=JC.CONTENTS):
    for kind in contents:
        for kk in JC.knot_kinds(op, kind):
            for shape in ((None,) if kind == "atlas" else JC.SHAPES.values()):
                yield from JC.case_references(op, kind, kk, shape, mask_kind, n)


@pytest.mark.parametrize("op", ALL_OPS)
def test_twin_meets_the_protocol(stage_twin, op):
    """All nine operators on every content and atlas, at the device tests' shapes (the same References).  Input conditions
    (JC.case_references; asserted from the oracle alone BEFORE the twin is called): contents have at most 1 % of their pixels
    replaced and no near-kink pixel left; atlases are finite, hold >= 100 smooth and (where the operator has convention points)
    >= 100 decided-kink pixels and are less than half near-kink; knot Jacobians are judged on inputs without near-kink pixels."""
    for ref in case_list(op):
        got = twin_jacobian(stage_twin, op, ref.x, ref.raw)
        J, K = got if isinstance(got, tuple) else (got, None)
        line = JC.report(ref, ref.check(J), "twin")
        if K is not None:
            kref = JC.knot_reference(ref)
            if kref is not ref:
                K = twin_jacobian(stage_twin, op, kref.x, kref.raw)[1]
            line += f" | knots {kref.check_knots(K):.1e} of {kref.knot_bound()[0]:.1e}"
        print(line)


@pytest.mark.parametrize("op", JC.STAGES)
@pytest.mark.parametrize("mask_kind", ["bool", "soft"])
def test_twin_stages_under_masks(stage_twin, op, mask_kind):
    """The stages under a bool mask (a masked-out pixel is exactly 0) and a soft one, with torch.chunk's uneven split.  Input
    conditions as above, asserted before the twin runs."""
    n = 47 if op == "lab_stage" else 61
    for ref in case_list(op, mask_kind, n, ("random", "grid8", "atlas")):
        J, K = twin_jacobian(stage_twin, op, ref.x, ref.raw, ref.mask, binary=mask_kind == "bool")
        line = JC.report(ref, ref.check(J), "twin")
        kref = JC.knot_reference(ref)  # (an atlas part: its near-kink pixels replaced, for the knot sums)
        if kref is not ref:
            K = twin_jacobian(stage_twin, op, kref.x, kref.raw, kref.mask, binary=mask_kind == "bool")[1]
        print(line + f" | knots {kref.check_knots(K):.1e} of {kref.knot_bound()[0]:.1e}")


# ---------------------------------------------------------------------------------------------------------------- mutants
def _old_accepts(ref, Jm, seed=0):
    """The earlier bar, check_image_grad (tests/test_twin_stage_bwd.py, = tests/test_gpu_stage_grads.py's) on the mutant under ITS
    protocol: a random cotangent, the float32 reference as want32."""
    w = torch.randn(ref.J64.shape[1:], generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    pull = lambda J: (J * w.permute(1, 0, 2, 3)[:, :, None]).sum(0).numpy()  # noqa: E731  sum_c w_c row_c
    try:
        old_check_image_grad(pull(Jm), pull(ref.J64), ref.label, pull(ref.J32))
    except AssertionError:
        return False
    return True


def _refused(ref, Jm):
    with pytest.raises(AssertionError, match="beyond tol"):
        ref.check(Jm)
    ref.check(ref.J64)  # (the unmutated Jacobian passes)


def test_mutant_one_entry_off_by_1e_4_on_the_dim_pixels():
    """The pixel's largest entry times 1 + 1e-4 where mag < 0.1 G: refused; the earlier helper accepts it.  On the two converters
    whose gradient spans more than a decade on random content (lab2rgb: dark pixels; rgb2hsv: near-grey ones).
    (Input condition, asserted first: such pixels exist.)"""
    for op in ("lab2rgb", "rgb2hsv"):
        ref = JC.decidable_inputs(op, JC.content("random", op, SHAPE, 3), label=op)
        dim = ref.mag < 0.1 * ref.G
        assert int(dim.sum()) >= 10, op
        flat = ref.J64.permute(1, 3, 4, 0, 2).reshape(*ref.mag.shape, 9)
        top = flat.abs().argmax(-1, keepdim=True)
        Jm = flat.scatter(-1, top, flat.gather(-1, top) * torch.where(dim, 1 + 1e-4, 1.0)[..., None])
        Jm = Jm.reshape(*ref.mag.shape, 3, 3).permute(3, 0, 4, 1, 2)
        _refused(ref, Jm)
        assert _old_accepts(ref, Jm), op


def _with_near_greys(x):
    """x with four near-grey pixels (channels 1e-6 apart: |d h / d x| ~ 1 / (6 df) ~ 1e5), as a full frame holds a few by
    chance: they set the tensor-wide maximum the earlier helper scales by."""
    x = x.clone()
    x[0, :, -1, -4:] = torch.tensor([[0.5, 0.5 + 2e-6, 0.5 + 1e-6]]).T
    return x


def test_mutant_rows_swapped_on_half_a_percent():
    """Rows 1 and 2 swapped on 0.5 % of the pixels: refused, for every converter.  The earlier helper sees a swap on plain random
    content (an error of the gradient's own size on 0.5 % of the pixels is above its quantile); it accepts the same swap as soon
    as the input holds a few near-grey pixels, whose hue gradient sets the maximum it scales by -- asserted on rgb2hsv, where
    the protocol here still refuses it."""
    def swapped(ref):
        pick = (torch.arange(ref.mag.numel()).reshape(ref.mag.shape) % 200 == 7) & ref.smooth  # every 200th pixel
        assert int(pick.sum()) >= 3
        return torch.where(pick[None, :, None], ref.J64[[0, 2, 1]], ref.J64)
    for op in JC.CONVERTERS:
        ref = JC.decidable_inputs(op, JC.content("random", op, SHAPE, 3), label=op)
        _refused(ref, swapped(ref))
    ref = JC.Reference("rgb2hsv", _with_near_greys(JC.content("random", "rgb2hsv", SHAPE, 3)), label="rgb2hsv with near-greys")
    assert ref.G > 1e4
    _refused(ref, swapped(ref))
    assert _old_accepts(ref, swapped(ref))


def _v_row_to_second_index(ref):
    """rgb2hsv at an exact tie of the maximum: d v / d x (row 2) moved from the first index attaining it to the second."""
    x = ref.x
    mx = x.amax(1, keepdim=True)
    at = (x == mx) & (x > 1e-9) & (x < 1)
    tie = at.sum(1) >= 2
    first = at.float().argmax(1)
    second = (at.float() - torch.nn.functional.one_hot(first, 3).permute(0, 3, 1, 2)).argmax(1)
    Jm = ref.J64.clone()
    row = torch.nn.functional.one_hot(second, 3).permute(0, 3, 1, 2).double()
    Jm[2] = torch.where(tie[:, None], row, Jm[2])
    return Jm, tie


def test_mutant_tie_gradient_to_the_second_index():
    """At exact ties of rgb2hsv's maximum the v row sent to the second index: refused on grid8 (ties on a third of the rows)
    and on the atlas.  The earlier helper accepts it on the same grid8 content once a few near-grey pixels set its scale, where the
    protocol here still refuses it.  (Input condition, asserted first: tied pixels exist and the mutant moves a 1 there.)"""
    grid = JC.content("grid8", "rgb2hsv", SHAPE, 3)
    refs = [JC.decidable_inputs("rgb2hsv", grid, label="rgb2hsv grid8"),
            JC.Reference("rgb2hsv", JC.atlas("rgb2hsv")[0][1], label="rgb2hsv atlas/edges"),
            JC.Reference("rgb2hsv", _with_near_greys(grid), label="rgb2hsv grid8 with near-greys")]
    for ref in refs:
        Jm, tie = _v_row_to_second_index(ref)
        assert int(tie.sum()) >= 20 and float((Jm[2] - ref.J64[2]).abs()[tie[:, None].expand_as(Jm[2])].max()) == 1.0
        _refused(ref, Jm)
    assert refs[2].G > 1e4 and _old_accepts(refs[2], _v_row_to_second_index(refs[2])[0])


def test_mutant_clamp_gate_closed_at_a_bound_reached_exactly():
    """hsv2rgb's atlas at v == 1 exactly (torch.clamp passes the gradient at its bounds): the v column zeroed there is refused.
    (Input condition, asserted first: such pixels exist, are decided kinks or smooth, and carry a v gradient.)"""
    (_, x), = JC.atlas("hsv2rgb")
    ref = JC.Reference("hsv2rgb", x, label="hsv2rgb atlas")
    at = (x[:, 2] == 1.0) & ~ref.near & (ref.J64[:, :, 2].abs().amax(0) > 0.5)
    assert int(at.sum()) >= 20
    Jm = ref.J64.clone()
    Jm[:, :, 2] = torch.where(at[None], torch.zeros(()).double(), Jm[:, :, 2])
    _refused(ref, Jm)


def test_mutant_srgb_linear_slope_above_the_threshold():
    """rgb2lab with the linear branch's slope 1 / 12.92 used above 0.04045 (the branches' slopes differ by 1.7 % there).
    Used up to 4e-6 above the threshold -- beyond h -- it is refused.  Used ONE ULP above it (3.7e-9) it cannot be: that input
    is a near kink by the protocol's own definition, J64(x - h e_k) is the linear branch's Jacobian and a candidate -- the same
    class as hsv2rgb's ramp ends, float32's to take.  Both outcomes are asserted."""
    thr = JC.f32(0.04045)
    above, far = JC.ulp(thr, 1), JC.f32(0.04045 + 4e-6)
    x = JC._product([above, far], [0.3, 0.6], [0.2, 0.7], "rgb2lab").repeat(1, 1, 1, 8)
    ref = JC.Reference("rgb2lab", x, label="rgb2lab about 0.04045")
    u = (ref.x[:, 0].double() + 0.055) / 1.055
    ratio = (1 / 12.92) / (2.4 / 1.055 * u ** 1.4)  # linear slope / power slope
    for value, refused in ((far, True), (above, False)):
        at = ref.x[:, 0] == value
        # (one ulp above: a near kink, or -- where column 0 is small beside the pixel's largest entry -- smooth with the jump in C)
        assert int(at.sum()) >= 8 and bool((ref.smooth[at] & (ref.C[at] < 10) if refused else ref.near[at] | (ref.C[at] > 100)).all())
        Jm = ref.J64.clone()
        Jm[:, :, 0] = torch.where(at[None], Jm[:, :, 0] * ratio[None], Jm[:, :, 0])
        if refused:
            _refused(ref, Jm)
        else:
            ref.check(Jm)


# ------------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("op", ALL_OPS)
def test_input_conditions(op):
    """The replaced share of every content (<= 1 %, nothing near a kink left) and the class counts of every atlas, from the
    oracle alone, at the shapes the device tests use and under every mask they use; grid8's tied rows are decided kinks of
    the operators that start with rgb2hsv."""
    for mask_kind in (JC.MASKS[:4] if op in JC.STAGES else ("none",)):
        for ref in case_list(op, mask_kind):
            assert "atlas" in ref.label or (int(ref.near.sum()) == 0 and int(ref.smooth.sum()) >= 100), ref.label
            assert "grid8" not in ref.label or mask_kind != "none" or op not in ("rgb2hsv", "hsv_stage") or int(ref.decided.sum()) >= 100, (ref.label, ref.counts())
