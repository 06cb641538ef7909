"""Backward of the stand-alone curve ops, converters and fused stages (curl_math_bwd.h: adjust3_bwd, adjust_hsv_bwd,
lab_stage_bwd, hsv_stage_bwd, the converters' *_bwd, knots_bwd) on a host twin of their own (tests/twin/stage_twin.cpp),
against float64 autograd through the oracle: random inputs, 8-bit values with channel ties, saturated inputs (clamps
active), bool and soft masks, knot counts torch.chunk splits unevenly."""
import ctypes

import numpy as np
import pytest
import torch

import curl_oracle as O
from twin_build import FLAVOURS, twin_library

TOL = 2e-4  # tests/test_twin_bwd.py's


@pytest.fixture(scope="module", params=FLAVOURS)
def stage_twin(request):
    """The two flavours of conftest's `twin` fixture, for this twin's own source file."""
    return twin_library("stage_twin.cpp", request.param)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


OPS = {"adjust_rgb": (0, 3), "adjust_lab": (0, 3), "adjust_hsv": (1, 4), "lab_stage": (2, 3), "hsv_stage": (3, 4)}
CONVERTERS = {"rgb2lab": 0, "lab2rgb": 1, "rgb2hsv": 2, "hsv2rgb": 3}


def twin_stage(lib, op, img, mask, binary, raw, gout, greg):
    code, nc = OPS[op]
    img, raw, gout, greg = _f32(img), _f32(raw), _f32(gout), _f32(greg)
    mask = None if mask is None else _f32(mask)
    B, _, H, W = img.shape
    N = raw.shape[1]
    K = -(-N // nc)
    gi, gr = np.zeros_like(img), np.zeros_like(raw)
    lib.twin_stage_bwd(code, _p(img), _p(mask), int(binary), _p(raw), _p(gout), _p(greg), _p(gi), _p(gr), B,
                       ctypes.c_long(H * W), K, N - (nc - 1) * K)
    return gi, gr


def oracle_stage(op, img, mask, raw, gout, greg):
    """float64 autograd through the oracle (the reference's eager ops restated)."""
    x = torch.from_numpy(np.asarray(img, np.float64)).requires_grad_(True)
    k = torch.from_numpy(np.asarray(raw, np.float64)).requires_grad_(True)
    m = None if mask is None else torch.from_numpy(np.asarray(mask, np.float64))
    if op in ("lab_stage", "hsv_stage"):
        m = torch.ones_like(x[:, :1]) if m is None else m
        fn = O.lab_stage if op == "lab_stage" else O.hsv_stage
        out, reg = fn(x, m, k, k.shape[1])
    else:
        out, reg = getattr(O, op)(x, k)
    ((out * torch.from_numpy(np.asarray(gout, np.float64))).sum() + (reg * torch.from_numpy(np.asarray(greg, np.float64))).sum()).backward()
    return x.grad.numpy(), k.grad.numpy()


def check_image_grad(got, want, what, want32=None):
    """want32: the same autograd in float32.  Where IT differs from float64 by more than the tolerance the pixel sits on a
    kink of the reference (8-bit hues of exactly 1/3, 2/3: the float32 rounding of 6h lands on a ramp's end) and either
    one-sided derivative is the reference's answer: such pixels (at most 1 %) are left out."""
    d = np.abs(np.asarray(got, np.float64) - want)
    scale = max(np.abs(want).max(), 1e-30)
    if want32 is not None:
        kink = np.abs(np.asarray(want32, np.float64) - want) > TOL * scale
        assert kink.mean() <= 0.01, (what, float(kink.mean()))
        d = d[~kink]
    assert np.quantile(d, 0.999) <= TOL * scale and d.max() <= 20 * TOL * scale, (what, float(d.max() / scale))


def check_knot_grad(got, want, what):
    r = float(np.abs(np.asarray(got, np.float64) - want).max() / max(1e-12, np.abs(want).max()))
    assert r <= TOL, (what, r)


def make_case(case, op, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = 2, 12, 20
    img = torch.rand(B, 3, H, W, generator=g)
    if case == "grid8":
        img = torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255  # ties on the 8-bit grid
        img[:, 1, :3] = img[:, 0, :3]
        img[:, 2, 3:6] = img[:, 1, 3:6]
    if case == "saturated":
        img = img * 1.6 - 0.3  # out-of-range inputs: clamps active
    mask, binary = None, True
    if case == "boolmask":
        mask = (torch.rand(B, 1, H, W, generator=g) > 0.3).float()
    if case == "softmask":
        mask, binary = torch.rand(B, 1, H, W, generator=g), False
    nc = OPS[op][1]
    n = nc * 16 - (5 if case == "uneven" else 0)  # torch.chunk: the last curve shorter (16, 16, 11 / 16, 16, 16, 11)
    raw = torch.randn(B, n, generator=g) * 0.3
    gout = torch.randn(B, 3, H, W, generator=g)
    greg = torch.rand(B, generator=g)
    return img.numpy(), None if mask is None else mask.numpy(), binary, raw.numpy(), gout.numpy(), greg.numpy()


CASES = ["random", "grid8", "saturated", "boolmask", "softmask", "uneven"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("op", list(OPS))
def test_stage_backward_vs_oracle_autograd(stage_twin, op, case):
    if case in ("boolmask", "softmask") and op not in ("lab_stage", "hsv_stage"):
        pytest.skip("the curve ops take no mask")
    img, mask, binary, raw, gout, greg = make_case(case, op, 100 + CASES.index(case))
    gi, gr = twin_stage(stage_twin, op, img, mask, binary, raw, gout, greg)
    wi, wr = oracle_stage(op, img, mask, raw, gout, greg)
    check_image_grad(gi, wi, (op, case, "img"))
    check_knot_grad(gr, wr, (op, case, "knots"))


@pytest.mark.parametrize("case", ["random", "grid8", "saturated"])
@pytest.mark.parametrize("name", list(CONVERTERS))
def test_converter_backward_vs_oracle_autograd(stage_twin, name, case):
    img, _, _, _, gout, _ = make_case(case, "adjust_rgb", 200 + 7 * CONVERTERS[name] + len(case))
    gi = np.zeros_like(img)
    stage_twin.twin_convert_bwd(CONVERTERS[name], _p(_f32(img)), _p(_f32(gout)), _p(gi), img.shape[0],
                                ctypes.c_long(img.shape[2] * img.shape[3]))
    want = {}
    for dt in (torch.float64, torch.float32):
        x = torch.from_numpy(img).to(dt).requires_grad_(True)
        (getattr(O, name)(x) * torch.from_numpy(gout).to(dt)).sum().backward()
        want[dt] = x.grad.numpy()
    check_image_grad(gi, want[torch.float64], (name, case), want[torch.float32])


def test_regulariser_only(stage_twin):
    """grad_out = 0: the knot gradient is the regulariser's alone, the image gradient exactly 0."""
    for op in OPS:
        img, mask, binary, raw, gout, greg = make_case("random", op, 7)
        gout = np.zeros_like(gout)
        gi, gr = twin_stage(stage_twin, op, img, mask, binary, raw, gout, greg)
        _, wr = oracle_stage(op, img, mask, raw, gout, greg)
        assert np.abs(gi).max() == 0
        check_knot_grad(gr, wr, op)
