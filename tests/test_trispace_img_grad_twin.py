"""Host twin of the fused polynomial model's image gradient (tests/twin/trispace_img_grad_twin.cpp: curl_math_poly.h's
trispace_img_grad_n compiled for the host) against float64 autograd through the oracle, under the bound of
tests/trispace_img_grad_ref.py: K = 32 yardsticks, never more than 2e-4 of the largest gradient, every pixel outside the
exception set (8-bit content: every pixel).  A wrong or missing term is an error of 1e-2 and more on these inputs.
Largest twin / yardstick ratio on record: 3.04 (the one-pixel case; 1.9 otherwise) on random floats, 1.23 on 8-bit content."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from trispace_img_grad_ref import case, case_8bit, check
from twin_build import BUILD, COMMON, FLAVOURS, stale, twin_library

SOURCE = "trispace_img_grad_twin.cpp"


@pytest.fixture(scope="module", params=FLAVOURS)
def grad_twin(request):
    """The two flavours of conftest's `twin` fixture, for this twin's own source file."""
    return twin_library(SOURCE, request.param)


def _twin_grad(lib, img, c, w, residual_only):
    img, c, w = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (img, c, w))
    B, _, H, W = img.shape
    out = np.empty_like(img)
    P = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    assert lib.twin_trispace_img_grad(P(img), P(c), P(w), P(out), B, H, W, c.shape[-1], int(residual_only)) == 0
    return torch.from_numpy(out)


RANDOM = [(126, False, (2, 12, 20)), (126, True, (1, 37, 41)), (35, False, (3, 33, 65)), (35, True, (1, 1, 1))]


@pytest.mark.parametrize("nc,residual_only,shape", RANDOM, ids=[f"{n}-{'res' if r else 'img'}-{'x'.join(map(str, s))}" for n, r, s in RANDOM])
def test_twin_against_float64_autograd(grad_twin, nc, residual_only, shape):
    img, c, w, g64, yard, exc = case(nc, residual_only, shape)
    check(_twin_grad(grad_twin, img, c, w, residual_only), g64, yard, exc, f"twin nc={nc} residual_only={residual_only} {shape}")


@pytest.mark.parametrize("nc", [126, 35])
@pytest.mark.parametrize("residual_only", [False, True], ids=["img", "res"])
def test_twin_on_8bit_content(grad_twin, nc, residual_only):
    """Exact ties, exact zeros and clamp bounds: every pixel within the bound, no exception set."""
    img, c, w, g64, yard = case_8bit(nc, residual_only)
    check(_twin_grad(grad_twin, img, c, w, residual_only), g64, yard, None, f"twin 8-bit nc={nc} residual_only={residual_only}")


def test_twin_standalone_under_sanitizers():
    """The same source as a stand-alone program with its own main, built with AddressSanitizer and UBSan, run once."""
    exe = os.path.join(BUILD, "trispace_img_grad_twin_san")
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "twin", SOURCE)
    if stale(exe, src):
        subprocess.check_call(["g++", "-O1", "-g", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-DTWIN_MAIN"] + COMMON + ["-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("sum") == 4 and "runtime error" not in p.stderr
