"""Host twin of the encoder's view from image bytes (tests/twin/encoder_view_twin.cpp: curl_math_view.h compiled for the host,
the two passes run from the plan as the kernel runs them) against Pillow: every case of tests/golden/encoder_view.npz byte
for byte and, where Pillow is installed, a few hundred seeded random shapes against Pillow itself.  Equality is exact
everywhere: the arithmetic is integer and byte / 255 is correctly rounded.  Both flavours of twin_build.py: the coefficient
routine is float64 and must not be contracted (its one candidate, 0.5 + p * 2^22, happens to be exact either way: a power of
two times p -- the contracting flavour guards the routine against a change that is not)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import encoder_view_cases as cases
from conftest import ROOT
from twin_build import BUILD, COMMON, FLAVOURS, stale, twin_library

SOURCE = "encoder_view_twin.cpp"


@pytest.fixture(scope="module", params=FLAVOURS)
def view_twin(request):
    lib = twin_library(SOURCE, request.param)
    lib.twin_view_plan_ints.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


def twin_view(lib, img, mask, size):
    """-> (view_u8 [B,3,S,S], view f32, mask_u8 [B,S,S] | None, mask_view f32 [B,1,S,S] | None)"""
    img = np.ascontiguousarray(img)
    B, H, W, C = img.shape
    vu, v = np.empty((B, 3, size, size), np.uint8), np.empty((B, 3, size, size), np.float32)
    mu = mv = None
    if mask is not None:
        mask = np.ascontiguousarray(mask)
        mu, mv = np.empty((B, size, size), np.uint8), np.empty((B, 1, size, size), np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    assert lib.twin_encoder_view(P(img), C, P(mask), P(vu), P(v), P(mu), P(mv), B, H, W, size) == 0
    return vu, v, mu, mv


@pytest.mark.parametrize("name", list(cases.CASES))
def test_twin_reproduces_the_fixture(view_twin, golden, name):
    size = cases.CASES[name][2]
    img, mask = cases.inputs(name, golden)
    vu, v, mu, mv = twin_view(view_twin, img, mask, size)
    want, want_m = golden[f"{name}/view"], golden[f"{name}/mask_view"]
    assert np.array_equal(vu, want), np.argwhere(vu != want)[:4]
    assert np.array_equal(mu, want_m), np.argwhere(mu != want_m)[:4]
    assert np.array_equal(v, want.astype(np.float32) / np.float32(255.0))          # to_tensor: correctly rounded
    assert np.array_equal(mv[:, 0], (want_m > 0).astype(np.float32))
    vu2, v2, mu2, mv2 = twin_view(view_twin, img, None, size)                       # no mask: the same view
    assert mu2 is None and np.array_equal(vu2, vu) and np.array_equal(v2, v)


def test_twin_on_constant_images(view_twin):
    """All 0 and all 255: the rounded coefficients of a row need not sum to 2^22, the clip and the normalisation are exact."""
    for H, W, size in ((40, 56, 32), (641, 481, 32), (20, 27, 32), (97, 1003, 16)):
        for byte in (0, 255):
            img, mask = np.full((1, H, W, 3), byte, np.uint8), np.full((1, H, W), byte, np.uint8)
            vu, v, mu, mv = twin_view(view_twin, img, mask, size)
            assert (vu == byte).all() and (mu == byte).all()
            assert (v == np.float32(byte // 255)).all() and (mv == np.float32(byte // 255)).all()


def test_twin_plan_is_the_librarys(view_twin):
    """The twin and libcurlhip.so compile the same text: the same plan, integer for integer."""
    from curl_amd import _lib
    lib = _lib.load()
    for H, W, size in [c[:3] for c in cases.CASES.values()] + [(512, 575, 8), (333, 517, 320)]:
        n = view_twin.twin_view_plan_ints(H, W, size)
        assert n * 4 == lib.curl_encoder_view_plan_bytes(H, W, size) > 0
        a, b = np.zeros(n, np.int32), np.ones(n, np.int32)
        assert view_twin.twin_view_plan(H, W, size, a.ctypes.data_as(ctypes.c_void_p)) == 0
        assert lib.curl_encoder_view_plan(H, W, size, b.ctypes.data, n * 4) == 0
        assert np.array_equal(a, b), (H, W, size)


def test_twin_against_pillow_on_random_shapes(view_twin):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20240611)
    for i in range(300):
        size = int(rng.choice([8, 16, 32, 48]))
        short = int(rng.integers(max(1, size // 4), 6 * size))
        long = short + int(rng.integers(0, 3 * short + 2)) * int(rng.integers(0, 2))
        H, W = (short, long) if i % 2 else (long, short)
        img = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        mask = (rng.integers(1, 256, (1, H, W)) * (rng.random((1, H, W)) > 0.9)).astype(np.uint8)
        ow, oh, top, left = cases.view_geometry(H, W, size)
        box = (left, top, left + size, top + size)
        want = np.asarray(Image.fromarray(img[0]).resize((ow, oh), Image.BILINEAR).crop(box))
        want_m = np.asarray(Image.fromarray(mask[0]).resize((ow, oh), Image.BILINEAR).crop(box))
        vu, _, mu, _ = twin_view(view_twin, img, mask, size)
        assert np.array_equal(vu[0].transpose(1, 2, 0), want), (H, W, size)
        assert np.array_equal(mu[0], want_m), (H, W, size)


def test_twin_standalone_under_sanitizers():
    """The same source as a stand-alone program with its own main, built with AddressSanitizer and UBSan, run once."""
    exe = os.path.join(BUILD, "encoder_view_twin_san")
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "twin", SOURCE)
    if stale(exe, src):
        subprocess.check_call(["g++", "-O1", "-g", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-DTWIN_MAIN"] + COMMON + ["-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("sum") == 8 and "runtime error" not in p.stderr
