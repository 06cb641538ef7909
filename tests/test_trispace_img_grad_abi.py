"""The fused polynomial model's image-gradient entry point (curl_trispace_bwd_img_f32, include/curl_hip_grad.h): exported,
declared in a header that compiles as C99 and C++17, bound from _lib.SIGNATURES_GRAD beside the unchanged SIGNATURES, and its
argument errors reported as return codes through curl_last_error before any HIP call (fake device pointers, no device
needed)."""
import ctypes
import re
import subprocess

import pytest

from conftest import ROOT

E_NULL, E_SHAPE, E_KNOTS, E_FLAGS = -1, -2, -3, -6
NAME = "curl_trispace_bwd_img_f32"


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


def test_exported_declared_and_bound():
    from curl_amd import _lib
    lib = _lib.load()
    grad = dict(_declared("curl_hip_grad.h"))
    assert set(grad) == set(_lib.SIGNATURES_GRAD) == {NAME}
    assert len(grad[NAME].split(",")) == len(_lib.SIGNATURES_GRAD[NAME][1]) == 10
    fn = getattr(lib, NAME)  # exported
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES_GRAD[NAME][1]  # and bound by load()
    # the first table is still exactly curl_hip.h (tests/test_abi.py holds it to that)
    assert set(_lib.SIGNATURES) == {n for n, _ in _declared("curl_hip.h")} and NAME not in _lib.SIGNATURES
    assert lib.curl_version() >= 112


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_grad.h"\n'
                   "int main(void) { return curl_trispace_bwd_img_f32(0, 0, 0, 0, 1, 1, 1, 35, CURL_F_RESIDUAL_ONLY, 0) == CURL_E_NULL ? 0 : 1; }\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def _args(**kw):
    a = dict(img=ctypes.c_void_p(1 << 20), coeffs=ctypes.c_void_p(2 << 20), gout=ctypes.c_void_p(3 << 20),
             gimg=ctypes.c_void_p(4 << 20), B=1, H=4, W=4, nc=126, flags=0)
    a.update(kw)
    return [a[k] for k in ("img", "coeffs", "gout", "gimg", "B", "H", "W", "nc", "flags")] + [None]


@pytest.mark.parametrize("kw,code,word", [
    (dict(img=None), E_NULL, b"NULL"), (dict(gout=None), E_NULL, b"NULL"), (dict(coeffs=None), E_NULL, b"coeffs"),
    (dict(gimg=None), E_NULL, b"grad_img"),
    (dict(nc=34), E_KNOTS, b"126 or 35"), (dict(nc=0), E_KNOTS, b"126 or 35"),
    (dict(coeffs=ctypes.c_void_p((2 << 20) + 4)), E_SHAPE, b"8-byte"),
    (dict(coeffs=ctypes.c_void_p((2 << 20) + 2), nc=35), E_SHAPE, b"4-byte"),
    (dict(gimg=ctypes.c_void_p(1 << 20)), E_SHAPE, b"alias"),      # grad_img == img
    (dict(gimg=ctypes.c_void_p(2 << 20)), E_SHAPE, b"alias"),      # grad_img == coeffs
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x2), E_FLAGS, b"flag"), (dict(flags=0x4 | 0x100), E_FLAGS, b"flag"),
    (dict(B=0), E_SHAPE, b"positive"), (dict(H=0), E_SHAPE, b"positive"), (dict(W=-1), E_SHAPE, b"positive"),
    (dict(B=65536), E_SHAPE, b"65535"), (dict(H=1 << 16, W=(1 << 14) + 1), E_SHAPE, b"2^30"),
])
def test_argument_errors_are_codes(kw, code, word):
    from curl_amd import _lib
    lib = _lib.load()
    assert getattr(lib, NAME)(*_args(**kw)) == code, kw
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())
