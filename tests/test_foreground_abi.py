"""The foreground-aware byte entries (include/curl_hip_fg.h): declared in a header that compiles as C99 and C++17, exported,
bound from _lib.SIGNATURES_FG beside the three unchanged tables, every argument error a return code with its text before any
HIP call (fake device pointers, no device needed)."""
import ctypes
import re
import subprocess

import pytest

from conftest import ROOT

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
NAMES = {"curl_trispace_fwd_fg_u8hwc": 11, "curl_layer_fwd_fg_u8hwc": 18}
TRI, LAYER = "curl_trispace_fwd_fg_u8hwc", "curl_layer_fwd_fg_u8hwc"


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl = dict(_declared("curl_hip_fg.h"))
    assert set(decl) == set(_lib.SIGNATURES_FG) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_FG[name][1]) == n, name
        fn = getattr(lib, name)  # exported
        assert fn.restype is _lib.SIGNATURES_FG[name][0] and list(fn.argtypes) == _lib.SIGNATURES_FG[name][1]  # bound by load()
    # the other three tables are still exactly their headers
    assert set(_lib.SIGNATURES) == {n for n, _ in _declared("curl_hip.h")}
    assert set(_lib.SIGNATURES_GRAD) == {n for n, _ in _declared("curl_hip_grad.h")}
    assert set(_lib.SIGNATURES_VIEW) == {n for n, _ in _declared("curl_hip_view.h")}
    assert not set(NAMES) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_GRAD) | set(_lib.SIGNATURES_VIEW))
    assert lib.curl_version() >= 115


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_fg.h"\n'
                   "int main(void) {\n"
                   "  if (curl_trispace_fwd_fg_u8hwc(0, 3, 0, 0, 0, 1, 8, 8, 126, 0, 0) != CURL_E_NULL) return 2;\n"
                   "  return curl_layer_fwd_fg_u8hwc(0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8, 8, CURL_K_UNEVEN(16, 14), 16, 16, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def _p(n):
    return ctypes.c_void_p(n << 20)


def _tri(**kw):
    a = dict(img=_p(1), channels=3, coeffs=_p(2), fg=_p(3), out=_p(4), B=1, H=8, W=8, nc=126, flags=0)
    a.update(kw)
    return [a[k] for k in ("img", "channels", "coeffs", "fg", "out", "B", "H", "W", "nc", "flags")] + [None]


def _layer(lib, **kw):
    a = dict(img=_p(1), channels=3, rawL=_p(2), rawR=_p(3), rawH=_p(4), fg=_p(5), out=_p(6), reg=_p(7), ws=_p(8), ws_bytes=None,
             B=1, H=8, W=8, Kl=16, Kr=16, Kh=16, flags=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.curl_workspace_bytes(max(a["B"], 1), 160)
    return [a[k] for k in ("img", "channels", "rawL", "rawR", "rawH", "fg", "out", "reg", "ws", "ws_bytes", "B", "H", "W", "Kl", "Kr",
                           "Kh", "flags")] + [None]


# what both entries refuse alike
COMMON = [
    (dict(fg=None), E_MASK, b"fg_mask"),
    (dict(channels=2), E_SHAPE, b"channels"), (dict(channels=5), E_SHAPE, b"channels"), (dict(channels=0), E_SHAPE, b"channels"),
    (dict(channels=1), E_SHAPE, b"channels"),
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x4), E_FLAGS, b"flag"), (dict(flags=0x400000), E_FLAGS, b"flag"),
    (dict(flags=0x80000000), E_FLAGS, b"flag"),
    (dict(img=None), E_NULL, b"NULL"), (dict(out=None), E_NULL, b"NULL"),
    (dict(B=0), E_SHAPE, b"positive"), (dict(H=0), E_SHAPE, b"positive"), (dict(W=-1), E_SHAPE, b"positive"),
    (dict(B=65536), E_SHAPE, b"65535"), (dict(H=1 << 16, W=(1 << 14) + 1), E_SHAPE, b"2^30"),
]


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(coeffs=None), E_NULL, b"coeffs"),
    (dict(nc=125), E_KNOTS, b"num_coeffs"), (dict(nc=0), E_KNOTS, b"num_coeffs"), (dict(nc=56), E_KNOTS, b"num_coeffs"),
    (dict(nc=56 | (2 << 16)), E_KNOTS, b"order"), (dict(nc=35 | (5 << 16)), E_KNOTS, b"order"),
    (dict(coeffs=ctypes.c_void_p((2 << 20) + 4)), E_SHAPE, b"8-byte"),
    (dict(coeffs=ctypes.c_void_p((2 << 20) + 2), nc=35), E_SHAPE, b"4-byte"),
])
def test_trispace_argument_errors_are_codes(lib, kw, code, word):
    assert lib.curl_trispace_fwd_fg_u8hwc(*_tri(**kw)) == code, kw
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(rawL=None), E_NULL, b"rawL/rawR/rawH"), (dict(rawR=None), E_NULL, b"rawL/rawR/rawH"), (dict(rawH=None), E_NULL, b"rawL/rawR/rawH"),
    (dict(Kl=1), E_KNOTS, b"knots per curve"), (dict(Kr=300), E_KNOTS, b"knots per curve"), (dict(Kh=-1), E_KNOTS, b"knots per curve"),
    (dict(Kh=16 | (17 << 16)), E_KNOTS, b"last curve"),
    (dict(ws=None), E_WORKSPACE, b"NULL"), (dict(ws=ctypes.c_void_p((8 << 20) + 4)), E_WORKSPACE, b"16-byte"),
    (dict(ws_bytes=8), E_WORKSPACE, b"too small"),
])
def test_layer_argument_errors_are_codes(lib, kw, code, word):
    assert lib.curl_layer_fwd_fg_u8hwc(*_layer(lib, **kw)) == code, kw
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


def test_python_surface_exists():
    """ops and infer carry the new capability (their GPU behaviour: tests/test_gpu_foreground.py)."""
    import inspect
    from curl_amd import infer, ops
    assert list(inspect.signature(ops.trispace_foreground_u8hwc).parameters) == ["img_u8", "coeffs", "fg_mask"]
    assert list(inspect.signature(ops.curl_layer_foreground_u8hwc).parameters) == ["img_u8", "L", "R", "H", "fg_mask"]
    assert inspect.signature(infer.enhance).parameters["foreground"].default is False
    import torch
    with pytest.raises(RuntimeError):  # no CPU fallback
        ops.trispace_foreground_u8hwc(torch.zeros(1, 4, 4, 4, dtype=torch.uint8), torch.zeros(1, 3, 3, 126), torch.zeros(1, 4, 4, dtype=torch.uint8))
