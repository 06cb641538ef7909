"""The encoder view's entry points (include/curl_hip_view.h): declared in a header that compiles as C99 and C++17, exported,
bound from _lib.SIGNATURES_VIEW beside the two unchanged tables, every argument error a return code with its text before any
HIP call (fake device pointers, no device needed) -- and the plan, which is built on the host: its geometry against the two
torchvision rules and its coefficient tables against a float64 restatement of Pillow's routine (encoder_view_cases.py),
integer for integer."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import encoder_view_cases as cases
from conftest import ROOT

E_NULL, E_SHAPE, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -4, -5, -6
NAMES = {"curl_encoder_view_plan_bytes": 3, "curl_encoder_view_plan": 5, "curl_encoder_view_u8hwc": 13}
HEADER_INTS = 16
STAMP = 0x43565031


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl = dict(_declared("curl_hip_view.h"))
    assert set(decl) == set(_lib.SIGNATURES_VIEW) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_VIEW[name][1]) == n, name
        fn = getattr(lib, name)  # exported
        assert fn.restype is _lib.SIGNATURES_VIEW[name][0] and list(fn.argtypes) == _lib.SIGNATURES_VIEW[name][1]  # bound by load()
    # the other two tables are still exactly their headers
    assert set(_lib.SIGNATURES) == {n for n, _ in _declared("curl_hip.h")}
    assert set(_lib.SIGNATURES_GRAD) == {n for n, _ in _declared("curl_hip_grad.h")}
    assert not set(NAMES) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_GRAD))
    assert lib.curl_version() >= 114


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_view.h"\n'
                   "int main(void) {\n"
                   "  int plan[4];\n"
                   "  if (curl_encoder_view_plan_bytes(8, 8, CURL_VIEW_SIZE_MIN) == 0) return 2;\n"
                   "  if (curl_encoder_view_plan(8, 8, CURL_VIEW_SIZE_MAX + CURL_VIEW_MAX_SHRINK, plan, sizeof plan) != CURL_E_SHAPE) return 3;\n"
                   "  return curl_encoder_view_u8hwc(0, 3, 0, 0, 0, 0, 0, 1, 8, 8, CURL_VIEW_SIZE_DEFAULT, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def _args(lib, **kw):
    a = dict(img=ctypes.c_void_p(1 << 20), channels=3, mask=ctypes.c_void_p(2 << 20), plan=ctypes.c_void_p(3 << 20), plan_bytes=None,
             view=ctypes.c_void_p(4 << 20), mview=ctypes.c_void_p(5 << 20), B=1, H=40, W=56, size=32, flags=0)
    a.update(kw)
    if a["plan_bytes"] is None:
        a["plan_bytes"] = max(lib.curl_encoder_view_plan_bytes(a["H"], a["W"], a["size"]), 64)
    return [a[k] for k in ("img", "channels", "mask", "plan", "plan_bytes", "view", "mview", "B", "H", "W", "size", "flags")] + [None]


@pytest.mark.parametrize("kw,code,word", [
    (dict(img=None), E_NULL, b"NULL"), (dict(view=None), E_NULL, b"NULL"), (dict(plan=None), E_NULL, b"plan_dev"),
    (dict(channels=2), E_SHAPE, b"channels"), (dict(channels=5), E_SHAPE, b"channels"), (dict(channels=1), E_SHAPE, b"channels"),
    (dict(size=7), E_SHAPE, b"8 .. 1024"), (dict(size=1025), E_SHAPE, b"8 .. 1024"), (dict(size=0), E_SHAPE, b"8 .. 1024"),
    (dict(H=513, W=600, size=8), E_SHAPE, b"exceeds 64"), (dict(H=3000, W=2049, size=32), E_SHAPE, b"exceeds 64"),
    (dict(plan_bytes=64), E_WORKSPACE, b"too small"), (dict(plan_bytes=0), E_WORKSPACE, b"too small"),
    (dict(plan=ctypes.c_void_p((3 << 20) + 2)), E_WORKSPACE, b"4-byte"),
    (dict(mask=None), E_MASK, b"both"), (dict(mview=None), E_MASK, b"both"),
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x4), E_FLAGS, b"flag"), (dict(flags=0x80000000), E_FLAGS, b"flag"),
    (dict(B=0), E_SHAPE, b"positive"), (dict(H=0), E_SHAPE, b"positive"), (dict(W=-1), E_SHAPE, b"positive"),
    (dict(B=65536), E_SHAPE, b"65535"), (dict(H=1 << 16, W=(1 << 14) + 1, size=1024), E_SHAPE, b"2^30"),
])
def test_argument_errors_are_codes(lib, kw, code, word):
    assert lib.curl_encoder_view_u8hwc(*_args(lib, **kw)) == code, kw
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


def test_plan_argument_errors(lib):
    n = lib.curl_encoder_view_plan_bytes(40, 56, 32)
    buf = np.zeros(n // 4 + 2, dtype=np.int32)
    assert n == 4 * (HEADER_INTS + 32 * ((2 + 5) + (2 + 5)))  # 40x56 -> 32: scale 1.25 on both axes, ksize 5
    assert lib.curl_encoder_view_plan(40, 56, 32, None, n) == E_NULL and b"NULL" in lib.curl_last_error()
    assert lib.curl_encoder_view_plan(40, 56, 32, buf.ctypes.data, n - 1) == E_WORKSPACE and b"too small" in lib.curl_last_error()
    assert lib.curl_encoder_view_plan(40, 56, 32, buf.ctypes.data + 1, n) == E_WORKSPACE and b"4-byte" in lib.curl_last_error()
    assert lib.curl_encoder_view_plan(40, 56, 7, buf.ctypes.data, n) == E_SHAPE and b"8 .. 1024" in lib.curl_last_error()
    assert lib.curl_encoder_view_plan(0, 56, 32, buf.ctypes.data, n) == E_SHAPE and b"positive" in lib.curl_last_error()
    assert lib.curl_encoder_view_plan(2049, 3000, 32, buf.ctypes.data, 1 << 20) == E_SHAPE and b"exceeds 64" in lib.curl_last_error()
    for shape in ((0, 56, 32), (40, 56, 7), (40, 56, 1025), (513, 600, 8)):
        assert lib.curl_encoder_view_plan_bytes(*shape) == 0, shape
    assert lib.curl_encoder_view_plan_bytes(512, 575, 8) > 0  # 64x exactly; the long axis at 71.9x, ksize 145
    buf[-2:] = 77
    assert lib.curl_encoder_view_plan(40, 56, 32, buf.ctypes.data, n) == 0
    assert list(buf[-2:]) == [77, 77] and buf[0] == STAMP  # nothing past the size it names


def _plan(lib, H, W, size):
    n = lib.curl_encoder_view_plan_bytes(H, W, size)
    assert n > 0 and n % 4 == 0, (H, W, size)
    buf = np.full(n // 4, -1, dtype=np.int32)
    assert lib.curl_encoder_view_plan(H, W, size, buf.ctypes.data, n) == 0, lib.curl_last_error()
    return buf


def _tables(plan, size):
    """-> (header dict, X rows [size, 2 + ksize_x], Y rows [size, 2 + ksize_y])"""
    h = dict(zip(("stamp", "H", "W", "size", "ow", "oh", "top", "left", "ksize_x", "ksize_y"), plan[:10].tolist()))
    assert h["stamp"] == STAMP and not plan[10:HEADER_INTS].any()
    nx = size * (2 + h["ksize_x"])
    assert plan.size == HEADER_INTS + nx + size * (2 + h["ksize_y"])
    return h, plan[HEADER_INTS:HEADER_INTS + nx].reshape(size, -1), plan[HEADER_INTS + nx:].reshape(size, -1)


@pytest.mark.parametrize("out", [16, 32, 320])
def test_plan_coefficients_are_the_float64_restatement(lib, out):
    """Every axis length 1..700 against out: a square image has that axis twice, uncropped."""
    for n_in in range(1, 701):
        h, X, Y = _tables(_plan(lib, n_in, n_in, out), out)
        want = cases.axis_rows(n_in, out)
        assert h["ksize_x"] == h["ksize_y"] == cases.axis_ksize(n_in, out) and (h["top"], h["left"]) == (0, 0), n_in
        assert np.array_equal(X, want) and np.array_equal(Y, want), (n_in, out, np.argwhere(X != want)[:4])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_plan_of_the_cases_is_the_cropped_tables(lib, name):
    H, W, size = cases.CASES[name][:3]
    h, X, Y = _tables(_plan(lib, H, W, size), size)
    ow, oh, top, left = cases.view_geometry(H, W, size)
    assert (h["H"], h["W"], h["size"], h["ow"], h["oh"], h["top"], h["left"]) == (H, W, size, ow, oh, top, left)
    assert np.array_equal(X, cases.axis_rows(W, ow, left, size)) and np.array_equal(Y, cases.axis_rows(H, oh, top, size))


@pytest.mark.parametrize("size", [16, 32, 320])
def test_plan_geometry_is_torchvisions(lib, size):
    """The two size rules over short sides 1..700 (as far as the 64x limit admits) and long sides around them, both ways round;
    margins of every parity, so halves that round to even in both directions."""
    seen = set()
    for short in range(1, min(700, 64 * size) + 1):
        for long in {short, short + 1, short + 2, short + 3, (short * 3) // 2 + 1, 2 * short + 7, 5 * short + 2}:
            for H, W in ((short, long), (long, short)):
                got = _plan(lib, H, W, size)[:10].tolist()
                ow, oh, top, left = cases.view_geometry(H, W, size)
                assert got[1:8] == [H, W, size, ow, oh, top, left], (H, W, size, got)
                seen.add(((oh - size) % 4, (ow - size) % 4))
    assert {(0, 1), (0, 3), (1, 0), (3, 0)} <= seen
