"""The stand-alone polynomial layer's backward entry point (curl_poly_layer_bwd_f32): declared, exported, bound, its scratch
size equal to the header's formula, and its argument errors reported as return codes through curl_last_error before any HIP
call (fake device pointers, no device needed)."""
import ctypes
import re

import pytest

from conftest import ROOT

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
NAME, SCRATCH = "curl_poly_layer_bwd_f32", "curl_poly_layer_bwd_scratch_bytes"


def test_declared_exported_and_bound():
    from curl_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/curl_hip.h").read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(curl_\w+)\s*\(", src, flags=re.M))
    for n in (NAME, SCRATCH):
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES[NAME][1]) == 13 and len(_lib.SIGNATURES[SCRATCH][1]) == 4
    assert lib.curl_version() >= 111


def _formula(B, H, W, V):
    """include/curl_hip.h: B * tiles * 3 * NC floats, tiles = ceil(H*W / (1024 * steps)), steps = B*H*W / 2^20 in [4, 16]"""
    steps = min(max(B * H * W >> 20, 4), 16)
    tiles = -(-H * W // (1024 * steps))
    return B * tiles * 3 * (126 if V == 5 else 35) * 4


def test_scratch_bytes():
    from curl_amd import _lib, ops
    lib = _lib.load()
    assert lib.curl_poly_layer_bwd_scratch_bytes(2, 20, 64, 3) == _formula(2, 20, 64, 3) == 2 * 1 * 105 * 4
    assert lib.curl_poly_layer_bwd_scratch_bytes(8, 1500, 1000, 5) == _formula(8, 1500, 1000, 5) == 8 * 134 * 378 * 4
    assert lib.curl_poly_layer_bwd_scratch_bytes(32, 256, 256, 3) == _formula(32, 256, 256, 3) == 32 * 16 * 105 * 4
    assert ops.poly_layer_bwd_tile(8, 1500, 1000) == 11264 and ops.poly_layer_bwd_tile(1, 3, 5) == 4096
    for bad in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, -1, 5), (1, 4, 4, 4), (1, 4, 4, 0)):
        assert lib.curl_poly_layer_bwd_scratch_bytes(*bad) == 0, bad


def _args(lib, B=1, H=4, W=4, V=5, **kw):
    fake = ctypes.c_void_p(4096)
    a = dict(img=fake, coeffs=fake, gout=fake, gimg=fake, gcoef=fake, scratch=fake,
             scratch_bytes=lib.curl_poly_layer_bwd_scratch_bytes(B, H, W, V), B=B, H=H, W=W, V=V, flags=0)
    a.update(kw)
    return [a[k] for k in ("img", "coeffs", "gout", "gimg", "gcoef", "scratch", "scratch_bytes", "B", "H", "W", "V", "flags")] + [None]


@pytest.mark.parametrize("kw,code,word", [
    (dict(img=None), E_NULL, b"NULL"), (dict(coeffs=None), E_NULL, b"coeffs"), (dict(gout=None), E_NULL, b"NULL"),
    (dict(gimg=None, gcoef=None), E_NULL, b"both NULL"),
    (dict(B=0), E_SHAPE, b"positive"), (dict(H=0), E_SHAPE, b"positive"), (dict(W=-1), E_SHAPE, b"positive"),
    (dict(V=4), E_SHAPE, b"num_variables"), (dict(V=126), E_SHAPE, b"num_variables"),
    (dict(B=65536, scratch_bytes=1 << 40), E_SHAPE, b"65535"),
    (dict(H=1 << 16, W=(1 << 14) + 1, scratch_bytes=1 << 40), E_SHAPE, b"2^30"),
    (dict(flags=0x4), E_FLAGS, b"flag"), (dict(flags=0x1), E_FLAGS, b"flag"),
    (dict(scratch=None), E_WORKSPACE, b"curl_poly_layer_bwd_scratch_bytes"),
    (dict(scratch=ctypes.c_void_p(4100)), E_WORKSPACE, b"misaligned"),
    (dict(scratch_bytes=4), E_WORKSPACE, b"curl_poly_layer_bwd_scratch_bytes"),
    # the image gradient alone needs no scratch -- but every other check still comes first
    (dict(gcoef=None, scratch=None, scratch_bytes=0, flags=0x2), E_FLAGS, b"flag"),
    (dict(gcoef=None, scratch=None, scratch_bytes=0, V=2), E_SHAPE, b"num_variables"),
])
def test_argument_errors_are_codes(kw, code, word):
    from curl_amd import _lib
    lib = _lib.load()
    assert lib.curl_poly_layer_bwd_f32(*_args(lib, **kw)) == code, kw
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())
