"""The backward entry points of the stand-alone curve ops, converters and stages: declared, exported, bound, and their
argument errors reported as return codes through curl_last_error before any HIP call (no device needed)."""
import ctypes
import re

from conftest import ROOT

NEW = ["curl_adjust_rgb_bwd_f32", "curl_adjust_lab_bwd_f32", "curl_adjust_hsv_bwd_f32", "curl_rgb2lab_bwd_f32",
       "curl_lab2rgb_bwd_f32", "curl_rgb2hsv_bwd_f32", "curl_hsv2rgb_bwd_f32", "curl_lab_stage_bwd_f32",
       "curl_hsv_stage_bwd_f32"]
E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
F_PWL, F_WS_READY = 0x2, 0x40000


def test_declared_exported_and_bound():
    from curl_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/curl_hip.h").read(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(curl_\w+)\s*\(", src, flags=re.M))
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.curl_version() >= 109


def _stage_args(lib, name, B=1, H=4, W=4, K=16, **kw):
    """Valid-looking arguments of a curve / stage backward entry (fake device pointers: the call must fail before any use)."""
    fake = ctypes.c_void_p(4096)
    nc = 4 if "hsv" in name else 3
    a = dict(img=fake, mask=None, kind=0, raw=fake, gout=fake, greg=None, gimg=fake, graw=fake, ws=fake,
             ws_bytes=lib.curl_workspace_bytes(B, nc * K), scratch=fake, scratch_bytes=lib.curl_layer_bwd_scratch_bytes(B, H, W),
             B=B, H=H, W=W, K=K, flags=0)
    a.update(kw)
    head = [a["img"]] + ([a["mask"], a["kind"]] if "stage" in name else [])
    return head + [a["raw"], a["gout"], a["greg"], a["gimg"], a["graw"], a["ws"], a["ws_bytes"], a["scratch"],
                   a["scratch_bytes"], a["B"], a["H"], a["W"], a["K"], a["flags"], None]


def test_argument_errors_are_codes():
    from curl_amd import _lib
    lib = _lib.load()
    curve = [n for n in NEW if "adjust" in n or "stage" in n]
    for name in curve:
        fn = getattr(lib, name)
        for kw, code, word in ((dict(graw=None), E_NULL, b"grad_raw"), (dict(gout=None), E_NULL, b"NULL"),
                               (dict(raw=None), E_NULL, b"NULL"), (dict(B=0), E_SHAPE, b"positive"),
                               (dict(K=300), E_KNOTS, b"knots"), (dict(K=1), E_KNOTS, b"knots"),
                               (dict(flags=F_PWL), E_FLAGS, b"PWL"), (dict(flags=F_PWL | F_WS_READY), E_FLAGS, b"PWL"),
                               (dict(flags=0x1), E_FLAGS, b"flag"),
                               (dict(ws=None), E_WORKSPACE, b"workspace"), (dict(ws_bytes=16), E_WORKSPACE, b"small"),
                               (dict(ws=ctypes.c_void_p(4100)), E_WORKSPACE, b"aligned"),
                               (dict(scratch=None), E_WORKSPACE, b"scratch"), (dict(scratch_bytes=4), E_WORKSPACE, b"scratch"),
                               (dict(scratch=ctypes.c_void_p(4100)), E_WORKSPACE, b"misaligned"),
                               (dict(K=16 | (17 << 16)), E_KNOTS, b"last curve")):
            assert fn(*_stage_args(lib, name, **kw)) == code, (name, kw)
            assert word in lib.curl_last_error(), (name, kw, lib.curl_last_error())
    for name in ("curl_lab_stage_bwd_f32", "curl_hsv_stage_bwd_f32"):
        fn = getattr(lib, name)
        assert fn(*_stage_args(lib, name, kind=7, mask=ctypes.c_void_p(4096))) == E_MASK  # bad mask kind
        assert b"mask_kind must be" in lib.curl_last_error()
        assert fn(*_stage_args(lib, name, kind=1, mask=None)) == E_MASK  # kind set, pointer NULL
        assert b"mask pointer" in lib.curl_last_error()
    fake = ctypes.c_void_p(4096)
    for name in ("curl_rgb2lab_bwd_f32", "curl_lab2rgb_bwd_f32", "curl_rgb2hsv_bwd_f32", "curl_hsv2rgb_bwd_f32"):
        fn = getattr(lib, name)
        assert fn(None, fake, fake, 1, 4, 4, 0, None) == E_NULL
        assert fn(fake, None, fake, 1, 4, 4, 0, None) == E_NULL
        assert fn(fake, fake, None, 1, 4, 4, 0, None) == E_NULL and b"grad_in" in lib.curl_last_error()
        assert fn(fake, fake, fake, 1, 0, 4, 0, None) == E_SHAPE
        assert fn(fake, fake, fake, 1, 4, 4, F_PWL, None) == E_FLAGS
