"""The fused layer's PWL backward entry point (curl_layer_pwl_bwd_f32): declared, exported, bound, its argument errors
reported as return codes through curl_last_error before any HIP call (fake device pointers, no device needed), and the
Python surface that refuses what it has no kernel for."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
F_EXACT_ORDER, F_PWL, F_WS_READY, F_MASK_FIRST = 0x1, 0x2, 0x40000, 0x400000
NAME = "curl_layer_pwl_bwd_f32"


def test_declared_exported_and_bound():
    from curl_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/curl_hip.h").read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(curl_\w+)\s*\(", src, flags=re.M))
    for n in (NAME, "curl_layer_pwl_bwd_scratch_bytes"):
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    # exactly curl_layer_bwd_f32's argument list
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["curl_layer_bwd_f32"]
    assert lib.curl_version() >= 110


def test_scratch_bytes():
    from curl_amd import _lib
    lib = _lib.load()
    # one row of n_knots floats per 256-pixel block (the scalar path's count: an upper bound)
    assert lib.curl_layer_pwl_bwd_scratch_bytes(2, 16, 20, 16, 16, 16) == 2 * 2 * 160 * 4
    assert lib.curl_layer_pwl_bwd_scratch_bytes(1, 1000, 1500, 256, 2, 16) == 5860 * (768 + 6 + 64) * 4
    for bad in ((0, 4, 4, 16, 16, 16), (1, 0, 4, 16, 16, 16), (1, 4, 4, 1, 16, 16), (1, 4, 4, 16, 257, 16)):
        assert lib.curl_layer_pwl_bwd_scratch_bytes(*bad) == 0, bad


def _args(lib, B=1, H=4, W=4, Kl=16, Kr=16, Kh=16, **kw):
    fake = ctypes.c_void_p(4096)
    n = 3 * (Kl & 0xffff) + 3 * (Kr & 0xffff) + 4 * (Kh & 0xffff)
    a = dict(img=fake, mask=None, kind=0, L=fake, R=fake, H_=fake, gout=fake, greg=None, gimg=fake, gL=fake, gR=fake, gH=fake,
             ws=fake, ws_bytes=lib.curl_workspace_bytes(B, n), scratch=fake,
             scratch_bytes=lib.curl_layer_pwl_bwd_scratch_bytes(B, H, W, Kl, Kr, Kh), B=B, H=H, W=W, Kl=Kl, Kr=Kr, Kh=Kh,
             flags=0)
    a.update(kw)
    return [a[k] for k in ("img", "mask", "kind", "L", "R", "H_", "gout", "greg", "gimg", "gL", "gR", "gH", "ws", "ws_bytes",
                           "scratch", "scratch_bytes", "B", "H", "W", "Kl", "Kr", "Kh", "flags")] + [None]


@pytest.mark.parametrize("kw,code,word", [
    (dict(L=None), E_NULL, b"rawL/rawR/rawH"), (dict(gH=None), E_NULL, b"grad_rawL/R/H"),
    (dict(img=None), E_NULL, b"NULL"), (dict(gout=None), E_NULL, b"NULL"),
    (dict(B=0), E_SHAPE, b"positive"), (dict(W=-1), E_SHAPE, b"positive"),
    (dict(Kl=1), E_KNOTS, b"knots per curve"), (dict(Kh=257), E_KNOTS, b"knots per curve"),
    (dict(Kr=16 | (8 << 16)), E_KNOTS, b"CURL_K_UNEVEN"),
    (dict(kind=7, mask=ctypes.c_void_p(4096)), E_MASK, b"mask_kind must be"), (dict(kind=1), E_MASK, b"mask pointer"),
    (dict(flags=F_PWL), E_FLAGS, b"flag bit"), (dict(flags=F_EXACT_ORDER), E_FLAGS, b"flag bit"),
    (dict(flags=F_WS_READY | 0x100), E_FLAGS, b"flag bit"), (dict(flags=0x20000), E_FLAGS, b"flag bit"),
    (dict(ws=None), E_WORKSPACE, b"workspace is NULL"), (dict(ws_bytes=16), E_WORKSPACE, b"too small"),
    (dict(ws=ctypes.c_void_p(4100)), E_WORKSPACE, b"aligned"),
    (dict(scratch=None), E_WORKSPACE, b"curl_layer_pwl_bwd_scratch_bytes"),
    (dict(scratch=ctypes.c_void_p(4100)), E_WORKSPACE, b"misaligned"),
    # the affine backward's scratch is too small here: the rows are n_knots wide, not 20
    (dict(scratch_bytes=4 * 20), E_WORKSPACE, b"curl_layer_pwl_bwd_scratch_bytes"),
])
def test_argument_errors_are_codes(kw, code, word):
    from curl_amd import _lib
    lib = _lib.load()
    assert lib.curl_layer_pwl_bwd_f32(*_args(lib, **kw)) == code, kw
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


def test_affine_backward_still_refuses_pwl():
    from curl_amd import _lib
    lib = _lib.load()
    a = _args(lib, flags=F_PWL)
    a[15] = lib.curl_layer_bwd_scratch_bytes(1, 4, 4)
    assert lib.curl_layer_bwd_f32(*a) == E_FLAGS


def test_gcurlnet_refuses_the_fused_loss_forward_with_pwl():
    from curl_amd import model
    torch.manual_seed(0)
    net = model.GCURLNet(backbone=model.CurveEncoder(num_outputs=160, width=0.25, num_features=64), paper_pwl=True).eval()
    assert net.curllayer.paper_pwl
    img = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError, match="paper_pwl"):
        net(img, None, target=img, criterion=None)


@pytest.mark.parametrize("argv,word", [(["--arch", "curl", "--paper_pwl", "--fused_forward"], "--fused_forward"),
                                       (["--arch", "trispace", "--paper_pwl"], "--arch curl")])
def test_train_refuses_paper_pwl_combinations(argv, word):
    from curl_amd import train
    with pytest.raises(SystemExit, match=word):
        train.main(argv)
