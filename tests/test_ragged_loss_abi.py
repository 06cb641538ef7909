"""The ragged CURLLoss entries (include/curl_hip_ragged_loss.h) without a device: the header compiles as C99 and C++17, the four
names are declared, exported and bound from _lib.SIGNATURES_RAGGED_LOSS beside the nine unchanged tables; the plan's limits,
its offsets against the op-0 curl_ragged_plan's, a three-image plan worked out by hand, the workspace query; every single-fault
argument list of curl_loss_ragged_u8hwc a return code with its word before any HIP call (fake device pointers);
ops.curl_loss_from_stats against the oracle in float64; and the host side of ops.loss_stats_u8hwc_ragged /
curl_loss_u8hwc_ragged, infer.enhance_and_evaluate_many and infer_dir --loss."""
import ctypes
import inspect
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ragged_loss_ref import LossReference, loss_formula, plan_by_hand
from ragged_msssim_ref import SHAPES as BATCH_SHAPES

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
PLAN_BYTES, PLAN, WS, ENTRY = ("curl_loss_ragged_plan_bytes", "curl_loss_ragged_plan", "curl_loss_ragged_workspace_bytes",
                               "curl_loss_ragged_u8hwc")
NAMES = {PLAN_BYTES: 1, PLAN: 6, WS: 1, ENTRY: 16}
HEADER_WORDS, DESC_WORDS, LEVEL_WORD, LEVEL_WORDS, TERMS_WORD, TERMS = 32, 64, 16, 8, 28, 5
STAMP, OP = 0x4C535231, 6
TABLES = {"SIGNATURES": "curl_hip.h", "SIGNATURES_GRAD": "curl_hip_grad.h", "SIGNATURES_VIEW": "curl_hip_view.h",
          "SIGNATURES_FG": "curl_hip_fg.h", "SIGNATURES_RAGGED": "curl_hip_ragged.h", "SIGNATURES_VIEW_RAGGED": "curl_hip_view_ragged.h",
          "SIGNATURES_RAGGED_FG": "curl_hip_ragged_fg.h", "SIGNATURES_RAGGED_SCORE": "curl_hip_ragged_score.h",
          "SIGNATURES_RAGGED_MSSSIM": "curl_hip_ragged_msssim.h"}


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl = dict(_declared("curl_hip_ragged_loss.h"))
    assert set(decl) == set(_lib.SIGNATURES_RAGGED_LOSS) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_RAGGED_LOSS[name][1]) == n, name
        fn = getattr(lib, name)  # exported
        assert fn.restype is _lib.SIGNATURES_RAGGED_LOSS[name][0] and list(fn.argtypes) == _lib.SIGNATURES_RAGGED_LOSS[name][1]
        twin = name.replace("curl_loss_", "curl_msssim_")  # the argument lists are the MS-SSIM entries'
        assert _lib.SIGNATURES_RAGGED_LOSS[name] == _lib.SIGNATURES_RAGGED_MSSSIM[twin]
    for table, header in TABLES.items():  # the nine existing tables still equal their headers
        assert set(getattr(_lib, table)) == {n for n, _ in _declared(header)}, table
    assert lib.curl_version() >= 121
    assert (_lib.LOSS_RAGGED_STAMP, _lib.LOSS_RAGGED_OP, _lib.LOSS_RAGGED_HEADER_WORDS, _lib.LOSS_RAGGED_DESC_WORDS,
            _lib.LOSS_RAGGED_LEVEL_WORD, _lib.LOSS_RAGGED_LEVEL_WORDS, _lib.LOSS_RAGGED_TERMS_WORD, _lib.LOSS_RAGGED_TERMS) == \
        (STAMP, OP, HEADER_WORDS, DESC_WORDS, LEVEL_WORD, LEVEL_WORDS, TERMS_WORD, TERMS)
    assert _lib.LOSS_RAGGED_STAMP != _lib.MSSSIM_RAGGED_STAMP
    hdr = open(f"{ROOT}/include/curl_hip_ragged_loss.h").read()
    for macro, value in (("STAMP", "0x4C535231"), ("OP", "6"), ("HEADER_WORDS", "32"), ("DESC_WORDS", "64"), ("LEVEL_WORD", "16"),
                         ("LEVEL_WORDS", "8"), ("TERMS_WORD", "28"), ("TERMS", "5")):
        assert re.search(rf"#define CURL_LOSS_RAGGED_{macro} {value}\b", hdr), macro
    assert "bytes written" in hdr.lower() or "BYTES" in hdr  # what is scored is said where it is declared


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_ragged_loss.h"\n'
                   "int main(void) {\n"
                   "  int hw[1] = {32};\n"
                   "  long long buf[(CURL_LOSS_RAGGED_HEADER_WORDS + CURL_LOSS_RAGGED_DESC_WORDS) / 2];\n"
                   "  if (curl_loss_ragged_plan_bytes(1) != sizeof buf) return 4;\n"
                   "  if (curl_loss_ragged_plan(1, hw, hw, 1, buf, sizeof buf) != CURL_OK) return 3;\n"
                   "  if (curl_loss_ragged_workspace_bytes(buf) == 0) return 2;\n"
                   "  return curl_loss_ragged_u8hwc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, buf, 0, 0, 11, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


# ------------------------------------------------------------------ the plan
def _plan(lib, shapes, has_mask=1, expect=0):
    B = len(shapes)
    hs, ws = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(2))
    nbytes = lib.curl_loss_ragged_plan_bytes(B)
    assert nbytes == 4 * (HEADER_WORDS + DESC_WORDS * B)
    buf = np.zeros(nbytes // 4 + 2, dtype=np.int32)
    assert buf.ctypes.data % 8 == 0
    rc = lib.curl_loss_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, has_mask, buf.ctypes.data, nbytes)
    assert rc == expect, (rc, lib.curl_last_error())
    return buf


def _msssim_plan(lib, shapes, has_mask):
    B = len(shapes)
    hs, ws = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(2))
    nbytes = lib.curl_msssim_ragged_plan_bytes(B)
    buf = np.zeros(nbytes // 4 + 2, dtype=np.int32)
    assert lib.curl_msssim_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, has_mask, buf.ctypes.data, nbytes) == 0
    return buf


def _op0_plan(lib, shapes, has_mask):
    B = len(shapes)
    hs, ws = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(2))
    cs = np.full(B, 3, dtype=np.int32)
    nbytes = lib.curl_ragged_plan_bytes(B, 0)
    buf = np.zeros(nbytes // 4 + 2, dtype=np.int32)
    assert lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, 0, buf.ctypes.data, nbytes) == 0
    return buf


def _i64(words, at):
    return int(np.ascontiguousarray(words[at:at + 2]).view(np.int64)[0])


def test_plan_limits(lib):
    assert lib.curl_loss_ragged_plan_bytes(0) == 0 and lib.curl_loss_ragged_plan_bytes(65536) == 0
    assert lib.curl_loss_ragged_plan_bytes(65535) == 4 * (HEADER_WORDS + DESC_WORDS * 65535)
    _plan(lib, [(32, 32)])
    _plan(lib, [(40, 36), (32, 40), (64, 31)], expect=E_SHAPE)  # an image 31 wide is refused and its index is named
    assert b"image 2" in lib.curl_last_error() and b"64x31" in lib.curl_last_error() and b">= 32" in lib.curl_last_error()
    _plan(lib, [(40, 36), (31, 40), (20, 31)], expect=E_SHAPE)  # the FIRST offending image
    assert b"image 1" in lib.curl_last_error() and b"31x40" in lib.curl_last_error()
    _plan(lib, [(32768, 32769)], expect=E_SHAPE)  # H*W > 2^30
    assert b"2^30" in lib.curl_last_error()
    _plan(lib, [(32768, 32768)])
    _plan(lib, [(0, 40)], expect=E_SHAPE)
    _plan(lib, [(40, -1)], expect=E_SHAPE)
    # 2048 images of 2^30 pixels are 2^31 level-0 tiles: one more workgroup than a launch's grid holds
    _plan(lib, [(32768, 32768)] * 2048, expect=E_SHAPE)
    assert b"grid" in lib.curl_last_error() and b"2^31" in lib.curl_last_error()
    one = np.array([32], dtype=np.int32)
    good = np.zeros(HEADER_WORDS + DESC_WORDS + 2, dtype=np.int32)
    nb = 4 * (HEADER_WORDS + DESC_WORDS)
    assert lib.curl_loss_ragged_plan(0, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data, nb) == E_SHAPE
    assert lib.curl_loss_ragged_plan(65536, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data, nb) == E_SHAPE
    assert lib.curl_loss_ragged_plan(1, None, one.ctypes.data, 1, good.ctypes.data, nb) == E_NULL
    assert lib.curl_loss_ragged_plan(1, one.ctypes.data, None, 1, good.ctypes.data, nb) == E_NULL
    assert lib.curl_loss_ragged_plan(1, one.ctypes.data, one.ctypes.data, 1, None, nb) == E_NULL
    assert lib.curl_loss_ragged_plan(1, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data, nb - 1) == E_WORKSPACE
    assert lib.curl_loss_ragged_plan(1, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data + 4, nb) == E_WORKSPACE


@pytest.mark.parametrize("has_mask", [1, 0])
def test_plan_offsets_are_the_op0_plans(lib, has_mask):
    """Every rgb_off / mask_off equals the out_off / mask_off of curl_ragged_plan for operator 0 and the same shape list, and
    the arena sizes its out / mask arena's: the arenas are RaggedBytes.pack's, and enhance_many's out arena can be passed as it is."""
    shapes = BATCH_SHAPES + [(33, 33), (32, 35)]  # odd pixel counts: padding between the images
    p, q = _plan(lib, shapes, has_mask), _op0_plan(lib, shapes, has_mask)
    assert _i64(p, 12) == _i64(q, 16) and _i64(p, 14) == _i64(q, 14) and (_i64(p, 14) > 0) == bool(has_mask)
    op0 = {int(q[32 + 16 * k + 1]): (_i64(q, 32 + 16 * k + 14), _i64(q, 32 + 16 * k + 12)) for k in range(len(shapes))}
    for i, (h, w) in enumerate(shapes):
        d = p[HEADER_WORDS + DESC_WORDS * i:HEADER_WORDS + DESC_WORDS * (i + 1)]
        assert (int(d[0]), int(d[1]), int(d[2])) == (i, h, w)
        assert (_i64(d, 4), _i64(d, 6)) == op0[i], i


@pytest.mark.parametrize("has_mask", [1, 0])
def test_a_plan_worked_out_by_hand(lib, has_mask):
    shapes = [(32, 32), (33, 47), (97, 129)]
    p = _plan(lib, shapes, has_mask)
    images, head = plan_by_hand(shapes, has_mask)
    # the figures themselves, not only the second implementation of the rule
    assert head["grid"] == [25, 6, 3, 3, 3] and head["pair0"] == [0, 25, 31, 34, 37]
    assert head["rgb_bytes"] == 45267 and head["mask_bytes"] == (15089 if has_mask else 0)
    assert head["partial_off"] == 39200 and head["terms_off"] == 39200 + 40 * 16 and head["ws_bytes"] == 39840 + 25 * 40
    assert [[(lv["h"], lv["w"]) for lv in img["levels"]] for img in images] == [
        [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], [(33, 47), (16, 23), (8, 11), (4, 5), (2, 2)],
        [(97, 129), (48, 64), (24, 32), (12, 16), (6, 8)]]
    assert [[lv["tiles"] for lv in img["levels"]] for img in images] == [[1, 1, 1, 1, 1], [4, 1, 1, 1, 1], [20, 4, 1, 1, 1]]
    assert [[lv["first"] for lv in img["levels"]] for img in images] == [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [5, 2, 2, 2, 2]]
    assert [img["rgb_off"] for img in images] == [0, 3072, 7728]
    assert [[lv["planes"] for lv in img["levels"]] for img in images] == [
        [0, 0, 2048, 2560, 2688], [0, 2720, 5664, 6368, 6528], [0, 6560, 31136, 37280, 38816]]  # two planes: 8 h w bytes a level
    # ... and the library's words
    assert (int(p[0]) & 0xffffffff, int(p[1]), int(p[2]), int(p[3]), int(p[4])) == (STAMP, 3, OP, has_mask, 6)
    assert [int(v) for v in p[5:10]] == head["grid"] and [int(v) for v in p[22:27]] == head["pair0"]
    assert (_i64(p, 12), _i64(p, 14), _i64(p, 16), _i64(p, 20)) == (head["rgb_bytes"], head["mask_bytes"], head["ws_bytes"], head["partial_off"])
    assert _i64(p, TERMS_WORD) == head["terms_off"]
    for i, img in enumerate(images):
        d = p[HEADER_WORDS + DESC_WORDS * i:HEADER_WORDS + DESC_WORDS * (i + 1)]
        assert (_i64(d, 4), _i64(d, 6)) == (img["rgb_off"], img["mask_off"])
        for l, lv in enumerate(img["levels"]):
            v = d[LEVEL_WORD + LEVEL_WORDS * l:LEVEL_WORD + LEVEL_WORDS * (l + 1)]
            assert [int(x) for x in v[:6]] == [lv["h"], lv["w"], lv["tiles_x"], lv["tiles"], lv["first"], lv["pair"]], (i, l)
            assert _i64(v, 6) == lv["planes"], (i, l)
    assert lib.curl_loss_ragged_workspace_bytes(p.ctypes.data) == head["ws_bytes"]
    # the MS-SSIM plan's twin: every word that means the same is equal; stamp, operator, hash, plane offsets and sizes differ
    q = _msssim_plan(lib, shapes, has_mask)
    same = [1, 3, 4] + list(range(5, 10)) + [12, 13, 14, 15] + list(range(22, 27))
    assert all(int(p[k]) == int(q[k]) for k in same) and int(p[0]) != int(q[0]) and int(p[2]) != int(q[2]) and _i64(p, 18) != _i64(q, 18)
    for i in range(len(shapes)):
        d, e = (x[HEADER_WORDS + DESC_WORDS * i:HEADER_WORDS + DESC_WORDS * (i + 1)] for x in (p, q))
        assert [int(v) for v in d[:8]] == [int(v) for v in e[:8]]
        for l in range(5):
            at = LEVEL_WORD + LEVEL_WORDS * l
            assert [int(v) for v in d[at:at + 6]] == [int(v) for v in e[at:at + 6]] and 3 * _i64(d, at + 6) == _i64(e, at + 6)
    # the hash covers (stamp, has_mask, B, every H, W)
    assert _i64(p, 18) != _i64(_plan(lib, shapes, 1 - has_mask), 18)
    assert _i64(p, 18) != _i64(_plan(lib, shapes[::-1], has_mask), 18) and _i64(p, 18) != _i64(_plan(lib, shapes[:2], has_mask), 18)
    assert _i64(p, 18) != _i64(_plan(lib, [(32, 32), (47, 33), (97, 129)], has_mask), 18)
    assert _i64(p, 18) == _i64(_plan(lib, shapes, has_mask), 18)


def test_workspace_bytes(lib):
    for has_mask in (0, 1):
        p = _plan(lib, BATCH_SHAPES, has_mask)
        _, head = plan_by_hand(BATCH_SHAPES, has_mask)
        assert lib.curl_loss_ragged_workspace_bytes(p.ctypes.data) == head["ws_bytes"] == _i64(p, 16)
        planes = sum(8 * (h >> l) * (w >> l) for h, w in BATCH_SHAPES for l in range(1, 5))
        assert head["partial_off"] >= planes
        assert head["ws_bytes"] == head["partial_off"] + 16 * sum(int(v) for v in p[5:10]) + 8 * TERMS * int(p[5])
    assert lib.curl_loss_ragged_workspace_bytes(None) == 0
    assert lib.curl_loss_ragged_workspace_bytes(np.zeros_like(p).ctypes.data) == 0
    bad = p.copy()
    bad[0] ^= 1
    assert lib.curl_loss_ragged_workspace_bytes(bad.ctypes.data) == 0
    other = p.copy()
    other[2] = 0
    assert lib.curl_loss_ragged_workspace_bytes(other.ctypes.data) == 0
    moved = p.copy()
    moved[TERMS_WORD] += 8
    assert lib.curl_loss_ragged_workspace_bytes(moved.ctypes.data) == 0
    # the plans of the other headers are no such plan, and this one is none of theirs
    assert lib.curl_loss_ragged_workspace_bytes(_op0_plan(lib, BATCH_SHAPES, 1).ctypes.data) == 0
    assert lib.curl_loss_ragged_workspace_bytes(_msssim_plan(lib, BATCH_SHAPES, 1).ctypes.data) == 0
    assert lib.curl_ragged_score_workspace_bytes(p.ctypes.data) == 0 and lib.curl_msssim_ragged_workspace_bytes(p.ctypes.data) == 0


# ------------------------------------------------------------------ the entry's argument lists
def _p(n, off=0):
    return ctypes.c_void_p((n << 20) + off)


SHAPES = [(40, 36), (33, 47)]


@pytest.fixture(scope="module")
def plans(lib):
    """name -> host plan words.  'zeros': no plan at all; 'stamp': one bit of the stamp wrong; 'op0': curl_ragged_plan's plan of
    operator 0; 'msssim': curl_msssim_ragged_plan's; 'operator': this header's plan with another operator word; 'shifted': four
    bytes off the 8-byte grid."""
    out = {"masks": _plan(lib, SHAPES, 1), "nomask": _plan(lib, SHAPES, 0), "op0": _op0_plan(lib, SHAPES, 1),
           "msssim": _msssim_plan(lib, SHAPES, 1)}
    out["zeros"] = np.zeros_like(out["masks"])
    out["stamp"] = out["masks"].copy()
    out["stamp"][0] ^= 1
    out["operator"] = out["masks"].copy()
    out["operator"][2] = 5
    shifted = np.zeros(out["masks"].size + 1, dtype=np.int32)
    shifted[1:] = out["masks"]
    out["shifted"] = shifted[1:]
    assert shifted[1:].ctypes.data % 8 == 4
    return out


def _args(plans, **kw):
    a = dict(a=_p(1), b=_p(2), mask=_p(3), stats=_p(4), ws=_p(6), plan="masks", host="plan", dev=_p(5), plan_bytes=None, window=11,
             flags=0, d_a=0, d_b=0, d_mask=0, d_stats=0, d_ws=0)
    a.update(kw)
    good = plans["masks"]
    host = plans[a["plan"]].ctypes.data if a["host"] == "plan" else a["host"]
    pb = 4 * (HEADER_WORDS + len(SHAPES) * DESC_WORDS) if a["plan_bytes"] is None else a["plan_bytes"]
    return [a["a"], _i64(good, 12) + a["d_a"], a["b"], _i64(good, 12) + a["d_b"], a["mask"], _i64(good, 14) + a["d_mask"], a["stats"],
            120 * len(SHAPES) + a["d_stats"], a["ws"], _i64(good, 16) + a["d_ws"], host, a["dev"], pb, a["window"], a["flags"], None]


FAULTS = [
    (dict(a=None), E_NULL, b"NULL"), (dict(b=None), E_NULL, b"NULL"), (dict(host=None), E_NULL, b"host_plan"),
    (dict(dev=None), E_NULL, b"plan_dev"),
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x400000), E_FLAGS, b"flag"), (dict(flags=0x80000000), E_FLAGS, b"flag"),
    (dict(plan="zeros"), E_WORKSPACE, b"ragged loss: host_plan holds no plan"), (dict(plan="stamp"), E_WORKSPACE, b"no plan"),
    (dict(plan="op0"), E_WORKSPACE, b"no plan"), (dict(plan="msssim"), E_WORKSPACE, b"no plan (curl_loss_ragged_plan)"),
    (dict(plan="shifted"), E_WORKSPACE, b"8-byte"),
    (dict(plan="operator"), E_WORKSPACE, b"another operator"),
    (dict(plan="nomask"), E_WORKSPACE, b"without masks"),
    (dict(dev=_p(5, 4)), E_WORKSPACE, b"8-byte"), (dict(plan_bytes=4 * (HEADER_WORDS + 2 * DESC_WORDS) - 1), E_WORKSPACE, b"too small"),
    (dict(d_a=-1), E_WORKSPACE, b"ragged loss: the pred arena"), (dict(d_b=-1), E_WORKSPACE, b"ragged loss: the target arena"),
    (dict(d_mask=-1), E_WORKSPACE, b"mask arena"),
    (dict(stats=None), E_WORKSPACE, b"ragged loss: stats"), (dict(d_stats=-1), E_WORKSPACE, b"stats is too small (120 bytes"),
    (dict(stats=_p(4, 4)), E_WORKSPACE, b"stats"),
    (dict(ws=None), E_WORKSPACE, b"ragged loss: workspace"), (dict(d_ws=-1), E_WORKSPACE, b"curl_loss_ragged_workspace_bytes"),
    (dict(ws=_p(6, 4)), E_WORKSPACE, b"workspace"),
    (dict(a=_p(1, 1)), E_SHAPE, b"4-byte"), (dict(b=_p(2, 2)), E_SHAPE, b"4-byte"), (dict(mask=_p(3, 1)), E_SHAPE, b"4-byte"),
    (dict(window=0), E_KNOTS, b"window_size"), (dict(window=13), E_KNOTS, b"window_size"), (dict(window=4), E_KNOTS, b"window_size"),
    (dict(window=-3), E_KNOTS, b"window_size"),
]


@pytest.mark.parametrize("kw,code,word", FAULTS)
def test_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_loss_ragged_u8hwc(*_args(plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


def test_the_checks_come_in_the_msssim_entrys_order(lib, plans):
    """Two faults at once: the earlier check of curl_msssim_ragged_u8hwc's order answers."""
    for kw, code, word in ((dict(a=None, flags=1), E_NULL, b"NULL"), (dict(flags=1, plan="operator"), E_FLAGS, b"flag"),
                           (dict(plan="operator", d_a=-1), E_WORKSPACE, b"another operator"), (dict(d_b=-1, stats=None), E_WORKSPACE, b"target arena"),
                           (dict(d_ws=-1, a=_p(1, 1)), E_WORKSPACE, b"workspace"), (dict(a=_p(1, 1), window=4), E_SHAPE, b"4-byte")):
        assert lib.curl_loss_ragged_u8hwc(*_args(plans, **kw)) == code, (kw, lib.curl_last_error())
        assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


# ------------------------------------------------------------------ the Python surface on the host
BATCH = [(32, 32), (33, 47), (40, 36)]


def test_curl_loss_from_stats_is_the_oracles_loss():
    """[3,5] statistics built from the oracle in float64 for an image under a random mask -- the sums from curl_loss_terms'
    pieces, the level statistics from criterion_check.msssim_level_stats on the oracle's L planes -- give the oracle's
    curl_loss with its own one-channel msssim, to 1e-12; on the CPU, in float64; N = 0 gives nan."""
    import torch
    import criterion_check as CC
    from curl_amd import ops
    g = torch.Generator().manual_seed(11)
    rows, shapes, want = [], [], []
    for (h, w), mask_kind in (((40, 36), "random"), ((33, 47), "none"), ((64, 35), "zero"), ((37, 50), "random")):
        a, b = (torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.int32).to(torch.uint8) for _ in range(2))
        mask = {"random": torch.tensor([0, 1, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (h, w), generator=g)], "none": None,
                "zero": torch.zeros(h, w, dtype=torch.uint8)}[mask_kind]
        ref = LossReference(a, b, mask)
        ssims, mcs = CC.msssim_level_stats(ref.Lp, ref.Lt, 11)
        assert ssims.dtype == torch.float64 and ref.Lp.dtype == torch.float64
        rows.append(np.stack([ref.row0, ssims[0].numpy(), mcs[0].numpy()]))
        shapes.append((h, w))
        want.append(ref.loss)
        assert (ref.n == 0) == (mask_kind == "zero") and (mask_kind != "random" or 0 < ref.n < h * w)
    stats = torch.from_numpy(np.stack(rows))
    got = ops.curl_loss_from_stats(stats, shapes)
    assert got.dtype == torch.float64 and got.shape == (4,) and got.device.type == "cpu"
    got, want = got.numpy(), np.array(want)
    assert np.isnan(got[2]) and np.isnan(want[2])  # the reference's 0 / 0
    keep = [0, 1, 3]
    assert np.isfinite(got[keep]).all() and np.abs(got[keep] - want[keep]).max() <= 1e-12, (got, want)
    assert np.abs(loss_formula(stats.numpy(), shapes)[keep] - want[keep]).max() <= 1e-12  # and the numpy formula the GPU tests use
    assert 0.05 < got[keep].min() and got[keep].max() < 3.0
    for bad_stats, bad_shapes in ((stats[:, :2], shapes), (stats, shapes[:3]), (stats[0], shapes[:1])):
        with pytest.raises(ValueError):
            ops.curl_loss_from_stats(bad_stats, bad_shapes)
    empty = ops.curl_loss_from_stats(torch.zeros(0, 3, 5, dtype=torch.float64), [])
    assert empty.shape == (0,) and empty.dtype == torch.float64


def test_loss_ops_on_the_host():
    import torch
    from curl_amd import ops
    a = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in BATCH]
    b = [torch.ones(h, w, 3, dtype=torch.uint8) for h, w in BATCH]
    ms = [t[..., 0].contiguous() for t in a]
    sig = inspect.signature(ops.loss_stats_u8hwc_ragged).parameters
    assert list(sig) == ["pred", "target", "masks", "window_size"] and sig["masks"].default is None and sig["window_size"].default == 11
    sig = inspect.signature(ops.curl_loss_u8hwc_ragged).parameters
    assert list(sig) == ["pred", "target", "masks"] and sig["masks"].default is None
    assert list(inspect.signature(ops.curl_loss_from_stats).parameters) == ["stats", "shapes"]
    for call in (ops.loss_stats_u8hwc_ragged, ops.curl_loss_u8hwc_ragged):
        for x, y, m in ((a, b, ms), (a, b, None), (ops.RaggedBytes.pack(a), ops.RaggedBytes.pack(b), ops.RaggedBytes.pack(ms)),
                        ([t.numpy() for t in a], [t.numpy() for t in b], [t.numpy() for t in ms])):
            with pytest.raises(RuntimeError, match="HIP device only"):  # a CPU arena raises: no CPU fallback
                call(x, y, m)
        rgba = [torch.zeros(h, w, 4, dtype=torch.uint8) for h, w in BATCH]
        for x, y in ((rgba, b), (a, rgba), (ops.RaggedBytes.pack(rgba), b), ([t.float() for t in a], b),
                     (a, [t.numpy().astype(np.int16) for t in b]), (a, b[:2]), (a, [b[0], b[2], b[1]]), (a[:2], b), (ms, ms)):
            with pytest.raises(ValueError):
                call(x, y)
        for bad in (ms[:2], [ms[0], ms[2], ms[1]], [ms[0], ms[1], a[2]], [ms[0], ms[1], ms[2].float()], ops.RaggedBytes.pack(a)):
            with pytest.raises(ValueError):
                call(a, b, bad)
        # an image under 32 on a side is named by its index, before anything is packed or uploaded
        small = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in ((40, 40), (64, 31), (20, 50))]
        with pytest.raises(ValueError, match="image 1 is 64x31"):
            call(small, small)
        with pytest.raises(ValueError, match="image 0 is 31x32"):
            call(ops.RaggedBytes.pack([torch.zeros(31, 32, 3, dtype=torch.uint8)]), ops.RaggedBytes.pack([torch.zeros(31, 32, 3, dtype=torch.uint8)]))
    for window in (0, 2, 13, -1, 4.0 + 0.5):
        with pytest.raises(ValueError, match="window_size"):
            ops.loss_stats_u8hwc_ragged(a, b, None, window)
    stats = ops.loss_stats_u8hwc_ragged([], [])
    assert stats.shape == (0, 3, 5) and stats.dtype == torch.float64
    assert ops.loss_stats_u8hwc_ragged([], [], []).shape == (0, 3, 5)
    value = ops.curl_loss_u8hwc_ragged([], [], None)
    assert value.shape == (0,) and value.dtype == torch.float64


def test_enhance_and_evaluate_many_on_the_host():
    from curl_amd import infer
    sig = inspect.signature(infer.enhance_and_evaluate_many).parameters
    assert list(sig) == list(inspect.signature(infer.enhance_and_score_many).parameters)
    assert sig["view"].default == "pil" and sig["batch_size"].default == 32 and sig["foreground"].default is False
    assert "bytes written" in infer.enhance_and_evaluate_many.__doc__.lower()
    imgs = [np.zeros((40, 40, 3), np.uint8), np.zeros((41, 40, 4), np.uint8)]
    masks = [np.zeros(t.shape[:2], np.uint8) for t in imgs]
    with pytest.raises(ValueError, match="target 1"):
        infer.enhance_and_evaluate_many(None, imgs, masks, [np.zeros((40, 40, 3), np.uint8), np.zeros((40, 41, 3), np.uint8)], "cpu")
    with pytest.raises(ValueError):
        infer.enhance_and_evaluate_many(None, imgs, masks, imgs[:1], "cpu")
    with pytest.raises(ValueError):
        infer.enhance_and_evaluate_many(None, [], [], [], "cpu", batch_size=0)
    outs, psnr, msssim, loss = infer.enhance_and_evaluate_many(None, [], [], [], "cpu")
    assert outs == [] and psnr.shape == (0,) and msssim.shape == (0,) and loss.shape == (0,) and loss.dtype == np.float64
    assert len(infer.enhance_and_score_many(None, [], [], [], "cpu")) == 2  # the siblings' return values are as they were
    assert len(infer.enhance_and_score_many_msssim(None, [], [], [], "cpu")) == 3


def _folders(tmp_path, stems):
    from PIL import Image
    for d in ("in", "masks", "gt"):
        (tmp_path / d).mkdir()
    for s in stems:
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "in" / f"{s}.png")
        Image.fromarray(np.zeros((8, 8), np.uint8)).save(tmp_path / "masks" / f"{s}.png")
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "gt" / f"{s}.png")
    return ["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random", "--out_dir",
            str(tmp_path / "out")]


def test_infer_dir_parses_loss(monkeypatch, tmp_path, capsys):
    """--loss (with --gt_dir) selects enhance_and_evaluate_many and appends a loss column and its mean over the finite values;
    with --msssim the msssim column stands before it; without the flag the other two functions are called and the lines are as
    they were (the model and the functions are stubbed: nothing reaches a device).  --loss without --gt_dir is an error."""
    from curl_amd import infer_dir
    calls = []
    psnrs = {"a": 30.0, "b": float("inf"), "c": 25.0, "d": 20.5}
    seconds = {"a": 0.75, "b": 1.0, "c": float("nan"), "d": 0.5}
    thirds = {"a": 0.25, "b": 0.0, "c": float("nan"), "d": float("nan")}
    out8 = np.zeros((8, 8, 3), np.uint8)
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: None)

    def start():
        return sum(c[1] for c in calls[:-1]) % len(psnrs)

    def column(values, k, n):
        return np.array([values[s] for s in sorted(values)][k:k + n])

    def score(net, imgs, ms, tgts, device, view="pil", batch_size=32, foreground=False):
        calls.append(("psnr", len(imgs), foreground))
        return [out8] * len(imgs), column(psnrs, start(), len(imgs))

    def score2(net, imgs, ms, tgts, device, view="pil", batch_size=32, foreground=False):
        calls.append(("msssim", len(imgs), foreground))
        return [out8] * len(imgs), column(psnrs, start(), len(imgs)), column(seconds, start(), len(imgs))

    def score3(net, imgs, ms, tgts, device, view="pil", batch_size=32, foreground=False):
        calls.append(("loss", len(imgs), foreground))
        return [out8] * len(imgs), column(psnrs, start(), len(imgs)), column(seconds, start(), len(imgs)), column(thirds, start(), len(imgs))
    monkeypatch.setattr(infer_dir, "enhance_and_score_many", score)
    monkeypatch.setattr(infer_dir, "enhance_and_score_many_msssim", score2)
    monkeypatch.setattr(infer_dir, "enhance_and_evaluate_many", score3)
    base = _folders(tmp_path, sorted(psnrs)) + ["--gt_dir", str(tmp_path / "gt")]
    assert infer_dir.main(base + ["--batch_size", "3"]) == 0
    assert calls == [("psnr", 3, False), ("psnr", 1, False)]
    plain = capsys.readouterr().out.splitlines()
    assert [len(ln.split("\t")) for ln in plain] == [2, 2, 2, 2, 3]  # as before
    del calls[:]
    assert infer_dir.main(base + ["--batch_size", "3", "--msssim"]) == 0
    assert calls == [("msssim", 3, False), ("msssim", 1, False)]
    with_ms = capsys.readouterr().out.splitlines()
    assert [len(ln.split("\t")) for ln in with_ms] == [3, 3, 3, 3, 5]  # as before
    del calls[:]
    scores = tmp_path / "scores.txt"
    assert infer_dir.main(base + ["--loss", "--batch_size", "3", "--scores_file", str(scores), "--foreground_masks"]) == 0
    assert calls == [("loss", 3, True), ("loss", 1, True)]  # one call per batch
    lines = capsys.readouterr().out.splitlines()
    assert scores.read_text().splitlines() == lines and len(lines) == 5
    rows = [ln.split("\t") for ln in lines]
    assert [r[0] for r in rows] == ["a", "b", "c", "d", "mean"] and [len(r) for r in rows] == [3, 3, 3, 3, 5]
    assert ["\t".join(r[:2]) for r in rows[:4]] == plain[:4]  # the psnr column is the plain run's
    assert [float(r[2]) for r in rows[:2]] == [0.25, 0.0] and np.isnan(float(rows[2][2])) and np.isnan(float(rows[3][2]))
    assert float(rows[4][1]) == (30.0 + 25.0 + 20.5) / 3 and float(rows[4][2]) == 0.125  # the mean over the finite ones
    assert (int(rows[4][3]), int(rows[4][4])) == (1, 2)
    del calls[:]
    assert infer_dir.main(base + ["--loss", "--msssim", "--batch_size", "3"]) == 0
    assert calls == [("loss", 3, False), ("loss", 1, False)]
    rows = [ln.split("\t") for ln in capsys.readouterr().out.splitlines()]
    assert [len(r) for r in rows] == [4, 4, 4, 4, 7]
    assert ["\t".join(r[:3]) for r in rows[:4]] == with_ms[:4]  # psnr and msssim columns are the --msssim run's
    assert [float(r[3]) for r in rows[:2]] == [0.25, 0.0]
    assert [float(v) for v in rows[4][1:4]] == [(30.0 + 25.0 + 20.5) / 3, (0.75 + 1.0 + 0.5) / 3, 0.125]
    assert [int(v) for v in rows[4][4:]] == [1, 1, 2]
    with pytest.raises(SystemExit):
        infer_dir.main(base[:-2] + ["--loss"])  # needs --gt_dir
