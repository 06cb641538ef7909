"""The ragged MS-SSIM entries (include/curl_hip_ragged_msssim.h) without a device: the header compiles as C99 and C++17, the
four names are declared, exported and bound from _lib.SIGNATURES_RAGGED_MSSSIM beside the eight unchanged tables; the plan's
limits, its offsets against the op-0 curl_ragged_plan's, a three-image plan worked out by hand, the workspace query; every
single-fault argument list of curl_msssim_ragged_u8hwc a return code with its word before any HIP call (fake device
pointers); and the host side of ops.msssim_stats_u8hwc_ragged / msssim_u8hwc_ragged, infer.enhance_and_score_many_msssim and
infer_dir --msssim."""
import ctypes
import inspect
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ragged_msssim_ref import SHAPES as BATCH_SHAPES, WEIGHTS, msssim_formula, plan_by_hand

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
PLAN_BYTES, PLAN, WS, ENTRY = ("curl_msssim_ragged_plan_bytes", "curl_msssim_ragged_plan", "curl_msssim_ragged_workspace_bytes",
                               "curl_msssim_ragged_u8hwc")
NAMES = {PLAN_BYTES: 1, PLAN: 6, WS: 1, ENTRY: 16}
HEADER_WORDS, DESC_WORDS, LEVEL_WORD, LEVEL_WORDS = 32, 64, 16, 8
STAMP = 0x4D535231
TABLES = {"SIGNATURES": "curl_hip.h", "SIGNATURES_GRAD": "curl_hip_grad.h", "SIGNATURES_VIEW": "curl_hip_view.h",
          "SIGNATURES_FG": "curl_hip_fg.h", "SIGNATURES_RAGGED": "curl_hip_ragged.h", "SIGNATURES_VIEW_RAGGED": "curl_hip_view_ragged.h",
          "SIGNATURES_RAGGED_FG": "curl_hip_ragged_fg.h", "SIGNATURES_RAGGED_SCORE": "curl_hip_ragged_score.h"}


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl = dict(_declared("curl_hip_ragged_msssim.h"))
    assert set(decl) == set(_lib.SIGNATURES_RAGGED_MSSSIM) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_RAGGED_MSSSIM[name][1]) == n, name
        fn = getattr(lib, name)  # exported
        assert fn.restype is _lib.SIGNATURES_RAGGED_MSSSIM[name][0] and list(fn.argtypes) == _lib.SIGNATURES_RAGGED_MSSSIM[name][1]
    for table, header in TABLES.items():  # the eight existing tables still equal their headers
        assert set(getattr(_lib, table)) == {n for n, _ in _declared(header)}, table
    assert lib.curl_version() >= 120
    assert (_lib.MSSSIM_RAGGED_STAMP, _lib.MSSSIM_RAGGED_HEADER_WORDS, _lib.MSSSIM_RAGGED_DESC_WORDS, _lib.MSSSIM_RAGGED_LEVEL_WORD,
            _lib.MSSSIM_RAGGED_LEVEL_WORDS) == (STAMP, HEADER_WORDS, DESC_WORDS, LEVEL_WORD, LEVEL_WORDS)
    hdr = open(f"{ROOT}/include/curl_hip_ragged_msssim.h").read()
    for macro, value in (("STAMP", "0x4D535231"), ("HEADER_WORDS", "32"), ("DESC_WORDS", "64"), ("LEVEL_WORD", "16"), ("LEVEL_WORDS", "8")):
        assert re.search(rf"#define CURL_MSSSIM_RAGGED_{macro} {value}\b", hdr), macro


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_ragged_msssim.h"\n'
                   "int main(void) {\n"
                   "  int hw[1] = {32};\n"
                   "  long long buf[(CURL_MSSSIM_RAGGED_HEADER_WORDS + CURL_MSSSIM_RAGGED_DESC_WORDS) / 2];\n"
                   "  if (curl_msssim_ragged_plan_bytes(1) != sizeof buf) return 4;\n"
                   "  if (curl_msssim_ragged_plan(1, hw, hw, 1, buf, sizeof buf) != CURL_OK) return 3;\n"
                   "  if (curl_msssim_ragged_workspace_bytes(buf) == 0) return 2;\n"
                   "  return curl_msssim_ragged_u8hwc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, buf, 0, 0, 11, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


# ------------------------------------------------------------------ the plan
def _plan(lib, shapes, has_mask=1, expect=0):
    B = len(shapes)
    hs, ws = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(2))
    nbytes = lib.curl_msssim_ragged_plan_bytes(B)
    assert nbytes == 4 * (HEADER_WORDS + DESC_WORDS * B)
    buf = np.zeros(nbytes // 4 + 2, dtype=np.int32)
    assert buf.ctypes.data % 8 == 0
    rc = lib.curl_msssim_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, has_mask, buf.ctypes.data, nbytes)
    assert rc == expect, (rc, lib.curl_last_error())
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
    assert lib.curl_msssim_ragged_plan_bytes(0) == 0 and lib.curl_msssim_ragged_plan_bytes(65536) == 0
    assert lib.curl_msssim_ragged_plan_bytes(65535) == 4 * (HEADER_WORDS + DESC_WORDS * 65535)
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
    one = np.array([32], dtype=np.int32)
    good = np.zeros(HEADER_WORDS + DESC_WORDS + 2, dtype=np.int32)
    nb = 4 * (HEADER_WORDS + DESC_WORDS)
    assert lib.curl_msssim_ragged_plan(0, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data, nb) == E_SHAPE
    assert lib.curl_msssim_ragged_plan(65536, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data, nb) == E_SHAPE
    assert lib.curl_msssim_ragged_plan(1, None, one.ctypes.data, 1, good.ctypes.data, nb) == E_NULL
    assert lib.curl_msssim_ragged_plan(1, one.ctypes.data, None, 1, good.ctypes.data, nb) == E_NULL
    assert lib.curl_msssim_ragged_plan(1, one.ctypes.data, one.ctypes.data, 1, None, nb) == E_NULL
    assert lib.curl_msssim_ragged_plan(1, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data, nb - 1) == E_WORKSPACE
    assert lib.curl_msssim_ragged_plan(1, one.ctypes.data, one.ctypes.data, 1, good.ctypes.data + 4, nb) == E_WORKSPACE


@pytest.mark.parametrize("has_mask", [1, 0])
def test_plan_offsets_are_the_op0_plans(lib, has_mask):
    """Every rgb_off / mask_off equals the out_off / mask_off of curl_ragged_plan for operator 0 and the same shape list, and
    the arena sizes its out / mask arena's: the arenas are RaggedBytes.pack's."""
    shapes = BATCH_SHAPES + [(33, 33), (32, 35)]  # odd pixel counts: padding between the images
    p, q = _plan(lib, shapes, has_mask), _op0_plan(lib, shapes, has_mask)
    assert _i64(p, 12) == _i64(q, 16) and _i64(p, 14) == _i64(q, 14) and (_i64(p, 14) > 0) == bool(has_mask)
    op0 = {int(q[32 + 16 * k + 1]): (_i64(q, 32 + 16 * k + 14), _i64(q, 32 + 16 * k + 12)) for k in range(len(shapes))}
    padded = False
    for i, (h, w) in enumerate(shapes):
        d = p[HEADER_WORDS + DESC_WORDS * i:HEADER_WORDS + DESC_WORDS * (i + 1)]
        assert (int(d[0]), int(d[1]), int(d[2])) == (i, h, w)
        assert (_i64(d, 4), _i64(d, 6)) == op0[i], i
        assert _i64(d, 4) % 16 == 0 and _i64(d, 6) % 16 == 0
        if i:
            prev = p[HEADER_WORDS + DESC_WORDS * (i - 1):]
            padded |= _i64(d, 4) != _i64(prev, 4) + 3 * shapes[i - 1][0] * shapes[i - 1][1]
    assert padded


@pytest.mark.parametrize("has_mask", [1, 0])
def test_a_plan_worked_out_by_hand(lib, has_mask):
    shapes = [(32, 32), (33, 47), (97, 129)]
    p = _plan(lib, shapes, has_mask)
    images, head = plan_by_hand(shapes, has_mask)
    # the figures themselves, not only the second implementation of the rule
    assert head["grid"] == [25, 6, 3, 3, 3] and head["pair0"] == [0, 25, 31, 34, 37]
    assert head["rgb_bytes"] == 45267 and head["mask_bytes"] == (15089 if has_mask else 0)
    assert head["partial_off"] == 117600 and head["ws_bytes"] == 117600 + 40 * 16
    assert [[(lv["h"], lv["w"]) for lv in img["levels"]] for img in images] == [
        [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], [(33, 47), (16, 23), (8, 11), (4, 5), (2, 2)],
        [(97, 129), (48, 64), (24, 32), (12, 16), (6, 8)]]
    assert [[lv["tiles"] for lv in img["levels"]] for img in images] == [[1, 1, 1, 1, 1], [4, 1, 1, 1, 1], [20, 4, 1, 1, 1]]
    assert [[lv["first"] for lv in img["levels"]] for img in images] == [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [5, 2, 2, 2, 2]]
    assert [img["rgb_off"] for img in images] == [0, 3072, 7728]
    assert [img["levels"][1]["planes"] for img in images] == [0, 8160, 19680]
    # ... and the library's words
    assert (int(p[0]) & 0xffffffff, int(p[1]), int(p[2]), int(p[3]), int(p[4])) == (STAMP, 3, 5, has_mask, 6)
    assert [int(v) for v in p[5:10]] == head["grid"] and [int(v) for v in p[22:27]] == head["pair0"]
    assert (_i64(p, 12), _i64(p, 14), _i64(p, 16), _i64(p, 20)) == (head["rgb_bytes"], head["mask_bytes"], head["ws_bytes"], head["partial_off"])
    for i, img in enumerate(images):
        d = p[HEADER_WORDS + DESC_WORDS * i:HEADER_WORDS + DESC_WORDS * (i + 1)]
        assert (_i64(d, 4), _i64(d, 6)) == (img["rgb_off"], img["mask_off"])
        for l, lv in enumerate(img["levels"]):
            v = d[LEVEL_WORD + LEVEL_WORDS * l:LEVEL_WORD + LEVEL_WORDS * (l + 1)]
            assert [int(x) for x in v[:6]] == [lv["h"], lv["w"], lv["tiles_x"], lv["tiles"], lv["first"], lv["pair"]], (i, l)
            assert _i64(v, 6) == lv["planes"], (i, l)
    assert lib.curl_msssim_ragged_workspace_bytes(p.ctypes.data) == head["ws_bytes"]
    # the hash covers (has_mask, B, every H, W)
    assert _i64(p, 18) != _i64(_plan(lib, shapes, 1 - has_mask), 18)
    assert _i64(p, 18) != _i64(_plan(lib, shapes[::-1], has_mask), 18) and _i64(p, 18) != _i64(_plan(lib, shapes[:2], has_mask), 18)
    assert _i64(p, 18) != _i64(_plan(lib, [(32, 32), (47, 33), (97, 129)], has_mask), 18)
    assert _i64(p, 18) == _i64(_plan(lib, shapes, has_mask), 18)


def test_workspace_bytes(lib):
    for has_mask in (0, 1):
        p = _plan(lib, BATCH_SHAPES, has_mask)
        _, head = plan_by_hand(BATCH_SHAPES, has_mask)
        assert lib.curl_msssim_ragged_workspace_bytes(p.ctypes.data) == head["ws_bytes"] == _i64(p, 16)
        planes = sum(24 * (h >> l) * (w >> l) for h, w in BATCH_SHAPES for l in range(1, 5))
        assert head["partial_off"] >= planes and head["ws_bytes"] == head["partial_off"] + 16 * sum(int(v) for v in p[5:10])
    assert lib.curl_msssim_ragged_workspace_bytes(None) == 0
    assert lib.curl_msssim_ragged_workspace_bytes(np.zeros_like(p).ctypes.data) == 0
    bad = p.copy()
    bad[0] ^= 1
    assert lib.curl_msssim_ragged_workspace_bytes(bad.ctypes.data) == 0
    other = p.copy()
    other[2] = 0
    assert lib.curl_msssim_ragged_workspace_bytes(other.ctypes.data) == 0
    # a plan of curl_ragged_plan is no such plan, and this one is no plan of that header's
    q = _op0_plan(lib, BATCH_SHAPES, 1)
    assert lib.curl_msssim_ragged_workspace_bytes(q.ctypes.data) == 0
    assert lib.curl_ragged_score_workspace_bytes(p.ctypes.data) == 0


# ------------------------------------------------------------------ the entry's argument lists
def _p(n, off=0):
    return ctypes.c_void_p((n << 20) + off)


SHAPES = [(40, 36), (33, 47)]


@pytest.fixture(scope="module")
def plans(lib):
    """name -> host plan words.  'zeros': no plan at all; 'stamp': one bit of the stamp wrong; 'op0': curl_ragged_plan's plan of
    operator 0; 'operator': this header's plan with another operator word; 'shifted': four bytes off the 8-byte grid."""
    out = {"masks": _plan(lib, SHAPES, 1), "nomask": _plan(lib, SHAPES, 0), "op0": _op0_plan(lib, SHAPES, 1)}
    out["zeros"] = np.zeros_like(out["masks"])
    out["stamp"] = out["masks"].copy()
    out["stamp"][0] ^= 1
    out["operator"] = out["masks"].copy()
    out["operator"][2] = 126
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
            80 * len(SHAPES) + a["d_stats"], a["ws"], _i64(good, 16) + a["d_ws"], host, a["dev"], pb, a["window"], a["flags"], None]


FAULTS = [
    (dict(a=None), E_NULL, b"NULL"), (dict(b=None), E_NULL, b"NULL"), (dict(host=None), E_NULL, b"host_plan"),
    (dict(dev=None), E_NULL, b"plan_dev"),
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x400000), E_FLAGS, b"flag"), (dict(flags=0x80000000), E_FLAGS, b"flag"),
    (dict(plan="zeros"), E_WORKSPACE, b"no plan"), (dict(plan="stamp"), E_WORKSPACE, b"no plan"), (dict(plan="op0"), E_WORKSPACE, b"no plan"),
    (dict(plan="shifted"), E_WORKSPACE, b"8-byte"),
    (dict(plan="operator"), E_WORKSPACE, b"another operator"),
    (dict(plan="nomask"), E_WORKSPACE, b"without masks"),
    (dict(dev=_p(5, 4)), E_WORKSPACE, b"8-byte"), (dict(plan_bytes=4 * (HEADER_WORDS + 2 * DESC_WORDS) - 1), E_WORKSPACE, b"too small"),
    (dict(d_a=-1), E_WORKSPACE, b"a arena"), (dict(d_b=-1), E_WORKSPACE, b"b arena"), (dict(d_mask=-1), E_WORKSPACE, b"mask arena"),
    (dict(stats=None), E_WORKSPACE, b"stats"), (dict(d_stats=-1), E_WORKSPACE, b"stats"), (dict(stats=_p(4, 4)), E_WORKSPACE, b"stats"),
    (dict(ws=None), E_WORKSPACE, b"workspace"), (dict(d_ws=-1), E_WORKSPACE, b"workspace"), (dict(ws=_p(6, 4)), E_WORKSPACE, b"workspace"),
    (dict(a=_p(1, 1)), E_SHAPE, b"4-byte"), (dict(b=_p(2, 2)), E_SHAPE, b"4-byte"), (dict(mask=_p(3, 1)), E_SHAPE, b"4-byte"),
    (dict(window=0), E_KNOTS, b"window_size"), (dict(window=13), E_KNOTS, b"window_size"), (dict(window=4), E_KNOTS, b"window_size"),
    (dict(window=-3), E_KNOTS, b"window_size"),
]


@pytest.mark.parametrize("kw,code,word", FAULTS)
def test_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_msssim_ragged_u8hwc(*_args(plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


# ------------------------------------------------------------------ the Python surface on the host
BATCH = [(32, 32), (33, 47), (40, 36)]


def test_msssim_ops_on_the_host():
    import torch
    from curl_amd import ops
    a = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in BATCH]
    b = [torch.ones(h, w, 3, dtype=torch.uint8) for h, w in BATCH]
    ms = [t[..., 0].contiguous() for t in a]
    for call in (ops.msssim_stats_u8hwc_ragged, ops.msssim_u8hwc_ragged):
        sig = inspect.signature(call).parameters
        assert list(sig) == ["a", "b", "masks", "window_size"] and sig["masks"].default is None and sig["window_size"].default == 11
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
        for window in (0, 2, 13, -1, 4.0 + 0.5):
            with pytest.raises(ValueError, match="window_size"):
                call(a, b, None, window)
        # an image under 32 on a side is named by its index, before anything is packed or uploaded
        small = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in ((40, 40), (64, 31), (20, 50))]
        with pytest.raises(ValueError, match="image 1 is 64x31"):
            call(small, small)
        with pytest.raises(ValueError, match="image 0 is 31x32"):
            call(ops.RaggedBytes.pack([torch.zeros(31, 32, 3, dtype=torch.uint8)]), ops.RaggedBytes.pack([torch.zeros(31, 32, 3, dtype=torch.uint8)]))
    stats = ops.msssim_stats_u8hwc_ragged([], [])
    assert stats.shape == (0, 2, 5) and stats.dtype == torch.float64
    assert ops.msssim_stats_u8hwc_ragged([], [], []).shape == (0, 2, 5)
    value = ops.msssim_u8hwc_ragged([], [], None)
    assert value.shape == (0,) and value.dtype == torch.float64


def test_msssim_from_stats_is_the_formula():
    """ops.msssim_from_stats in float64 on the host against the numpy formula and against the oracle's msssim on its own
    statistics: the weights are the reference's float32 ones, the last factor enters four times."""
    import torch
    import curl_oracle as O
    import criterion_check as CC
    from curl_amd import ops
    g = torch.Generator().manual_seed(5)
    stats = torch.rand(7, 2, 5, generator=g, dtype=torch.float64) * 1.2 - 0.2
    got = ops.msssim_from_stats(stats)
    assert got.dtype == torch.float64 and got.shape == (7,)
    assert np.abs(got.numpy() - msssim_formula(stats.numpy())).max() <= 1e-12
    x = (stats.numpy() + 1) / 2
    by_hand = np.prod(x[:, 1, :4] ** WEIGHTS[:4], axis=1) * (x[:, 0, 4] ** WEIGHTS[4]) ** 4
    assert np.abs(got.numpy() - by_hand).max() <= 1e-12
    a, b = torch.rand(2, 3, 40, 36, generator=g, dtype=torch.float64), torch.rand(2, 3, 40, 36, generator=g, dtype=torch.float64)
    ssims, mcs = CC.msssim_level_stats(a, b, 11)
    assert (ops.msssim_from_stats(torch.stack((ssims, mcs), 1)) - O.msssim(a, b)).abs().max() <= 1e-12


def test_enhance_and_score_many_msssim_on_the_host():
    from curl_amd import infer
    sig = inspect.signature(infer.enhance_and_score_many_msssim).parameters
    assert list(sig) == list(inspect.signature(infer.enhance_and_score_many).parameters)
    assert sig["view"].default == "pil" and sig["batch_size"].default == 32 and sig["foreground"].default is False
    imgs = [np.zeros((40, 40, 3), np.uint8), np.zeros((41, 40, 4), np.uint8)]
    masks = [np.zeros(t.shape[:2], np.uint8) for t in imgs]
    with pytest.raises(ValueError, match="target 1"):
        infer.enhance_and_score_many_msssim(None, imgs, masks, [np.zeros((40, 40, 3), np.uint8), np.zeros((40, 41, 3), np.uint8)], "cpu")
    with pytest.raises(ValueError):
        infer.enhance_and_score_many_msssim(None, imgs, masks, imgs[:1], "cpu")
    with pytest.raises(ValueError):
        infer.enhance_and_score_many_msssim(None, [], [], [], "cpu", batch_size=0)
    outs, psnr, msssim = infer.enhance_and_score_many_msssim(None, [], [], [], "cpu")
    assert outs == [] and psnr.shape == (0,) and msssim.shape == (0,) and msssim.dtype == np.float64
    assert len(infer.enhance_and_score_many(None, [], [], [], "cpu")) == 2  # the sibling's return value is as it was


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


def test_infer_dir_parses_msssim(monkeypatch, tmp_path, capsys):
    """--msssim (with --gt_dir) selects enhance_and_score_many_msssim and prints stem, psnr, msssim per image and the two means
    over their finite values; without the flag the PSNR-only function is called and the lines are as they were (the model and
    the functions are stubbed: nothing reaches a device)."""
    from curl_amd import infer_dir
    calls = []
    psnrs = {"a": 30.0, "b": float("inf"), "c": 25.0, "d": 20.5}
    seconds = {"a": 0.75, "b": 1.0, "c": float("nan"), "d": 0.5}
    out8 = np.zeros((8, 8, 3), np.uint8)
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: None)

    def start():
        return sum(c[1] for c in calls[:-1]) % len(psnrs)

    def score(net, imgs, ms, tgts, device, view="pil", batch_size=32, foreground=False):
        calls.append(("psnr", len(imgs), foreground))
        return [out8] * len(imgs), np.array([psnrs[s] for s in sorted(psnrs)][start():start() + len(imgs)])

    def score2(net, imgs, ms, tgts, device, view="pil", batch_size=32, foreground=False):
        calls.append(("msssim", len(imgs), foreground))
        k = start()
        return ([out8] * len(imgs), np.array([psnrs[s] for s in sorted(psnrs)][k:k + len(imgs)]),
                np.array([seconds[s] for s in sorted(seconds)][k:k + len(imgs)]))
    monkeypatch.setattr(infer_dir, "enhance_and_score_many", score)
    monkeypatch.setattr(infer_dir, "enhance_and_score_many_msssim", score2)
    base = _folders(tmp_path, sorted(psnrs)) + ["--gt_dir", str(tmp_path / "gt")]
    assert infer_dir.main(base + ["--batch_size", "3"]) == 0
    assert calls == [("psnr", 3, False), ("psnr", 1, False)]
    plain = capsys.readouterr().out.splitlines()
    assert [len(ln.split("\t")) for ln in plain] == [2, 2, 2, 2, 3] and plain[4].split("\t")[0] == "mean"  # as now
    del calls[:]
    scores = tmp_path / "scores.txt"
    assert infer_dir.main(base + ["--msssim", "--batch_size", "3", "--scores_file", str(scores), "--foreground_masks"]) == 0
    assert calls == [("msssim", 3, True), ("msssim", 1, True)]  # one call per batch
    lines = capsys.readouterr().out.splitlines()
    assert scores.read_text().splitlines() == lines and len(lines) == 5
    rows = [ln.split("\t") for ln in lines]
    assert [r[0] for r in rows] == ["a", "b", "c", "d", "mean"] and [len(r) for r in rows] == [3, 3, 3, 3, 5]
    assert [float(r[1]) for r in rows[:4]] == [30.0, float("inf"), 25.0, 20.5]
    assert [float(r[2]) for r in rows[:2]] == [0.75, 1.0] and np.isnan(float(rows[2][2])) and float(rows[3][2]) == 0.5
    assert float(rows[4][1]) == (30.0 + 25.0 + 20.5) / 3 and float(rows[4][2]) == (0.75 + 1.0 + 0.5) / 3
    assert (int(rows[4][3]), int(rows[4][4])) == (1, 1)
    with pytest.raises(SystemExit):
        infer_dir.main(base[:-2] + ["--msssim"])  # needs --gt_dir
