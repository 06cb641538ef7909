"""The encoder views of a ragged batch (include/curl_hip_view_ragged.h) without a device: the header compiles as C99 and
C++17, the three entries are exported and bound from _lib.SIGNATURES_VIEW_RAGGED beside the unchanged tables; the host-built
plan -- tables, offsets, tiling sums, LDS, sharing, size, hash -- for fixed and seeded random shape lists and their
permutations; every limit and every single-fault argument list a return code with its text before any HIP call (fake device
pointers); and the host side of ops.encoder_view_u8hwc_ragged.

(The entries are declared in a header of their own, not in curl_hip_view.h: tests/test_encoder_view_abi.py holds that header
and _lib.SIGNATURES_VIEW to the three entries they were released with.)"""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

import encoder_view_cases as cases
from conftest import ROOT

E_NULL, E_SHAPE, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -4, -5, -6
NAMES = {"curl_encoder_view_ragged_plan_bytes": 4, "curl_encoder_view_ragged_plan": 8, "curl_encoder_view_ragged_u8hwc": 12}
HEADER_WORDS, DESC_WORDS, STAMP, LDS_BUDGET = 32, 32, 0x52565031, 48 * 1024
VIEW_HEADER_INTS = 16


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl = dict(_declared("curl_hip_view_ragged.h"))
    assert set(decl) == set(_lib.SIGNATURES_VIEW_RAGGED) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_VIEW_RAGGED[name][1]) == n, name
        fn = getattr(lib, name)
        assert fn.restype is _lib.SIGNATURES_VIEW_RAGGED[name][0] and list(fn.argtypes) == _lib.SIGNATURES_VIEW_RAGGED[name][1]
    # the other tables are still exactly their headers
    for table, header in ((_lib.SIGNATURES, "curl_hip.h"), (_lib.SIGNATURES_GRAD, "curl_hip_grad.h"), (_lib.SIGNATURES_VIEW, "curl_hip_view.h"),
                          (_lib.SIGNATURES_FG, "curl_hip_fg.h"), (_lib.SIGNATURES_RAGGED, "curl_hip_ragged.h")):
        assert set(table) == {n for n, _ in _declared(header)}, header
    assert lib.curl_version() >= 117
    src = open(f"{ROOT}/include/curl_hip_view_ragged.h").read()
    consts = {k: int(v, 0) for k, v in re.findall(r"#define CURL_VIEW_RAGGED_(\w+) (\w+)", src)}
    assert consts == {"STAMP": STAMP, "HEADER_WORDS": HEADER_WORDS, "DESC_WORDS": DESC_WORDS, "MAX_IMAGES": 65535}
    assert (_lib.VIEW_RAGGED_STAMP, _lib.VIEW_RAGGED_HEADER_WORDS, _lib.VIEW_RAGGED_DESC_WORDS, _lib.VIEW_RAGGED_MAX_IMAGES) == \
        (STAMP, HEADER_WORDS, DESC_WORDS, 65535)


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_view_ragged.h"\n'
                   "int main(void) {\n"
                   "  int hw[1] = {8}, c[1] = {3};\n"
                   "  long long buf[4096];\n"
                   "  size_t n = curl_encoder_view_ragged_plan_bytes(1, hw, hw, CURL_VIEW_SIZE_MIN);\n"
                   "  if (n < 4 * (CURL_VIEW_RAGGED_HEADER_WORDS + CURL_VIEW_RAGGED_DESC_WORDS) || n > sizeof buf) return 3;\n"
                   "  if (curl_encoder_view_ragged_plan(1, hw, hw, c, 0, CURL_VIEW_SIZE_MIN, buf, sizeof buf) != CURL_OK) return 4;\n"
                   "  if (*(int*)buf != CURL_VIEW_RAGGED_STAMP || CURL_VIEW_RAGGED_MAX_IMAGES != 65535) return 5;\n"
                   "  return curl_encoder_view_ragged_u8hwc(0, 0, 0, 0, 0, 0, 0, 0, 0, CURL_VIEW_SIZE_DEFAULT, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


# ------------------------------------------------------------------ the plan
def _arr(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _plan(lib, shapes, size, has_mask=1, expect=0):
    """-> the plan's int32 words (or nothing when the return code is `expect` != 0)."""
    B = len(shapes)
    hs, ws, cs = (_arr([s[k] for s in shapes]) for k in range(3))
    nbytes = lib.curl_encoder_view_ragged_plan_bytes(B, hs.ctypes.data, ws.ctypes.data, size)
    if expect:
        buf = np.zeros(max(nbytes // 4, 1 << 16), dtype=np.int32)
        rc = lib.curl_encoder_view_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, size, buf.ctypes.data, buf.nbytes)
        assert rc == expect, (rc, lib.curl_last_error())
        return None
    assert nbytes > 0 and nbytes % 4 == 0
    buf = np.full(nbytes // 4 + 2, -1, dtype=np.int32)
    assert buf.ctypes.data % 8 == 0
    rc = lib.curl_encoder_view_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, size, buf.ctypes.data, nbytes)
    assert rc == 0, (rc, lib.curl_last_error())
    assert (buf[-2:] == -1).all()  # nothing past the plan's bytes
    return buf[:-2]


def _i64(words):
    return np.ascontiguousarray(words).view(np.int64)


def _single_plan(lib, H, W, size):
    n = lib.curl_encoder_view_plan_bytes(H, W, size)
    buf = np.zeros(n // 4, dtype=np.int32)
    assert n > 0 and lib.curl_encoder_view_plan(H, W, size, buf.ctypes.data, n) == 0
    return buf


def _ragged_offsets(lib, shapes, has_mask):
    """img_off, mask_off per image and the two arena sizes of curl_ragged_plan (the curve layer's plan) for the same list."""
    B = len(shapes)
    hs, ws, cs = (_arr([s[k] for s in shapes]) for k in range(3))
    n = lib.curl_ragged_plan_bytes(B, 0)
    buf = np.zeros(n // 4, dtype=np.int32)
    assert lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, 0, buf.ctypes.data, n) == 0
    d = buf[32:32 + 16 * B].reshape(B, 16)
    off = _i64(d[:, 10:14].copy()).reshape(B, 2)
    by_image = np.empty_like(off)
    by_image[d[:, 1]] = off
    return by_image, [int(v) for v in _i64(buf[12:16])]


def _lds_of(d, size):
    """The workgroup's LDS from a descriptor's tiling fields, restated: X rows | Y rows | horizontal results | staged rows."""
    ksx, ksy, tc_log2, tr, _, nrows_cap, chunk_rows, pitch_img, pitch_mask = (int(v) for v in d[6:15])
    row = lambda k: (2 + k) | 1  # noqa: E731
    return 4 * ((row(ksx) << tc_log2) + tr * row(ksy) + (nrows_cap << tc_log2)) + chunk_rows * (pitch_img + pitch_mask)


def _check_plan(lib, shapes, size, has_mask=1):
    p = _plan(lib, shapes, size, has_mask)
    B = len(shapes)
    d = p[HEADER_WORDS:HEADER_WORDS + B * DESC_WORDS].reshape(B, DESC_WORDS)
    distinct = list(dict.fromkeys((h, w) for h, w, _ in shapes))
    assert (p[0], p[1], p[2], p[3], p[6], p[7]) == (STAMP, B, size, has_mask, len(distinct), 0) and (p[16:HEADER_WORDS] == 0).all()
    assert _i64(p[14:16])[0] == p.nbytes  # plan bytes == curl_encoder_view_ragged_plan_bytes (_plan sized the buffer by it)
    assert (d[:, 19] == 0).all() and (d[:, 24:] == 0).all()
    assert list(d[:, 1]) == list(range(B))
    assert [tuple(r) for r in d[:, 2:5]] == [tuple(s) for s in shapes]
    # the tables: curl_encoder_view_plan's words after its header, and Pillow's coefficients restated
    table = _i64(d[:, 16:18].copy()).reshape(-1)
    seen = {}
    for i, (H, W, C) in enumerate(shapes):
        one = _single_plan(lib, H, W, size)
        words = one.size - VIEW_HEADER_INTS
        t0 = int(table[i])
        assert d[i, 18] == words and HEADER_WORDS + B * DESC_WORDS <= t0 and t0 + words <= p.size, i
        assert np.array_equal(p[t0:t0 + words], one[VIEW_HEADER_INTS:]), i
        ow, oh, top, left = cases.view_geometry(H, W, size)
        kx, ky = cases.axis_ksize(W, ow), cases.axis_ksize(H, oh)
        assert (d[i, 6], d[i, 7]) == (kx, ky)
        nx = size * (2 + kx)
        assert np.array_equal(p[t0:t0 + nx].reshape(size, -1), cases.axis_rows(W, ow, left, size)), i
        assert np.array_equal(p[t0 + nx:t0 + words].reshape(size, -1), cases.axis_rows(H, oh, top, size)), i
        assert seen.setdefault((H, W), t0) == t0  # equal shapes share one table
    # ... laid out one after the other in the order of first appearance, nothing else in the plan
    starts = [seen[s] for s in distinct]
    lens = [int(d[[i for i, s in enumerate(shapes) if s[:2] == hw][0], 18]) for hw in distinct]
    assert starts[0] == HEADER_WORDS + B * DESC_WORDS and all(starts[k + 1] == starts[k] + lens[k] for k in range(len(starts) - 1))
    assert starts[-1] + lens[-1] == p.size
    # the arenas: curl_ragged_plan's offsets and sizes for the same list
    off, sizes = _ragged_offsets(lib, shapes, has_mask)
    assert np.array_equal(_i64(d[:, 20:24].copy()).reshape(B, 2), off)
    assert [int(v) for v in _i64(p[8:12])] == sizes
    # the tiling: tiles of size x size, a running sum that ends at the grid
    tc, tr, tiles = 1 << d[:, 8].astype(np.int64), d[:, 9].astype(np.int64), d[:, 5].astype(np.int64)
    assert (d[:, 8] <= 5).all() and (tr >= 1).all() and (tr <= 16).all()
    assert (tiles == -(-size // tc) * -(-size // tr)).all()
    first = d[:, 0].astype(np.int64)
    assert first[0] == 0 and (first[1:] == np.cumsum(tiles)[:-1]).all() and p[4] == tiles.sum() and 0 < p[4] < 2 ** 31
    # the LDS: every image's from its own numbers, the launch's the largest, inside the budget
    lds = [_lds_of(d[i], size) for i in range(B)]
    assert list(d[:, 15]) == lds and p[5] == max(lds) <= LDS_BUDGET
    for i, (H, W, C) in enumerate(shapes):  # a staged row holds the window's bytes from the dword below its first
        assert d[i, 13] % 4 == 0 and d[i, 13] >= d[i, 10] * C + 3 and d[i, 12] >= 1 and d[i, 12] <= d[i, 11]
        assert (d[i, 14] % 4 == 0 and d[i, 14] >= d[i, 10] + 3) if has_mask else d[i, 14] == 0
    return p


def _hash(p):
    return int(_i64(p[12:14])[0])


GOLDEN_BATCH = [(40, 56, 3), (56, 40, 3), (32, 33, 3), (32, 35, 3), (37, 37, 3), (37, 37, 3), (20, 27, 3), (641, 481, 3), (40, 56, 4), (56, 40, 3)]
FIXED = {
    "one": ([(40, 56, 3)], 32),
    "golden_batch": (GOLDEN_BATCH, 32),                      # tests/test_gpu_ragged_view.py's batch 1
    "default_size": ([(1000, 1500, 3), (12, 20, 3)], 320),
    "extreme_aspect": ([(97, 1003, 3), (40, 56, 3)], 16),
    "equal_photographs": ([(341, 512, 4)] * 5, 320),
    "most_shrunk_beside_upscaled": ([(512, 575, 3), (8, 8, 4), (512, 512, 3)], 8),   # 64x exactly beside 1x
    "largest_size": ([(1024, 1100, 3), (9, 9, 3)], 1024),
}


@pytest.mark.parametrize("case", list(FIXED))
def test_plan_of_fixed_shape_lists(lib, case):
    shapes, size = FIXED[case]
    _check_plan(lib, shapes, size)
    _check_plan(lib, shapes, size, has_mask=0)


def test_tilings_differ_inside_one_batch(lib):
    d = _plan(lib, *FIXED["most_shrunk_beside_upscaled"])[HEADER_WORDS:HEADER_WORDS + 3 * DESC_WORDS].reshape(3, DESC_WORDS)
    assert len({tuple(r[8:10]) for r in d}) > 1 and len(set(d[:, 15])) > 1


def test_plan_of_65535_images(lib):
    p = _plan(lib, [(8, 8, 3)] * 65535, 8)
    d = p[HEADER_WORDS:HEADER_WORDS + 65535 * DESC_WORDS].reshape(65535, DESC_WORDS)
    one = _single_plan(lib, 8, 8, 8)
    assert p[1] == 65535 and p[6] == 1 and p.size == HEADER_WORDS + 65535 * DESC_WORDS + one.size - VIEW_HEADER_INTS
    assert (_i64(d[:, 16:18].copy()).reshape(-1) == HEADER_WORDS + 65535 * DESC_WORDS).all()  # one table for all
    assert (d[:, 0] == np.arange(65535) * d[0, 5]).all() and p[4] == 65535 * d[0, 5]
    assert (_i64(d[:, 20:22].copy()).reshape(-1) == np.arange(65535) * 192).all()  # 8 * 8 * 3 bytes each, already on the 16-byte grid


def test_plan_of_random_shape_lists_and_their_permutations(lib):
    rng = random.Random(4321)
    for size in (8, 32, 320):
        for _ in range(3):
            B = rng.randint(2, 24)
            pool = [(rng.randint(1, 64 * size if size == 8 else 700), rng.randint(1, 700)) for _ in range(max(2, B // 2))]
            shapes = []
            while len(shapes) < B:  # shapes repeat (shared tables); every one inside the 64x limit
                h, w = rng.choice(pool)
                if min(h, w) <= 64 * size and max(h, w) <= 71 * min(h, w):
                    shapes.append((h, w, rng.choice((3, 4))))
                else:
                    pool.append((rng.randint(1, 300), rng.randint(1, 300)))
            p = _check_plan(lib, shapes, size)
            perm = list(range(B))
            rng.shuffle(perm)
            permuted = [shapes[j] for j in perm]
            q = _check_plan(lib, permuted, size)
            dp = p[HEADER_WORDS:HEADER_WORDS + B * DESC_WORDS].reshape(B, DESC_WORDS)
            dq = q[HEADER_WORDS:HEADER_WORDS + B * DESC_WORDS].reshape(B, DESC_WORDS)
            for i, j in enumerate(perm):  # an image keeps its tiling in any company and place
                assert list(dq[i][2:16]) == list(dp[j][2:16]) and dq[i][18] == dp[j][18]
            assert (p[4], p[5], p[6], p.size) == (q[4], q[5], q[6], q.size)
            assert (_hash(p) != _hash(q)) == (permuted != shapes)


def test_hash_names_everything(lib):
    base = [(40, 56, 3), (56, 40, 4), (33, 65, 3)]
    h0 = _hash(_plan(lib, base, 32))
    others = {
        "size": _plan(lib, base, 33), "has_mask": _plan(lib, base, 32, has_mask=0),
        "H": _plan(lib, [(41, 56, 3)] + base[1:], 32), "W": _plan(lib, [base[0], (56, 41, 4), base[2]], 32),
        "channels": _plan(lib, base[:2] + [(33, 65, 4)], 32), "order": _plan(lib, [base[1], base[0], base[2]], 32),
        "B": _plan(lib, base[:2], 32),
    }
    hashes = {k: _hash(v) for k, v in others.items()}
    assert h0 not in hashes.values() and len(set(hashes.values())) == len(hashes), hashes
    assert _hash(_plan(lib, base, 32)) == h0


@pytest.mark.parametrize("shapes,size,code,word", [
    ([(40, 56, 3)], 7, E_SHAPE, b"8 .. 1024"), ([(40, 56, 3)], 1025, E_SHAPE, b"8 .. 1024"),
    ([(40, 56, 3), (513, 600, 3)], 8, E_SHAPE, b"exceeds 64"), ([(3000, 2049, 3)], 32, E_SHAPE, b"exceeds 64"),
    ([(40, 56, 2)], 32, E_SHAPE, b"channels"), ([(40, 56, 3), (40, 56, 5)], 32, E_SHAPE, b"channels"), ([(40, 56, 1)], 32, E_SHAPE, b"channels"),
    ([(0, 56, 3)], 32, E_SHAPE, b"positive"), ([(40, 56, 3), (40, -1, 3)], 32, E_SHAPE, b"positive"),
    ([(1 << 16, (1 << 14) + 1, 3)], 1024, E_SHAPE, b"2^30"),
])
def test_plan_limits_are_codes(lib, shapes, size, code, word):
    _plan(lib, shapes, size, expect=code)
    assert word in lib.curl_last_error(), lib.curl_last_error()
    if word != b"channels":  # (the size of a plan does not depend on the channel counts)
        hs, ws = _arr([s[0] for s in shapes]), _arr([s[1] for s in shapes])
        assert lib.curl_encoder_view_ragged_plan_bytes(len(shapes), hs.ctypes.data, ws.ctypes.data, size) == 0


def test_plan_argument_errors_are_codes(lib):
    hw, c = _arr([40]), _arr([3])
    nbytes = lib.curl_encoder_view_ragged_plan_bytes(1, hw.ctypes.data, hw.ctypes.data, 32)
    buf = np.zeros(nbytes // 4 + 4, dtype=np.int32)
    good = [1, hw.ctypes.data, hw.ctypes.data, c.ctypes.data, 1, 32, buf.ctypes.data, nbytes]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.curl_encoder_view_ragged_plan(*a)
    assert call() == 0
    for k in ("a1", "a2", "a3", "a6"):
        assert call(**{k: None}) == E_NULL and b"NULL" in lib.curl_last_error()
    assert call(a0=0) == E_SHAPE and b"positive" in lib.curl_last_error()
    assert call(a0=-3) == E_SHAPE
    assert call(a7=nbytes - 1) == E_WORKSPACE and b"too small" in lib.curl_last_error()
    assert call(a7=0) == E_WORKSPACE and b"too small" in lib.curl_last_error()
    assert call(a6=buf.ctypes.data + 4) == E_WORKSPACE and b"8-byte" in lib.curl_last_error()
    assert lib.curl_encoder_view_ragged_plan_bytes(0, hw.ctypes.data, hw.ctypes.data, 32) == 0
    assert lib.curl_encoder_view_ragged_plan_bytes(1, None, hw.ctypes.data, 32) == 0
    assert lib.curl_encoder_view_ragged_plan_bytes(1, hw.ctypes.data, None, 32) == 0
    big, three = _arr([8] * 65536), _arr([3] * 65536)
    assert lib.curl_encoder_view_ragged_plan_bytes(65536, big.ctypes.data, big.ctypes.data, 8) == 0
    room = np.zeros(HEADER_WORDS + DESC_WORDS * 65536 + 1024, dtype=np.int32)
    assert lib.curl_encoder_view_ragged_plan(65536, big.ctypes.data, big.ctypes.data, three.ctypes.data, 0, 8, room.ctypes.data, room.nbytes) == E_SHAPE
    assert b"65535" in lib.curl_last_error()


# ------------------------------------------------------------------ the launch entry: one argument list per fault
def _p(n, off=0):
    return ctypes.c_void_p((n << 20) + off)


SHAPES = [(40, 56, 3), (33, 65, 4)]


@pytest.fixture(scope="module")
def plans(lib):
    """name -> (host plan words, [image arena bytes, mask arena bytes]); 'zeros': no plan at all; 'stamp': one wrong bit."""
    out = {}
    for name, size, m in (("32", 32, 1), ("nomask", 32, 0), ("16", 16, 1)):
        p = _plan(lib, SHAPES, size, m)
        out[name] = (p, [int(v) for v in _i64(p[8:12])])
    out["zeros"] = (np.zeros_like(out["32"][0]), out["32"][1])
    wrong = out["32"][0].copy()
    wrong[0] ^= 1
    out["stamp"] = (wrong, out["32"][1])
    out["nomask"] = (out["nomask"][0], out["32"][1])  # (its own mask arena size is 0: the call's is the masked plan's)
    return out


def _launch(plans, **kw):
    a = dict(img=_p(1), mask=_p(2), plan="32", host="plan", dev=_p(3), plan_bytes=None, view=_p(4), mview=_p(5), size=32, flags=0,
             d_img=0, d_mask=0)
    a.update(kw)
    p, sizes = plans[a["plan"]]
    host = p.ctypes.data if a["host"] == "plan" else a["host"]
    pb = p.nbytes if a["plan_bytes"] is None else a["plan_bytes"]
    return [a["img"], sizes[0] + a["d_img"], a["mask"], sizes[1] + a["d_mask"], host, a["dev"], pb, a["view"], a["mview"], a["size"],
            a["flags"], None]


@pytest.mark.parametrize("kw,code,word", [
    (dict(img=None), E_NULL, b"NULL"), (dict(view=None), E_NULL, b"NULL"), (dict(host=None), E_NULL, b"host_plan"),
    (dict(dev=None), E_NULL, b"plan_dev"),
    (dict(plan="zeros"), E_WORKSPACE, b"no plan"), (dict(plan="stamp"), E_WORKSPACE, b"no plan"),
    (dict(size=16), E_WORKSPACE, b"another size"), (dict(plan="16"), E_WORKSPACE, b"another size"),
    (dict(plan="nomask"), E_WORKSPACE, b"without masks"),
    (dict(dev=_p(3, 4)), E_WORKSPACE, b"8-byte"), (dict(plan_bytes=4 * (HEADER_WORDS + 2 * DESC_WORDS)), E_WORKSPACE, b"too small"),
    (dict(plan_bytes=0), E_WORKSPACE, b"too small"),
    (dict(d_img=-1), E_WORKSPACE, b"image arena"), (dict(d_mask=-1), E_WORKSPACE, b"mask arena"),
    (dict(mview=None), E_MASK, b"both"), (dict(mask=None), E_MASK, b"both"),
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x400000), E_FLAGS, b"flag"), (dict(flags=0x80000000), E_FLAGS, b"flag"),
    (dict(view=_p(4, 2)), E_SHAPE, b"4-byte"), (dict(mview=_p(5, 1)), E_SHAPE, b"4-byte"),
])
def test_launch_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_encoder_view_ragged_u8hwc(*_launch(plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


def test_a_misaligned_host_plan_is_a_code(lib, plans):
    p = plans["32"][0]
    room = np.zeros(p.size + 2, dtype=np.int32)
    room[1:1 + p.size] = p
    assert lib.curl_encoder_view_ragged_u8hwc(*_launch(plans, host=room.ctypes.data + 4)) == E_WORKSPACE
    assert b"8-byte" in lib.curl_last_error()


# ------------------------------------------------------------------ ops.encoder_view_u8hwc_ragged on the host
def test_op_checks_its_arguments_on_the_host():
    import torch
    from curl_amd import ops
    imgs = [torch.zeros(h, w, c, dtype=torch.uint8) for h, w, c in ((12, 20, 3), (33, 65, 4), (40, 64, 3))]
    ms = [t[..., 0].contiguous() for t in imgs]
    for images, masks in ((imgs, ms), (ops.RaggedBytes.pack(imgs), ops.RaggedBytes.pack(ms)), (imgs, None)):
        with pytest.raises(RuntimeError, match="HIP device only"):  # no CPU fallback
            ops.encoder_view_u8hwc_ragged(images, masks)
    with pytest.raises(ValueError):
        ops.encoder_view_u8hwc_ragged([imgs[0].float()], None)                 # dtype
    with pytest.raises(ValueError):
        ops.encoder_view_u8hwc_ragged([imgs[0][..., :2]], None)                # channels
    with pytest.raises(ValueError):
        ops.encoder_view_u8hwc_ragged(imgs, ms[:2])                            # one mask per image
    with pytest.raises(ValueError):
        ops.encoder_view_u8hwc_ragged(imgs, [ms[0], ms[1], ms[1]])             # masks of the images' sizes
    with pytest.raises(ValueError):
        ops.encoder_view_u8hwc_ragged(imgs, [ms[0], ms[1], imgs[2]])           # a mask is [H,W]
    with pytest.raises(ValueError):
        ops.encoder_view_u8hwc_ragged(imgs[:2] + [torch.zeros(0, 4, 3, dtype=torch.uint8)])
    view, mview = ops.encoder_view_u8hwc_ragged([], None, size=32)
    assert view.shape == (0, 3, 32, 32) and view.dtype == torch.float32 and mview is None
    view, mview = ops.encoder_view_u8hwc_ragged([], [])
    assert view.shape == (0, 3, 320, 320) and mview.shape == (0, 1, 320, 320)


def test_view_ragged_plans_are_cached_and_bounded():
    from curl_amd import ops
    first = ops._view_ragged_plan([(40, 56)], [3], True, 32, "cpu")
    n = len(ops._view_ragged_plans)
    assert ops._view_ragged_plan([(40, 56)], [3], True, 32, "cpu") is first and len(ops._view_ragged_plans) == n  # kept
    assert first.img_off == [0] and first.img_bytes == 40 * 56 * 3 and first.mask_bytes == 40 * 56
    for k in range(40):
        ops._view_ragged_plan([(k + 8, 9)], [4], False, 8, "cpu")
    assert len(ops._view_ragged_plans) <= ops._VIEW_RAGGED_PLANS_KEPT
    with pytest.raises(ValueError):
        ops._view_ragged_plan([(513, 600)], [3], True, 8, "cpu")  # beyond 64x: the library's code, raised


def test_python_surface_exists():
    import inspect
    from curl_amd import infer, ops
    sig = inspect.signature(ops.encoder_view_u8hwc_ragged).parameters
    assert list(sig) == ["images", "masks", "size"] and sig["masks"].default is None and sig["size"].default == 320
    src = inspect.getsource(infer.enhance_many)
    assert "encoder_view_u8hwc_ragged" in src and "ops.encoder_view_u8hwc(" not in src
