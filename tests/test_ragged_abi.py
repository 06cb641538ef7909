"""The ragged byte entries (include/curl_hip_ragged.h) without a device: the header compiles as C99 and C++17, the entries are
exported and bound from _lib.SIGNATURES_RAGGED beside the four unchanged tables; the host-built plan -- offsets, arena sizes,
classes, tiling and the workgroup -> (image, tile) lookup, restated here -- for fixed and seeded random shape lists and five
operators; every limit and every single-fault argument list of the two launch entries a return code with its text before any
HIP call (fake device pointers); and the host side of ops.RaggedBytes.

(The limit "each arena < 2^63 bytes" cannot be reached through the other limits -- 65 535 images of 2^30 pixels of 4 bytes
are 2^48 bytes -- so no argument list exists for it.)"""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
NAMES = {"curl_ragged_plan_bytes": 2, "curl_ragged_plan": 8, "curl_ragged_arena_bytes": 4, "curl_trispace_fwd_ragged_u8hwc": 13,
         "curl_layer_fwd_ragged_u8hwc": 20}
TRI, LAYER = "curl_trispace_fwd_ragged_u8hwc", "curl_layer_fwd_ragged_u8hwc"
HEADER_WORDS, DESC_WORDS, STAMP, ALIGN = 32, 16, 0x52474731, 16
# the operators: 126 (row tiles), 35, one lower order per variable count (CURL_POLY_COEFFS(56, 3), (10, 2)), the layer
OPS = {"126": 126, "35": 35, "56": 56 | (3 << 16), "10": 10 | (2 << 16), "layer": 0}
COUNT = {"126": 126, "35": 35, "56": 56, "10": 10, "layer": 0}


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl = dict(_declared("curl_hip_ragged.h"))
    assert set(decl) == set(_lib.SIGNATURES_RAGGED) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_RAGGED[name][1]) == n, name
        fn = getattr(lib, name)
        assert fn.restype is _lib.SIGNATURES_RAGGED[name][0] and list(fn.argtypes) == _lib.SIGNATURES_RAGGED[name][1]
    assert set(_lib.SIGNATURES) == {n for n, _ in _declared("curl_hip.h")}
    assert set(_lib.SIGNATURES_GRAD) == {n for n, _ in _declared("curl_hip_grad.h")}
    assert set(_lib.SIGNATURES_VIEW) == {n for n, _ in _declared("curl_hip_view.h")}
    assert set(_lib.SIGNATURES_FG) == {n for n, _ in _declared("curl_hip_fg.h")}
    assert lib.curl_version() >= 116
    # the layout constants of the header, as _lib.py and this file restate them
    src = open(f"{ROOT}/include/curl_hip_ragged.h").read()
    consts = {k: int(v, 0) for k, v in re.findall(r"#define CURL_RAGGED_(\w+) (\w+)", src)}
    assert consts == {"ALIGN": ALIGN, "STAMP": STAMP, "HEADER_WORDS": HEADER_WORDS, "DESC_WORDS": DESC_WORDS, "MAX_IMAGES": 65535}
    assert (_lib.RAGGED_ALIGN, _lib.RAGGED_STAMP, _lib.RAGGED_HEADER_WORDS, _lib.RAGGED_DESC_WORDS, _lib.RAGGED_MAX_IMAGES) == \
        (ALIGN, STAMP, HEADER_WORDS, DESC_WORDS, 65535)


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_ragged.h"\n'
                   "int main(void) {\n"
                   "  int hw[1] = {8}, c[1] = {3};\n"
                   "  long long buf[(CURL_RAGGED_HEADER_WORDS + CURL_RAGGED_DESC_WORDS) / 2];\n"
                   "  size_t a, b, d;\n"
                   "  if (curl_ragged_plan_bytes(1, 126) != sizeof buf) return 3;\n"
                   "  if (curl_ragged_plan(1, hw, hw, c, 0, 126, buf, sizeof buf) != CURL_OK || curl_ragged_arena_bytes(buf, &a, &b, &d)) return 4;\n"
                   "  if (*(int*)buf != CURL_RAGGED_STAMP || a % CURL_RAGGED_ALIGN != 0 || CURL_RAGGED_MAX_IMAGES != 65535) return 5;\n"
                   "  if (curl_trispace_fwd_ragged_u8hwc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 126, 0, 0) != CURL_E_NULL) return 2;\n"
                   "  return curl_layer_fwd_ragged_u8hwc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, CURL_K_UNEVEN(16, 14), 16, 16, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


# ------------------------------------------------------------------ the plan
def _arr(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _plan(lib, shapes, op, has_mask=1, expect=0):
    """-> the plan's int32 words (or the return code when it is not `expect` = 0)."""
    B = len(shapes)
    hs, ws, cs = (_arr([s[k] for s in shapes]) for k in range(3))
    nbytes = lib.curl_ragged_plan_bytes(B, op)
    assert nbytes == 4 * (HEADER_WORDS + DESC_WORDS * B)
    buf = np.full(nbytes // 4 + 2, -1, dtype=np.int32)
    assert buf.ctypes.data % 8 == 0
    rc = lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, op, buf.ctypes.data, nbytes)
    assert rc == expect, (rc, lib.curl_last_error())
    assert (buf[-2:] == -1).all()  # nothing past the plan's bytes
    return buf[:-2]


def _i64(words):
    return np.ascontiguousarray(words).view(np.int64)


def _lookup(first, wg):
    """The kernel's search, restated: the last descriptor whose first workgroup is <= wg."""
    lo, hi = 0, len(first)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if first[mid] <= wg:
            lo = mid
        else:
            hi = mid
    return lo


def _row_threads(units_rows, fold_weight):
    """[(units, H)] of one launch -> its block size: the fewest wave slots plus row folds summed over the rows (a fold weighs
    half a wave on the dword path, two waves on the byte path), the larger on a tie."""
    best_t, best = 64, None
    for t in (64, 128, 192, 256):
        cost = sum((2 * -(-u // t) * (t // 64) + fold_weight * -(-u // t)) * h for u, h in units_rows)
        if best is None or cost <= best:
            best_t, best = t, cost
    return best_t


def _check_plan(lib, shapes, name, has_mask=1):
    op, rows = OPS[name], name == "126"
    p = _plan(lib, shapes, op, has_mask)
    B = len(shapes)
    H, W, C = (np.array([s[k] for s in shapes], dtype=np.int64) for k in range(3))
    d = p[HEADER_WORDS:].reshape(B, DESC_WORDS)
    dword = (W % 4 == 0) if rows else ((H * W) % 4 == 0)
    n_dword = int(dword.sum())
    assert (p[0], p[1], p[2], p[3]) == (STAMP, B, COUNT[name], has_mask)
    assert (p[4], p[5], p[6]) == ((n_dword > 0) + (n_dword < B), n_dword, B - n_dword)
    assert (p[11] == 0) and (p[20:HEADER_WORDS] == 0).all() and (d[:, 9] == 0).all()
    # class membership and order: the dword class's descriptors in index order, then the byte class's
    idx = d[:, 1].astype(np.int64)
    assert list(idx) == [i for i in range(B) if dword[i]] + [i for i in range(B) if not dword[i]]
    assert (d[:, 2] == H[idx]).all() and (d[:, 3] == W[idx]).all() and (d[:, 4] == C[idx]).all()
    # offsets: multiples of 16, increasing in index order, no overlap, only the padding alignment needs; arena sizes
    off = _i64(d[:, 10:16].copy()).reshape(B, 3)
    by_image = np.empty_like(off)
    by_image[idx] = off
    sizes = _i64(p[12:18])
    for k, per_px in ((0, C), (1, np.ones(B, dtype=np.int64) if has_mask else np.zeros(B, dtype=np.int64)), (2, np.full(B, 3))):
        o, nb = by_image[:, k], H * W * per_px
        if k == 1 and not has_mask:
            assert (o == 0).all() and sizes[1] == 0
            continue
        assert (o % ALIGN == 0).all() and o[0] == 0
        assert (o[1:] == (o[:-1] + nb[:-1] + ALIGN - 1) // ALIGN * ALIGN).all()  # increasing, disjoint, minimal padding
        assert sizes[k] == o[-1] + nb[-1]
    out = [ctypes.c_size_t() for _ in range(3)]
    assert lib.curl_ragged_arena_bytes(p.ctypes.data, *(ctypes.addressof(v) for v in out)) == 0
    assert [v.value for v in out] == list(sizes)
    # tiling of each launch, and the walk of every workgroup id
    for cls, (lo, hi) in enumerate(((0, n_dword), (n_dword, B))):
        threads, grid = int(p[7 + 2 * cls]), int(p[8 + 2 * cls])
        if lo == hi:
            assert threads == 0 and grid == 0
            continue
        vec = 4 if cls == 0 else 1
        dd = d[lo:hi].astype(np.int64)
        n = dd[:, 2] * dd[:, 3] // vec
        assert (dd[:, 5] == n).all()
        if rows:
            units = dd[:, 3] // vec
            assert threads == _row_threads(list(zip(units.tolist(), dd[:, 2].tolist())), 1 if cls == 0 else 4)
            segs = -(-units // threads)
            assert (dd[:, 6] == units).all() and (dd[:, 7] == segs).all() and (dd[:, 8] == segs * dd[:, 2]).all()
        else:
            assert threads == 256 and (dd[:, 6] == 0).all() and (dd[:, 7] == 0).all() and (dd[:, 8] == -(-n // 256)).all()
        first, tiles = dd[:, 0], dd[:, 8]
        assert first[0] == 0 and (first[1:] == np.cumsum(tiles)[:-1]).all() and grid == tiles.sum() and 0 < grid < 2 ** 31
        wg = np.arange(grid, dtype=np.int64)
        which = np.searchsorted(first, wg, side="right") - 1  # = _lookup, for every workgroup id at once
        probe = sorted({0, grid - 1, grid // 2} | {int(f) for f in first[:64]} | {int(f) - 1 for f in first[1:64]})
        assert all(_lookup(first, w) == which[w] for w in probe)
        chunk = wg - first[which]
        assert (chunk >= 0).all() and (chunk < tiles[which]).all()
        # every (image, tile) exactly once, nothing else: per image the chunks are 0 .. tiles - 1 in order
        assert (np.bincount(which, minlength=hi - lo) == tiles).all()
        assert (chunk == wg - np.repeat(first, tiles)).all()
        # the tiles cover every group of the image: flat tile t holds groups [256 t, 256 t + 256), row tile (r, s) holds
        # groups r * units + [threads * s, threads * s + threads)
        if rows:
            assert (dd[:, 7] * threads >= dd[:, 6]).all() and ((dd[:, 7] - 1) * threads < dd[:, 6]).all()
        else:
            assert (tiles * 256 >= n).all() and ((tiles - 1) * 256 < n).all()
    return p


WIDTHS = [(3, w, 3 + (k & 1)) for k, w in enumerate((1, 3, 4, 1023, 1024, 1025, 1028, 1500))]
GPU_BATCH = [(1, 1, 3), (3, 5, 3), (4, 8, 4), (7, 9, 4), (12, 20, 3), (2, 1028, 3), (3, 1500, 4), (33, 65, 3), (40, 64, 3)]
FIXED = {
    "one": [(7, 9, 3)],
    "one_dword": [(8, 8, 4)],
    "tiny_beside_huge": [(1, 1, 3), (32768, 32768, 4)],
    "widths": WIDTHS,
    "all_dword": [(4, 8, 3), (2, 1028, 4), (40, 64, 3), (8, 1500, 3)],
    "all_byte": [(1, 1, 3), (3, 5, 4), (7, 9, 3), (33, 65, 4)],
    "mixed": GPU_BATCH,
}


@pytest.mark.parametrize("name", list(OPS))
@pytest.mark.parametrize("case", list(FIXED))
def test_plan_of_fixed_shape_lists(lib, case, name):
    _check_plan(lib, FIXED[case], name)
    _check_plan(lib, FIXED[case], name, has_mask=0)


@pytest.mark.parametrize("name", list(OPS))
def test_plan_of_65535_images(lib, name):
    p = _check_plan(lib, [(1, 1, 3)] * 65535, name)
    assert p[8] == 0 and p[10] == 65535  # one workgroup each, all in the byte class


@pytest.mark.parametrize("name", list(OPS))
def test_plan_of_random_shape_lists_and_their_permutations(lib, name):
    rng = random.Random(12345 + COUNT[name])
    for _ in range(6):
        B = rng.randint(2, 40)
        shapes = [(rng.randint(1, 90), rng.choice((1, 2, 3, 4, 5, 8, 12, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1028, 1500)),
                   rng.choice((3, 4))) for _ in range(B)]
        p = _check_plan(lib, shapes, name)
        perm = list(range(B))
        rng.shuffle(perm)
        permuted = [shapes[j] for j in perm]
        q = _check_plan(lib, permuted, name)
        # the plan of the permuted list is the permuted plan: image perm[i]'s descriptor but for its place (first workgroup,
        # index, offsets: _check_plan holds those to the rule), the same block sizes and grids
        assert list(p[4:11]) == list(q[4:11])
        dp = {int(r[1]): r for r in p[HEADER_WORDS:].reshape(B, DESC_WORDS)}
        dq = {int(r[1]): r for r in q[HEADER_WORDS:].reshape(B, DESC_WORDS)}
        for i, j in enumerate(perm):
            assert list(dq[i][2:10]) == list(dp[j][2:10])
        assert (_i64(p[18:20])[0] != _i64(q[18:20])[0]) == (permuted != shapes)
    # the hash names the operator and the masks too
    a, b = _plan(lib, GPU_BATCH, OPS[name], 1), _plan(lib, GPU_BATCH, OPS[name], 0)
    assert _i64(a[18:20])[0] != _i64(b[18:20])[0]


def test_row_block_size_of_one_shape_is_the_single_image_entrys(lib):
    """Batches of one shape: the block size host_api.inc's row_blocks picks for that image alone."""
    for shape, word, want in (((512, 341, 4), 9, 192), ((341, 512, 4), 7, 128), ((1000, 1500, 3), 7, 192)):
        for B in (1, 8):
            assert _plan(lib, [shape] * B, 126)[word] == want, (shape, B)


def test_plan_hash_differs_between_operators(lib):
    hashes = {name: int(_i64(_plan(lib, GPU_BATCH, op)[18:20])[0]) for name, op in OPS.items()}
    assert len(set(hashes.values())) == len(OPS)


@pytest.mark.parametrize("shapes,op,code,word", [
    ([(0, 4, 3)], 126, E_SHAPE, b"positive"), ([(4, -1, 3)], 0, E_SHAPE, b"positive"),
    ([(32768, 32769, 3)], 35, E_SHAPE, b"2^30"), ([(4, 4, 3), (1 << 15, (1 << 15) + 1, 4)], 0, E_SHAPE, b"2^30"),
    ([(4, 4, 2)], 126, E_SHAPE, b"channels"), ([(4, 4, 5)], 0, E_SHAPE, b"channels"), ([(4, 4, 1)], 35, E_SHAPE, b"channels"),
    ([(1 << 30, 1, 3)] * 3, 126, E_SHAPE, b"grid"),  # row tiles of one pixel: 2^30 workgroups per image
])
def test_plan_limits_are_codes(lib, shapes, op, code, word):
    _plan(lib, shapes, op, expect=code)
    assert word in lib.curl_last_error(), lib.curl_last_error()


def test_plan_argument_errors_are_codes(lib):
    hw, c = _arr([8]), _arr([3])
    buf = np.zeros(HEADER_WORDS + DESC_WORDS + 4, dtype=np.int32)
    nbytes = lib.curl_ragged_plan_bytes(1, 126)
    good = [1, hw.ctypes.data, hw.ctypes.data, c.ctypes.data, 1, 126, buf.ctypes.data, nbytes]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.curl_ragged_plan(*a)
    assert call() == 0
    for k in ("a1", "a2", "a3", "a6"):
        assert call(**{k: None}) == E_NULL and b"NULL" in lib.curl_last_error()
    assert call(a0=0) == E_SHAPE and b"positive" in lib.curl_last_error()
    assert call(a0=-3) == E_SHAPE
    assert call(a7=nbytes - 1) == E_WORKSPACE and b"too small" in lib.curl_last_error()
    assert call(a6=buf.ctypes.data + 4) == E_WORKSPACE and b"8-byte" in lib.curl_last_error()
    for bad in (125, 56, 56 | (2 << 16), 1):
        assert call(a5=bad) == E_KNOTS and b"num_coeffs" in lib.curl_last_error()
        assert lib.curl_ragged_plan_bytes(1, bad) == 0
    assert lib.curl_ragged_plan_bytes(0, 126) == 0 and lib.curl_ragged_plan_bytes(65536, 0) == 0
    big = _arr([1] * 65536)
    three = _arr([3] * 65536)
    room = np.zeros(HEADER_WORDS + DESC_WORDS * 65536, dtype=np.int32)
    assert lib.curl_ragged_plan(65536, big.ctypes.data, big.ctypes.data, three.ctypes.data, 0, 0, room.ctypes.data, room.nbytes) == E_SHAPE
    assert b"65535" in lib.curl_last_error()
    sz = ctypes.c_size_t()
    assert lib.curl_ragged_arena_bytes(None, *[ctypes.addressof(sz)] * 3) == E_NULL
    assert lib.curl_ragged_arena_bytes(buf.ctypes.data, None, ctypes.addressof(sz), ctypes.addressof(sz)) == E_NULL
    assert lib.curl_ragged_arena_bytes(room.ctypes.data, *[ctypes.addressof(sz)] * 3) == E_WORKSPACE and b"no plan" in lib.curl_last_error()


# ------------------------------------------------------------------ the launch entries: one argument list per fault
def _p(n, off=0):
    return ctypes.c_void_p((n << 20) + off)


SHAPES = [(8, 8, 3), (5, 7, 4)]


@pytest.fixture(scope="module")
def plans(lib):
    """name -> (host plan words, arena sizes); 'nomask': 126 without masks; 'zeros': no plan at all."""
    out = {}
    for name, op, m in (("126", 126, 1), ("35", 35, 1), ("layer", 0, 1), ("nomask", 126, 0)):
        p = _plan(lib, SHAPES, op, m)
        out[name] = (p, [int(v) for v in _i64(p[12:18])])
    out["zeros"] = (np.zeros_like(out["126"][0]), out["126"][1])
    return out


def _common(plans, a):
    p, sizes = plans[a["plan"]]
    host = p.ctypes.data if a["host"] == "plan" else a["host"]
    pb = p.nbytes if a["plan_bytes"] is None else a["plan_bytes"]
    return host, pb, [sizes[k] + a[d] for k, d in enumerate(("d_img", "d_mask", "d_out"))]


def _tri(plans, **kw):
    a = dict(img=_p(1), coeffs=_p(2), mask=_p(3), out=_p(4), plan="126", host="plan", dev=_p(5), plan_bytes=None, nc=126, flags=0,
             d_img=0, d_mask=0, d_out=0)
    a.update(kw)
    host, pb, (ib, mb, ob) = _common(plans, a)
    return [a["img"], ib, a["coeffs"], a["mask"], mb, a["out"], ob, host, a["dev"], pb, a["nc"], a["flags"], None]


def _layer(lib, plans, **kw):
    a = dict(img=_p(1), rawL=_p(2), rawR=_p(6), rawH=_p(7), mask=_p(3), out=_p(4), reg=_p(8), ws=_p(9), ws_bytes=None, plan="layer",
             host="plan", dev=_p(5), plan_bytes=None, Kl=16, Kr=16, Kh=16, flags=0, d_img=0, d_mask=0, d_out=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.curl_workspace_bytes(len(SHAPES), 160)
    host, pb, (ib, mb, ob) = _common(plans, a)
    return [a["img"], ib, a["rawL"], a["rawR"], a["rawH"], a["mask"], mb, a["out"], ob, a["reg"], a["ws"], a["ws_bytes"], host, a["dev"],
            pb, a["Kl"], a["Kr"], a["Kh"], a["flags"], None]


COMMON = [
    (dict(img=None), E_NULL, b"NULL"), (dict(out=None), E_NULL, b"NULL"), (dict(host=None), E_NULL, b"host_plan"),
    (dict(dev=None), E_NULL, b"plan_dev"),
    (dict(d_img=-1), E_WORKSPACE, b"image arena"), (dict(d_mask=-1), E_WORKSPACE, b"mask arena"), (dict(d_out=-1), E_WORKSPACE, b"out arena"),
    (dict(img=_p(1, 1)), E_SHAPE, b"4-byte"), (dict(mask=_p(3, 1)), E_SHAPE, b"4-byte"), (dict(out=_p(4, 1)), E_SHAPE, b"4-byte"),
    (dict(out=_p(4, 2)), E_SHAPE, b"4-byte"),
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x400000), E_FLAGS, b"flag"), (dict(flags=0x80000000), E_FLAGS, b"flag"),
    (dict(plan="zeros"), E_WORKSPACE, b"no plan"),
    (dict(dev=_p(5, 4)), E_WORKSPACE, b"8-byte"), (dict(plan_bytes=4 * (HEADER_WORDS + 2 * DESC_WORDS) - 1), E_WORKSPACE, b"too small"),
]


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(coeffs=None), E_NULL, b"coeffs"),
    (dict(plan="35"), E_WORKSPACE, b"another operator"), (dict(plan="layer"), E_WORKSPACE, b"another operator"),
    (dict(plan="35", nc=10 | (2 << 16)), E_WORKSPACE, b"another operator"),
    (dict(plan="nomask"), E_WORKSPACE, b"without masks"),
    (dict(nc=125), E_KNOTS, b"num_coeffs"), (dict(nc=0), E_KNOTS, b"num_coeffs"), (dict(nc=56), E_KNOTS, b"num_coeffs"),
    (dict(nc=56 | (2 << 16)), E_KNOTS, b"order"),
    (dict(coeffs=_p(2, 4)), E_SHAPE, b"8-byte"), (dict(coeffs=_p(2, 2), nc=35, plan="35"), E_SHAPE, b"4-byte"),
])
def test_trispace_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_trispace_fwd_ragged_u8hwc(*_tri(plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(plan="126"), E_WORKSPACE, b"another operator"), (dict(plan="35"), E_WORKSPACE, b"another operator"),
    (dict(rawL=None), E_NULL, b"rawL/rawR/rawH"), (dict(rawR=None), E_NULL, b"rawL/rawR/rawH"), (dict(rawH=None), E_NULL, b"rawL/rawR/rawH"),
    (dict(Kl=1), E_KNOTS, b"knots per curve"), (dict(Kr=300), E_KNOTS, b"knots per curve"), (dict(Kh=-1), E_KNOTS, b"knots per curve"),
    (dict(Kh=16 | (17 << 16)), E_KNOTS, b"last curve"),
    (dict(ws=None), E_WORKSPACE, b"NULL"), (dict(ws=_p(9, 4)), E_WORKSPACE, b"16-byte"), (dict(ws_bytes=8), E_WORKSPACE, b"too small"),
])
def test_layer_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_layer_fwd_ragged_u8hwc(*_layer(lib, plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


# ------------------------------------------------------------------ ops.RaggedBytes on the host
def test_ragged_bytes_pack_on_the_host():
    import torch
    from curl_amd import ops
    g = torch.Generator().manual_seed(3)
    imgs = [torch.randint(0, 256, (h, w, c), dtype=torch.uint8, generator=g) for h, w, c in GPU_BATCH]
    mixed = [t if k % 2 else t.numpy() for k, t in enumerate(imgs)]  # tensors and numpy arrays alike
    rb = ops.RaggedBytes.pack(mixed)
    assert len(rb) == 9 and rb.shapes == [(h, w) for h, w, _ in GPU_BATCH] and rb.channels == [c for _, _, c in GPU_BATCH]
    assert rb.arena.dtype == torch.uint8 and rb.arena.dim() == 1 and rb.device.type == "cpu"
    end = 0
    for (h, w, c), o in zip(GPU_BATCH, rb.offsets):
        assert o % 16 == 0 and o == (end + 15) // 16 * 16
        end = o + h * w * c
    assert rb.arena.numel() == end
    assert all(torch.equal(v, t) and v.shape == t.shape for v, t in zip(rb.images(), imgs))
    assert rb.image(3)[None].shape == (1, 7, 9, 4) and rb.image(3).data_ptr() == rb.arena.data_ptr() + rb.offsets[3]  # a view
    masks = ops.RaggedBytes.pack([t[..., 0].contiguous() for t in imgs])
    assert masks.channels == [1] * 9 and masks.image(4).shape == (12, 20) and torch.equal(masks.image(4), imgs[4][..., 0])
    assert all(o % 16 == 0 for o in masks.offsets)
    sliced = ops.RaggedBytes.pack([imgs[3].numpy()[::2, 1:]])  # a strided array
    assert torch.equal(sliced.image(0), imgs[3][::2, 1:])
    for bad in ([imgs[0].float()], [imgs[0][..., :2]], [imgs[0][None]], [torch.zeros(0, 5, 3, dtype=torch.uint8)],
                [torch.zeros(5, 0, 3, dtype=torch.uint8)], [imgs[1], imgs[1][..., 0]], [np.zeros((4, 4, 3), np.int16)]):
        with pytest.raises(ValueError):
            ops.RaggedBytes.pack(bad)
    assert len(ops.RaggedBytes.pack([])) == 0


def test_ragged_ops_on_the_host():
    import torch
    from curl_amd import ops
    imgs = [torch.zeros(h, w, c, dtype=torch.uint8) for h, w, c in GPU_BATCH[:3]]
    ms = [t[..., 0].contiguous() for t in imgs]
    coeffs = torch.zeros(3, 3, 3, 126)
    knots = [torch.zeros(3, n) for n in (48, 48, 64)]
    for images in (imgs, ops.RaggedBytes.pack(imgs)):
        with pytest.raises(RuntimeError, match="HIP device only"):  # no CPU fallback
            ops.trispace_forward_u8hwc_ragged(images, coeffs, ms)
        with pytest.raises(RuntimeError, match="HIP device only"):
            ops.curl_layer_forward_u8hwc_ragged(images, *knots)
    with pytest.raises(ValueError):  # (what the functions refuse of masks on a device: tests/test_gpu_ragged.py)
        ops.trispace_forward_u8hwc_ragged(imgs[:2] + [torch.zeros(0, 4, 3, dtype=torch.uint8)], coeffs)
    out = ops.trispace_forward_u8hwc_ragged([], coeffs[:0])
    assert len(out) == 0 and out.arena.numel() == 0 and out.images() == []
    out, reg = ops.curl_layer_forward_u8hwc_ragged([], *[k[:0] for k in knots])
    assert len(out) == 0 and reg.shape == (0,)


def test_ragged_plans_are_cached_and_bounded():
    from curl_amd import ops
    first = ops.RaggedBytes.layout([(5, 5)], [3])
    n = len(ops._ragged_plans)
    assert ops.RaggedBytes.layout([(5, 5)], [3]) == first and len(ops._ragged_plans) == n  # kept
    for k in range(40):
        ops.RaggedBytes.layout([(k + 1, 7)], [4])
    assert len(ops._ragged_plans) <= ops._RAGGED_PLANS_KEPT


def test_python_surface_exists():
    import inspect
    from curl_amd import infer, infer_dir, ops
    assert list(inspect.signature(ops.trispace_forward_u8hwc_ragged).parameters) == ["images", "coeffs", "white_masks"]
    assert list(inspect.signature(ops.curl_layer_forward_u8hwc_ragged).parameters) == ["images", "L", "R", "H", "white_masks"]
    sig = inspect.signature(infer.enhance_many).parameters
    assert list(sig) == ["net", "images_u8", "masks_u8", "device", "view", "batch_size"] and sig["view"].default == "pil" and sig["batch_size"].default == 32
    assert callable(infer_dir.main)
    with pytest.raises(SystemExit):
        infer_dir.main(["--img_dir", "x"])  # the other folders and the model are required
