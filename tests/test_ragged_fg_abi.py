"""The foreground-aware ragged byte entries (include/curl_hip_ragged_fg.h) without a device: the header compiles as C99 and
C++17, the two entries are declared, exported and bound from _lib.SIGNATURES_RAGGED_FG with the siblings' argument lists beside
the six unchanged tables; every single-fault argument list of the two a return code with its text before any HIP call (fake
device pointers); the host side of the two ops, infer.enhance_many_foreground and infer_dir --foreground_masks."""
import ctypes
import inspect
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
TRI, LAYER = "curl_trispace_fwd_ragged_fg_u8hwc", "curl_layer_fwd_ragged_fg_u8hwc"
NAMES = {TRI: 13, LAYER: 20}
SIBLING = {TRI: "curl_trispace_fwd_ragged_u8hwc", LAYER: "curl_layer_fwd_ragged_u8hwc"}
HEADER_WORDS, DESC_WORDS = 32, 16
TABLES = {"SIGNATURES": "curl_hip.h", "SIGNATURES_GRAD": "curl_hip_grad.h", "SIGNATURES_VIEW": "curl_hip_view.h",
          "SIGNATURES_FG": "curl_hip_fg.h", "SIGNATURES_RAGGED": "curl_hip_ragged.h", "SIGNATURES_VIEW_RAGGED": "curl_hip_view_ragged.h"}


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


def _types(args):
    """A declaration's argument list without the names: the C types, one per argument."""
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in args.split(",")]


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl, sibling = dict(_declared("curl_hip_ragged_fg.h")), dict(_declared("curl_hip_ragged.h"))
    assert set(decl) == set(_lib.SIGNATURES_RAGGED_FG) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_RAGGED_FG[name][1]) == n, name
        assert _types(decl[name]) == _types(sibling[SIBLING[name]]), name  # the sibling's argument list, type by type
        assert _lib.SIGNATURES_RAGGED_FG[name] == _lib.SIGNATURES_RAGGED[SIBLING[name]]
        fn = getattr(lib, name)  # exported
        assert fn.restype is _lib.SIGNATURES_RAGGED_FG[name][0] and list(fn.argtypes) == _lib.SIGNATURES_RAGGED_FG[name][1]
    for table, header in TABLES.items():  # the six existing tables still equal their headers
        assert set(getattr(_lib, table)) == {n for n, _ in _declared(header)}, table
    assert lib.curl_version() >= 118


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_ragged_fg.h"\n'
                   "int main(void) {\n"
                   "  int hw[1] = {8}, c[1] = {3};\n"
                   "  long long buf[(CURL_RAGGED_HEADER_WORDS + CURL_RAGGED_DESC_WORDS) / 2];\n"
                   "  if (curl_ragged_plan(1, hw, hw, c, 1, 126, buf, sizeof buf) != CURL_OK) return 3;\n"
                   "  if (curl_trispace_fwd_ragged_fg_u8hwc(0, 0, 0, 0, 0, 0, 0, buf, 0, 0, 126, 0, 0) != CURL_E_NULL) return 2;\n"
                   "  return curl_layer_fwd_ragged_fg_u8hwc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, buf, 0, 0, CURL_K_UNEVEN(16, 14), 16, 16, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


# ------------------------------------------------------------------ the launch entries: one argument list per fault
def _plan(lib, shapes, op, has_mask=1):
    B = len(shapes)
    hs, ws, cs = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(3))
    nbytes = lib.curl_ragged_plan_bytes(B, op)
    assert nbytes == 4 * (HEADER_WORDS + DESC_WORDS * B)
    buf = np.zeros(nbytes // 4 + 2, dtype=np.int32)  # (room for the plan four bytes further on: the misaligned host plan)
    assert buf.ctypes.data % 8 == 0
    assert lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, op, buf.ctypes.data, nbytes) == 0
    return buf


def _p(n, off=0):
    return ctypes.c_void_p((n << 20) + off)


SHAPES = [(8, 8, 3), (5, 7, 4)]


@pytest.fixture(scope="module")
def plans(lib):
    """name -> (host plan words, arena sizes); 'nomask': 126 without masks; 'zeros': no plan at all; 'stamp': one bit of the
    stamp wrong; 'shifted': the 126 plan four bytes off the 8-byte grid."""
    out = {}
    for name, op, m in (("126", 126, 1), ("35", 35, 1), ("layer", 0, 1), ("nomask", 126, 0), ("nomask_layer", 0, 0)):
        p = _plan(lib, SHAPES, op, m)
        out[name] = (p, [int(v) for v in np.ascontiguousarray(p[12:18]).view(np.int64)])
    out["zeros"] = (np.zeros_like(out["126"][0]), out["126"][1])
    for name in ("126", "layer"):
        bad = out[name][0].copy()
        bad[0] ^= 1
        out["stamp_" + name] = (bad, out[name][1])
        shifted = np.zeros(out[name][0].size + 1, dtype=np.int32)
        shifted[1:] = out[name][0]
        out["shifted_" + name] = (shifted[1:], out[name][1])
        assert shifted[1:].ctypes.data % 8 == 4
    return out


def _common(plans, a):
    p, sizes = plans[a["plan"]]
    host = p.ctypes.data if a["host"] == "plan" else a["host"]
    pb = 4 * (HEADER_WORDS + len(SHAPES) * DESC_WORDS) if a["plan_bytes"] is None else a["plan_bytes"]
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
    (dict(mask=None), E_MASK, b"mask_arena is NULL"),
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
    (dict(plan="nomask"), E_WORKSPACE, b"without masks"),
    (dict(plan="35"), E_WORKSPACE, b"another operator"), (dict(plan="layer"), E_WORKSPACE, b"another operator"),
    (dict(plan="35", nc=10 | (2 << 16)), E_WORKSPACE, b"another operator"),
    (dict(plan="stamp_126"), E_WORKSPACE, b"no plan"), (dict(plan="shifted_126"), E_WORKSPACE, b"8-byte"),
    (dict(nc=125), E_KNOTS, b"num_coeffs"), (dict(nc=0), E_KNOTS, b"num_coeffs"), (dict(nc=56 | (2 << 16)), E_KNOTS, b"order"),
    (dict(coeffs=_p(2, 4)), E_SHAPE, b"8-byte"), (dict(coeffs=_p(2, 2), nc=35, plan="35"), E_SHAPE, b"4-byte"),
])
def test_trispace_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_trispace_fwd_ragged_fg_u8hwc(*_tri(plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(plan="nomask_layer"), E_WORKSPACE, b"without masks"),
    (dict(plan="126"), E_WORKSPACE, b"another operator"), (dict(plan="35"), E_WORKSPACE, b"another operator"),
    (dict(plan="stamp_layer"), E_WORKSPACE, b"no plan"), (dict(plan="shifted_layer"), E_WORKSPACE, b"8-byte"),
    (dict(rawL=None), E_NULL, b"rawL/rawR/rawH"), (dict(rawR=None), E_NULL, b"rawL/rawR/rawH"), (dict(rawH=None), E_NULL, b"rawL/rawR/rawH"),
    (dict(Kl=1), E_KNOTS, b"knots per curve"), (dict(Kh=16 | (17 << 16)), E_KNOTS, b"last curve"),
    (dict(ws=None), E_WORKSPACE, b"NULL"), (dict(ws=_p(9, 4)), E_WORKSPACE, b"16-byte"), (dict(ws_bytes=8), E_WORKSPACE, b"too small"),
])
def test_layer_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_layer_fwd_ragged_fg_u8hwc(*_layer(lib, plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


# ------------------------------------------------------------------ the Python surface on the host
BATCH = [(1, 1, 3), (3, 5, 3), (4, 8, 4)]


def test_ragged_foreground_ops_on_the_host():
    import torch
    from curl_amd import ops
    imgs = [torch.zeros(h, w, c, dtype=torch.uint8) for h, w, c in BATCH]
    ms = [t[..., 0].contiguous() for t in imgs]
    coeffs = torch.zeros(3, 3, 3, 126)
    knots = [torch.zeros(3, n) for n in (48, 48, 64)]
    for images, masks in ((imgs, ms), (ops.RaggedBytes.pack(imgs), ops.RaggedBytes.pack(ms)), ([t.numpy() for t in imgs], [m.numpy() for m in ms])):
        with pytest.raises(RuntimeError, match="HIP device only"):  # no CPU fallback
            ops.trispace_foreground_u8hwc_ragged(images, coeffs, masks)
        with pytest.raises(RuntimeError, match="HIP device only"):
            ops.curl_layer_foreground_u8hwc_ragged(images, *knots, masks)
    bad_masks = (None,                                            # required
                 ms[:2],                                          # one mask per image
                 [ms[0], ms[1], ms[1]],                           # of the image's size
                 [ms[0], ms[1], imgs[2]],                         # [H,W], not an image
                 [ms[0], ms[1], ms[2].float()],                   # uint8
                 [ms[0], ms[1], ms[2].numpy().astype(np.int16)])
    for bad in bad_masks:
        with pytest.raises(ValueError):
            ops.trispace_foreground_u8hwc_ragged(imgs, coeffs, bad)
        with pytest.raises(ValueError):
            ops.curl_layer_foreground_u8hwc_ragged(imgs, *knots, bad)
    empty_img, empty_mask = torch.zeros(0, 4, 3, dtype=torch.uint8), torch.zeros(0, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.trispace_foreground_u8hwc_ragged(imgs[:2] + [empty_img], coeffs, ms[:2] + [empty_mask])
    with pytest.raises(ValueError):
        ops.curl_layer_foreground_u8hwc_ragged(imgs[:2] + [empty_img], *knots, ms[:2] + [empty_mask])
    out = ops.trispace_foreground_u8hwc_ragged([], coeffs[:0], [])
    assert len(out) == 0 and out.arena.numel() == 0 and out.images() == []
    out, reg = ops.curl_layer_foreground_u8hwc_ragged([], *[k[:0] for k in knots], [])
    assert len(out) == 0 and reg.shape == (0,)
    with pytest.raises(ValueError):
        ops.trispace_foreground_u8hwc_ragged([], coeffs[:0], None)


def test_python_surface_exists():
    from curl_amd import infer, infer_dir, ops
    assert list(inspect.signature(ops.trispace_foreground_u8hwc_ragged).parameters) == ["images", "coeffs", "fg_masks"]
    assert list(inspect.signature(ops.curl_layer_foreground_u8hwc_ragged).parameters) == ["images", "L", "R", "H", "fg_masks"]
    for name in ("trispace_foreground_u8hwc_ragged", "curl_layer_foreground_u8hwc_ragged"):
        assert inspect.signature(getattr(ops, name)).parameters["fg_masks"].default is inspect.Parameter.empty  # required
    plain, fg = inspect.signature(infer.enhance_many).parameters, inspect.signature(infer.enhance_many_foreground).parameters
    assert list(fg) == list(plain) == ["net", "images_u8", "masks_u8", "device", "view", "batch_size"]
    assert all(fg[k].default == plain[k].default and fg[k].kind == plain[k].kind for k in plain)
    assert fg["view"].default == "pil" and fg["batch_size"].default == 32
    src = inspect.getsource(infer.enhance_many_foreground)
    assert "encoder_view_u8hwc_ragged" in src  # the views are the ragged call's here too
    # the argument checks of enhance_many, before anything goes to a device
    for call in (infer.enhance_many, infer.enhance_many_foreground):
        with pytest.raises(ValueError):
            call(None, [np.zeros((8, 8, 3), np.uint8)], [], "cpu")
        with pytest.raises(ValueError):
            call(None, [], [], "cpu", view="nearest")
        with pytest.raises(ValueError):
            call(None, [], [], "cpu", batch_size=0)
        assert call(None, [], [], "cpu") == []


def test_infer_dir_parses_foreground_masks(monkeypatch, tmp_path):
    """--foreground_masks is a store_true flag, off by default, and selects enhance_many_foreground (empty folders: the model
    is stubbed, nothing reaches a device)."""
    from curl_amd import infer_dir
    calls = []
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: None)
    monkeypatch.setattr(infer_dir, "enhance_many", lambda *a, **k: calls.append("plain") or [])
    monkeypatch.setattr(infer_dir, "enhance_many_foreground", lambda *a, **k: calls.append("foreground") or [])
    from PIL import Image
    for d in ("in", "masks"):
        (tmp_path / d).mkdir()
        Image.fromarray(np.zeros((8, 8), np.uint8)).save(tmp_path / d / "a.png")
    base = ["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random", "--out_dir", str(tmp_path / "out")]
    assert infer_dir.main(base) == 0 and calls == ["plain"]
    assert infer_dir.main(base + ["--foreground_masks"]) == 0 and calls == ["plain", "foreground"]
    with pytest.raises(SystemExit):
        infer_dir.main(base + ["--foreground_masks", "yes"])  # a flag, not an option with a value
