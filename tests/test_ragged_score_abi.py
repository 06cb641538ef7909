"""The ragged score entries (include/curl_hip_ragged_score.h) without a device: the header compiles as C99 and C++17, the two
names are declared, exported and bound from _lib.SIGNATURES_RAGGED_SCORE beside the seven unchanged tables; the workspace
query; every single-fault argument list of curl_sse_ragged_u8hwc a return code with its word before any HIP call (fake device
pointers); the host side of ops.sse_u8hwc_ragged / psnr_u8hwc_ragged, infer.enhance_and_score_many and infer_dir --gt_dir;
and tests/ragged_score_ref.py's psnr_ref against the reference's metric.PSNRMetric.compute_mse."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ragged_score_ref import SHAPES as SCORE_SHAPES, psnr_ref, sse_ref

E_NULL, E_SHAPE, E_KNOTS, E_WORKSPACE, E_MASK, E_FLAGS = -1, -2, -3, -4, -5, -6
WS, SSE = "curl_ragged_score_workspace_bytes", "curl_sse_ragged_u8hwc"
NAMES = {WS: 1, SSE: 15}
HEADER_WORDS, DESC_WORDS = 32, 16
TABLES = {"SIGNATURES": "curl_hip.h", "SIGNATURES_GRAD": "curl_hip_grad.h", "SIGNATURES_VIEW": "curl_hip_view.h",
          "SIGNATURES_FG": "curl_hip_fg.h", "SIGNATURES_RAGGED": "curl_hip_ragged.h", "SIGNATURES_VIEW_RAGGED": "curl_hip_view_ragged.h",
          "SIGNATURES_RAGGED_FG": "curl_hip_ragged_fg.h"}


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/{header}").read(), flags=re.S)
    return re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*(curl_\w+)\s*\(([^)]*)\)", src, flags=re.M)


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


def test_exported_declared_and_bound(lib):
    from curl_amd import _lib
    decl = dict(_declared("curl_hip_ragged_score.h"))
    assert set(decl) == set(_lib.SIGNATURES_RAGGED_SCORE) == set(NAMES)
    for name, n in NAMES.items():
        assert len(decl[name].split(",")) == len(_lib.SIGNATURES_RAGGED_SCORE[name][1]) == n, name
        fn = getattr(lib, name)  # exported
        assert fn.restype is _lib.SIGNATURES_RAGGED_SCORE[name][0] and list(fn.argtypes) == _lib.SIGNATURES_RAGGED_SCORE[name][1]
    for table, header in TABLES.items():  # the seven existing tables still equal their headers
        assert set(getattr(_lib, table)) == {n for n, _ in _declared(header)}, table
    assert lib.curl_version() >= 119


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "curl_hip_ragged_score.h"\n'
                   "int main(void) {\n"
                   "  int hw[1] = {8}, c[1] = {3};\n"
                   "  long long buf[(CURL_RAGGED_HEADER_WORDS + CURL_RAGGED_DESC_WORDS) / 2];\n"
                   "  if (curl_ragged_plan(1, hw, hw, c, 1, 0, buf, sizeof buf) != CURL_OK) return 3;\n"
                   "  if (curl_ragged_score_workspace_bytes(buf) != 8) return 2;\n"
                   "  return curl_sse_ragged_u8hwc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, buf, 0, 0, 0, 0) == CURL_E_NULL ? 0 : 1;\n"
                   "}\n")
    subprocess.check_call([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


# ------------------------------------------------------------------ the plans of the argument lists
def _plan(lib, shapes, op, has_mask=1):
    B = len(shapes)
    hs, ws, cs = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(3))
    nbytes = lib.curl_ragged_plan_bytes(B, op)
    assert nbytes == 4 * (HEADER_WORDS + DESC_WORDS * B)
    buf = np.zeros(nbytes // 4 + 2, dtype=np.int32)
    assert buf.ctypes.data % 8 == 0
    assert lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, op, buf.ctypes.data, nbytes) == 0
    return buf


def _p(n, off=0):
    return ctypes.c_void_p((n << 20) + off)


# an RGBA image in the plan: its image arena is larger than its out arena, which is the one a and b are held to
SHAPES = [(8, 8, 4), (5, 7, 3)]


@pytest.fixture(scope="module")
def plans(lib):
    """name -> (host plan words, [img, mask, out] arena sizes); 'zeros': no plan at all; 'stamp': one bit of the stamp wrong;
    'shifted': the plan four bytes off the 8-byte grid."""
    out = {}
    for name, op, m in (("layer", 0, 1), ("nomask", 0, 0), ("126", 126, 1), ("35", 35, 1)):
        p = _plan(lib, SHAPES, op, m)
        out[name] = (p, [int(v) for v in np.ascontiguousarray(p[12:18]).view(np.int64)])
    out["zeros"] = (np.zeros_like(out["layer"][0]), out["layer"][1])
    bad = out["layer"][0].copy()
    bad[0] ^= 1
    out["stamp"] = (bad, out["layer"][1])
    shifted = np.zeros(out["layer"][0].size + 1, dtype=np.int32)
    shifted[1:] = out["layer"][0]
    out["shifted"] = (shifted[1:], out["layer"][1])
    assert shifted[1:].ctypes.data % 8 == 4
    assert out["layer"][1][0] > out["layer"][1][2]
    return out


def test_workspace_bytes(lib, plans):
    for name in ("layer", "nomask"):
        p = plans[name][0]
        assert p[8] > 0 and p[10] > 0  # both classes
        assert lib.curl_ragged_score_workspace_bytes(p.ctypes.data) == 8 * (int(p[8]) + int(p[10]))
    big = _plan(lib, [(h, w, 3) for h, w in SCORE_SHAPES], 0)
    assert lib.curl_ragged_score_workspace_bytes(big.ctypes.data) == 8 * (int(big[8]) + int(big[10])) == 8 * (1 + 1 + 2 + 3 + 22 + 8)
    for name in ("zeros", "stamp", "126", "35"):
        assert lib.curl_ragged_score_workspace_bytes(plans[name][0].ctypes.data) == 0, name
    assert lib.curl_ragged_score_workspace_bytes(None) == 0


def _args(lib, plans, **kw):
    a = dict(a=_p(1), b=_p(2), mask=_p(3), sums=_p(4), ws=_p(6), plan="layer", host="plan", dev=_p(5), plan_bytes=None, flags=0,
             d_a=0, d_b=0, d_mask=0, d_sums=0, d_ws=0)
    a.update(kw)
    p, sizes = plans[a["plan"]]
    host = p.ctypes.data if a["host"] == "plan" else a["host"]
    pb = 4 * (HEADER_WORDS + len(SHAPES) * DESC_WORDS) if a["plan_bytes"] is None else a["plan_bytes"]
    good = plans["layer"][0]
    ws_bytes = 8 * (int(good[8]) + int(good[10]))
    return [a["a"], sizes[2] + a["d_a"], a["b"], sizes[2] + a["d_b"], a["mask"], plans["layer"][1][1] + a["d_mask"], a["sums"],
            16 * len(SHAPES) + a["d_sums"], a["ws"], ws_bytes + a["d_ws"], host, a["dev"], pb, a["flags"], None]


FAULTS = [
    (dict(a=None), E_NULL, b"NULL"), (dict(b=None), E_NULL, b"NULL"), (dict(host=None), E_NULL, b"host_plan"),
    (dict(dev=None), E_NULL, b"plan_dev"),
    (dict(flags=0x1), E_FLAGS, b"flag"), (dict(flags=0x400000), E_FLAGS, b"flag"), (dict(flags=0x80000000), E_FLAGS, b"flag"),
    (dict(plan="zeros"), E_WORKSPACE, b"no plan"), (dict(plan="stamp"), E_WORKSPACE, b"no plan"),
    (dict(plan="shifted"), E_WORKSPACE, b"8-byte"),
    (dict(plan="126"), E_WORKSPACE, b"another operator"), (dict(plan="35"), E_WORKSPACE, b"another operator"),
    (dict(plan="nomask"), E_WORKSPACE, b"without masks"),
    (dict(dev=_p(5, 4)), E_WORKSPACE, b"8-byte"), (dict(plan_bytes=4 * (HEADER_WORDS + 2 * DESC_WORDS) - 1), E_WORKSPACE, b"too small"),
    (dict(d_a=-1), E_WORKSPACE, b"a arena"), (dict(d_b=-1), E_WORKSPACE, b"b arena"), (dict(d_mask=-1), E_WORKSPACE, b"mask arena"),
    (dict(sums=None), E_WORKSPACE, b"sums"), (dict(d_sums=-1), E_WORKSPACE, b"sums"), (dict(sums=_p(4, 4)), E_WORKSPACE, b"sums"),
    (dict(ws=None), E_WORKSPACE, b"workspace"), (dict(d_ws=-1), E_WORKSPACE, b"workspace"), (dict(ws=_p(6, 4)), E_WORKSPACE, b"workspace"),
    (dict(a=_p(1, 1)), E_SHAPE, b"4-byte"), (dict(b=_p(2, 2)), E_SHAPE, b"4-byte"), (dict(mask=_p(3, 1)), E_SHAPE, b"4-byte"),
]


@pytest.mark.parametrize("kw,code,word", FAULTS)
def test_argument_errors_are_codes(lib, plans, kw, code, word):
    assert lib.curl_sse_ragged_u8hwc(*_args(lib, plans, **kw)) == code, (kw, lib.curl_last_error())
    assert word in lib.curl_last_error(), (kw, lib.curl_last_error())


# ------------------------------------------------------------------ the Python surface on the host
BATCH = [(1, 1), (3, 5), (4, 8)]


def test_score_ops_on_the_host():
    import torch
    from curl_amd import ops
    a = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in BATCH]
    b = [torch.ones(h, w, 3, dtype=torch.uint8) for h, w in BATCH]
    ms = [t[..., 0].contiguous() for t in a]
    for call in (ops.sse_u8hwc_ragged, ops.psnr_u8hwc_ragged):
        assert list(inspect.signature(call).parameters) == ["a", "b", "masks"]
        assert inspect.signature(call).parameters["masks"].default is None
        for x, y, m in ((a, b, ms), (a, b, None), (ops.RaggedBytes.pack(a), ops.RaggedBytes.pack(b), ops.RaggedBytes.pack(ms)),
                        ([t.numpy() for t in a], [t.numpy() for t in b], [t.numpy() for t in ms])):
            with pytest.raises(RuntimeError, match="HIP device only"):  # no CPU fallback
                call(x, y, m)
        rgba = [torch.zeros(h, w, 4, dtype=torch.uint8) for h, w in BATCH]
        bad_pairs = ((rgba, b), (a, rgba), (ops.RaggedBytes.pack(rgba), b),   # four channels
                     ([t.float() for t in a], b), (a, [t.numpy().astype(np.int16) for t in b]),  # other dtypes
                     (a, b[:2]), (a, [b[0], b[2], b[1]]), (a[:2], b),         # differing shape lists
                     (ms, ms),                                                # masks are no images
                     (a[:2] + [torch.zeros(0, 4, 3, dtype=torch.uint8)], b[:2] + [torch.zeros(0, 4, 3, dtype=torch.uint8)]))
        for x, y in bad_pairs:
            with pytest.raises(ValueError):
                call(x, y)
        for bad in (ms[:2], [ms[0], ms[2], ms[1]], [ms[0], ms[1], a[2]], [ms[0], ms[1], ms[2].float()], ops.RaggedBytes.pack(a)):
            with pytest.raises(ValueError):
                call(a, b, bad)
    sums = ops.sse_u8hwc_ragged([], [])
    assert sums.shape == (0, 2) and sums.dtype == torch.int64
    assert ops.sse_u8hwc_ragged([], [], []).shape == (0, 2)
    psnr = ops.psnr_u8hwc_ragged([], [], None)
    assert psnr.shape == (0,) and psnr.dtype == torch.float64


def test_enhance_and_score_many_on_the_host():
    from curl_amd import infer
    sig = inspect.signature(infer.enhance_and_score_many).parameters
    assert list(sig) == ["net", "images_u8", "masks_u8", "targets_u8", "device", "view", "batch_size", "foreground"]
    assert sig["view"].default == "pil" and sig["batch_size"].default == 32 and sig["foreground"].default is False
    # the siblings keep their signatures
    for call in (infer.enhance_many, infer.enhance_many_foreground):
        assert list(inspect.signature(call).parameters) == ["net", "images_u8", "masks_u8", "device", "view", "batch_size"]
    imgs = [np.zeros((8, 8, 3), np.uint8), np.zeros((9, 8, 4), np.uint8)]
    masks = [np.zeros(t.shape[:2], np.uint8) for t in imgs]
    with pytest.raises(ValueError, match="target 1"):  # a target of another size, named by its index
        infer.enhance_and_score_many(None, imgs, masks, [np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8)], "cpu")
    with pytest.raises(ValueError, match="target 0"):
        infer.enhance_and_score_many(None, imgs, masks, [np.zeros((8, 8, 3), np.float32), np.zeros((9, 8, 3), np.uint8)], "cpu")
    with pytest.raises(ValueError):
        infer.enhance_and_score_many(None, imgs, masks, imgs[:1], "cpu")  # one target per image
    with pytest.raises(ValueError):
        infer.enhance_and_score_many(None, imgs, masks[:1], imgs, "cpu")  # enhance_many's own checks
    with pytest.raises(ValueError):
        infer.enhance_and_score_many(None, [], [], [], "cpu", view="nearest")
    with pytest.raises(ValueError):
        infer.enhance_and_score_many(None, [], [], [], "cpu", batch_size=0)
    outs, psnr = infer.enhance_and_score_many(None, [], [], [], "cpu")
    assert outs == [] and psnr.shape == (0,) and psnr.dtype == np.float64


def _folders(tmp_path, stems, gt_stems):
    from PIL import Image
    for d in ("in", "masks", "gt"):
        (tmp_path / d).mkdir()
    for s in stems:
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "in" / f"{s}.png")
        Image.fromarray(np.zeros((8, 8), np.uint8)).save(tmp_path / "masks" / f"{s}.png")
    for s in gt_stems:
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "gt" / f"{s}.jpg")  # matched by stem, any extension
    return ["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random", "--out_dir",
            str(tmp_path / "out")]


def test_infer_dir_parses_gt_dir(monkeypatch, tmp_path, capsys):
    """--gt_dir selects enhance_and_score_many (with the foreground flag handed on), prints one line per image and the mean
    over the finite ones, and writes the same lines to --scores_file; without it the two enhance functions are called through
    the module's names as before (the model and the three functions are stubbed: nothing reaches a device)."""
    from curl_amd import infer_dir
    calls = []
    values = {"a": 30.0, "b": float("inf"), "c": float("nan"), "d": 20.5}
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: None)
    monkeypatch.setattr(infer_dir, "enhance_many", lambda net, imgs, *a, **k: calls.append("plain") or [np.zeros((8, 8, 3), np.uint8)] * len(imgs))
    monkeypatch.setattr(infer_dir, "enhance_many_foreground",
                        lambda net, imgs, *a, **k: calls.append("foreground") or [np.zeros((8, 8, 3), np.uint8)] * len(imgs))

    def score(net, imgs, ms, tgts, device, view="pil", batch_size=32, foreground=False):
        assert len(imgs) == len(ms) == len(tgts) and all(t.shape == (8, 8, 3) and t.dtype == np.uint8 for t in tgts)
        calls.append(("score", len(imgs), foreground))
        start = sum(c[1] for c in calls[:-1] if isinstance(c, tuple) and c[0] == "score") % len(values)
        return [np.zeros((8, 8, 3), np.uint8)] * len(imgs), np.array([values[s] for s in sorted(values)][start:start + len(imgs)])
    monkeypatch.setattr(infer_dir, "enhance_and_score_many", score)
    base = _folders(tmp_path, sorted(values), sorted(values))
    assert infer_dir.main(base) == 0 and calls == ["plain"]
    assert infer_dir.main(base + ["--foreground_masks"]) == 0 and calls == ["plain", "foreground"]
    assert capsys.readouterr().out == ""
    del calls[:]
    scores = tmp_path / "scores.txt"
    assert infer_dir.main(base + ["--gt_dir", str(tmp_path / "gt"), "--scores_file", str(scores), "--batch_size", "3"]) == 0
    assert calls == [("score", 3, False), ("score", 1, False)]  # one call per batch
    lines = capsys.readouterr().out.splitlines()
    assert scores.read_text().splitlines() == lines and len(lines) == 5
    assert [ln.split("\t")[0] for ln in lines] == ["a", "b", "c", "d", "mean"]
    assert [float(ln.split("\t")[1]) for ln in lines[:2]] == [30.0, float("inf")] and np.isnan(float(lines[2].split("\t")[1]))
    assert float(lines[3].split("\t")[1]) == 20.5
    mean = lines[4].split("\t")
    assert float(mean[1]) == (30.0 + 20.5) / 2 and int(mean[2]) == 2  # the mean over the finite ones, two left out
    del calls[:]
    assert infer_dir.main(base + ["--gt_dir", str(tmp_path / "gt"), "--foreground_masks"]) == 0
    assert calls == [("score", 4, True)]
    with pytest.raises(SystemExit):
        infer_dir.main(base + ["--scores_file", str(scores)])  # needs --gt_dir
    with pytest.raises(SystemExit):
        infer_dir.main(base + ["--gt_dir"])


def test_infer_dir_gt_dir_with_a_missing_stem(monkeypatch, tmp_path):
    from curl_amd import infer_dir
    built = []
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: built.append(1))
    base = _folders(tmp_path, ["a", "b"], ["a"])
    with pytest.raises(FileNotFoundError, match="b"):
        infer_dir.main(base + ["--gt_dir", str(tmp_path / "gt")])
    assert built == []  # before the model is built


# ------------------------------------------------------------------ psnr_ref against the reference's metric
REFERENCE = os.environ.get("CURL_REFERENCE", "/root/reference")


def _reference_metric():
    path = os.path.join(REFERENCE, "metric.py")
    if not os.path.exists(path):
        pytest.skip("the reference is absent")
    saved = np.get_printoptions()
    spec = importlib.util.spec_from_file_location("_reference_metric", path)
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    except ImportError as e:  # (it imports matplotlib at the top)
        pytest.skip(f"the reference's metric.py does not import here: {e}")
    finally:
        np.set_printoptions(**saved)  # (the module sets numpy's print threshold on import)
    return mod


def test_psnr_ref_is_the_references():
    """psnr_ref of sse_ref's integers against 10 * log10(1 / compute_mse) of the reference on CPU float32 (metric.py:35-64 on
    bytes / 255 with the 0 / 1 mask `mask != 0`): nan and inf in the same places, finite values within 2e-3 dB.  The bound is
    derived, not tuned: a float32 x / 255 carries 2^-24 relative error and the smallest non-zero true difference is 1 / 255,
    so a term's relative error is <= 6e-5; a float32 sum of a few thousand terms adds at most ~1e-4; times 10 / ln 10 that
    is 7e-4 dB."""
    import torch
    metric = _reference_metric()
    rng = np.random.default_rng(1911)
    worst = 0.0
    for kind in ("random", "plus_minus_1", "equal"):
        for mask_kind in ("random", "none", "zero"):
            for h, w in SCORE_SHAPES:
                a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                if kind == "random":
                    b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                elif kind == "equal":
                    b = a.copy()
                else:
                    a = np.clip(a, 1, 254)
                    b = (a.astype(np.int16) + rng.choice([-1, 1], (h, w, 3))).astype(np.uint8)
                mask = {"random": rng.choice(np.array([0, 1, 128, 255], np.uint8), (h, w)), "none": None,
                        "zero": np.zeros((h, w), np.uint8)}[mask_kind]
                got = float(psnr_ref(*sse_ref(a, b, mask)))
                keep = np.ones((h, w), np.float32) if mask is None else (mask != 0).astype(np.float32)
                ta, tb = (torch.from_numpy(x).permute(2, 0, 1)[None].float() / 255.0 for x in (a, b))
                with np.errstate(divide="ignore", invalid="ignore"):
                    mse = metric.PSNRMetric.compute_mse(ta, tb, torch.from_numpy(keep)[None, None]).double().numpy()
                    want = float((10.0 * np.log10(1.0 / mse))[0])
                case = (kind, mask_kind, (h, w), got, want)
                if np.isfinite(want):
                    assert np.isfinite(got) and abs(got - want) <= 2e-3, case
                    worst = max(worst, abs(got - want))
                else:
                    assert (np.isnan(want) and np.isnan(got)) or (np.isinf(want) and got == want), case
    print(f"worst finite difference {worst:.3g} dB")
