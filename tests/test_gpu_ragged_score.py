"""The ragged score entry on the GPU (curl_sse_ragged_u8hwc, include/curl_hip_ragged_score.h): every image's integer sum of
squared differences and pixel count against numpy int64 (tests/ragged_score_ref.py), EXACTLY.

One batch of ten images (ragged_score_ref.SHAPES: both classes, one pixel, one group, idle lanes, a second and a ragged third
workgroup, tiles crossing rows, and 22 200 pixels).  Four kinds of content and five kinds of mask, rotated over the images
across the calls: in call r image j takes content (j + r) mod 4 and, in the sixteen calls with a mask arena, mask
(j + r div 4) mod 4 -- every image meets every pair.  The arenas are filled with random bytes before the images are copied in:
a read of padding changes a sum.
  content  r  random against random          e  equal
           x  all 0 against all 255           t  equal but the first pixel's R and the last pixel's B, which differ by 1
  mask     -  no mask arena (four calls)      f  all 255      z  all 0 (N = 0)
           c  random over {0, 1, 128, 255}    l  all 0 but the last pixel"""
import numpy as np
import pytest
import torch

import guard_arena as GA
from ragged_score_ref import SHAPES, psnr_ref, sse_ref

pytestmark = pytest.mark.gpu

B = len(SHAPES)
CONTENTS, MASKS = "rext", "fzcl"
HEADER_WORDS, DESC_WORDS = 32, 16
CALLS = [(r, None) for r in range(4)] + [(r, r // 4) for r in range(16)]  # (content rotation, mask rotation or None)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from curl_amd import ops as _ops
    from curl_amd import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return _ops


def _rand_u8(g, *shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)


@pytest.fixture(scope="module")
def data():
    """content kind -> the ten (a, b) pairs; mask kind -> the ten masks; and the memo of references.  Host tensors, made once,
    never changed."""
    g = torch.Generator().manual_seed(1911)
    pairs, masks = {k: [] for k in CONTENTS}, {k: [] for k in MASKS}
    for h, w in SHAPES:
        a = _rand_u8(g, h, w, 3)
        pairs["r"].append((a, _rand_u8(g, h, w, 3)))
        pairs["e"].append((a, a.clone()))
        pairs["x"].append((torch.zeros(h, w, 3, dtype=torch.uint8), torch.full((h, w, 3), 255, dtype=torch.uint8)))
        t = a.clamp(1, 254)
        u = t.clone()
        u[0, 0, 0] += 1
        u[-1, -1, 2] -= 1
        pairs["t"].append((t, u))
        last = torch.zeros(h, w, dtype=torch.uint8)
        last[-1, -1] = 7
        masks["f"].append(torch.full((h, w), 255, dtype=torch.uint8))
        masks["z"].append(torch.zeros(h, w, dtype=torch.uint8))
        masks["c"].append(torch.tensor([0, 1, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (h, w), generator=g)])
        masks["l"].append(last)
    return pairs, masks, {}


def _kinds(call):
    r, mr = call
    return [(CONTENTS[(j + r) % 4], None if mr is None else MASKS[(j + mr) % 4]) for j in range(B)]


def _ref(data, j, ck, mk):
    pairs, masks, memo = data
    if (j, ck, mk) not in memo:
        a, b = pairs[ck][j]
        memo[j, ck, mk] = sse_ref(a.numpy(), b.numpy(), None if mk is None else masks[mk][j].numpy())
    return memo[j, ck, mk]


def _noisy(ops, tensors, dev, g):
    """RaggedBytes.pack, but into an arena of random bytes: the padding between the images is not zero."""
    shapes, channels = [tuple(t.shape[:2]) for t in tensors], [t.shape[2] if t.dim() == 3 else 1 for t in tensors]
    offsets, nbytes = ops.RaggedBytes.layout(shapes, channels)
    arena = _rand_u8(g, nbytes)
    for t, o in zip(tensors, offsets):
        arena[o:o + t.numel()] = t.reshape(-1)
    return ops.RaggedBytes(arena.to(dev), shapes, offsets, channels)


def _batch(ops, data, dev, call, order, g):
    """-> (a, b, masks or None) as noisy arenas of the images `order` of the call, and their references [(sse, n)]."""
    pairs, masks, _ = data
    kinds = _kinds(call)
    a = _noisy(ops, [pairs[kinds[j][0]][j][0] for j in order], dev, g)
    b = _noisy(ops, [pairs[kinds[j][0]][j][1] for j in order], dev, g)
    m = None if call[1] is None else _noisy(ops, [masks[kinds[j][1]][j] for j in order], dev, g)
    return a, b, m, [_ref(data, j, *kinds[j]) for j in order]


def test_the_inputs_reach_what_they_are_for(data):
    """Conditions on the inputs, not on the code under test."""
    j = SHAPES.index((150, 148))
    assert _ref(data, j, "x", None) == (4330665000, 22200) and 4330665000 > 2 ** 32  # a 32-bit per-image sum is caught
    assert _ref(data, j, "x", "f") == (4330665000, 22200)
    for j in range(B):
        assert _ref(data, j, "t", None) == (2, SHAPES[j][0] * SHAPES[j][1])
        assert _ref(data, j, "e", "c")[0] == 0 and _ref(data, j, "r", "z") == (0, 0)
        assert _ref(data, j, "t", "l") == (2 if SHAPES[j] == (1, 1) else 1, 1)
    seen = {(j, k) for call in CALLS for j, k in enumerate(_kinds(call))}
    assert seen == {(j, (c, m)) for j in range(B) for c in CONTENTS for m in list(MASKS) + [None]}  # every image, every pair


# ------------------------------------------------------------------ 1. the sums are the integers, in any order and company
def test_sums_are_exact(ops, dev, data):
    g = torch.Generator().manual_seed(7)
    everyone = list(range(B))
    for call in CALLS:
        a, b, m, want = _batch(ops, data, dev, call, everyone, g)
        sums = ops.sse_u8hwc_ragged(a, b, m)
        assert sums.shape == (B, 2) and sums.dtype == torch.int64 and sums.device == a.device
        got = [tuple(int(v) for v in row) for row in sums.cpu()]
        assert got == want, (call, [(SHAPES[j], _kinds(call)[j], got[j], want[j]) for j in everyone if got[j] != want[j]])
        assert torch.equal(ops.sse_u8hwc_ragged(a, b, m), sums)  # a repeated call
        ra, rb_, rm, rwant = _batch(ops, data, dev, call, everyone[::-1], g)  # the batch reversed (other padding bytes too)
        back = [tuple(int(v) for v in row) for row in ops.sse_u8hwc_ragged(ra, rb_, rm).cpu()]
        assert back == rwant == want[::-1], call
    for call in (CALLS[1], CALLS[6]):  # an image alone gives its batch value
        for j in everyone:
            a, b, m, want = _batch(ops, data, dev, call, [j], g)
            alone = ops.sse_u8hwc_ragged(a, b, m)
            assert alone.shape == (1, 2) and tuple(int(v) for v in alone[0].cpu()) == want[0], (call, SHAPES[j])
    # lists of device tensors and of host arrays give the arenas' values
    pairs, masks, _ = data
    kinds = _kinds(CALLS[9])
    la, lb = [pairs[kinds[j][0]][j][0] for j in everyone], [pairs[kinds[j][0]][j][1] for j in everyone]
    lm = [masks[kinds[j][1]][j] for j in everyone]
    want = [_ref(data, j, *kinds[j]) for j in everyone]
    n = len(ops._ragged_plans)
    for x, y, z in (([t.to(dev) for t in la], [t.to(dev) for t in lb], [t.to(dev) for t in lm]),
                    ([t.to(dev) for t in la], [t.numpy() for t in lb], lm)):
        assert [tuple(int(v) for v in row) for row in ops.sse_u8hwc_ragged(x, y, z).cpu()] == want
    assert len(ops._ragged_plans) == n  # the cached plan of the shape list
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.sse_u8hwc_ragged(ops.RaggedBytes.pack(la, dev), ops.RaggedBytes.pack(lb), None)


# ------------------------------------------------------------------ 2. the PSNR of the integers
def test_psnr_is_psnr_ref(ops, dev, data):
    g = torch.Generator().manual_seed(8)
    finite = nans = infs = 0
    for call in CALLS:
        a, b, m, want = _batch(ops, data, dev, call, list(range(B)), g)
        got = ops.psnr_u8hwc_ragged(a, b, m)
        assert got.shape == (B,) and got.dtype == torch.float64 and got.device == a.device
        got = got.cpu().numpy()
        ref = psnr_ref([s for s, _ in want], [n for _, n in want])
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)), (call, got, ref)
        ok = np.isfinite(ref)
        assert not np.isneginf(got).any() and np.all(np.abs(got[ok] - ref[ok]) <= 1e-9), (call, got, ref)
        finite, nans, infs = finite + int(ok.sum()), nans + int(np.isnan(ref).sum()), infs + int(np.isposinf(ref).sum())
    assert finite and nans and infs


# ------------------------------------------------------------------ 3. nothing outside the buffers is touched
def _plan_words(lib, shapes, has_mask):
    n = len(shapes)
    hs, ws = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(2))
    cs = np.full(n, 3, dtype=np.int32)
    nbytes = lib.curl_ragged_plan_bytes(n, 0)
    host = torch.zeros(nbytes // 4, dtype=torch.int32)
    rc = lib.curl_ragged_plan(n, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, 0, host.data_ptr(), nbytes)
    assert rc == 0, lib.curl_last_error()
    return host


@pytest.mark.parametrize("call", [CALLS[2], CALLS[11]], ids=["no_masks", "masks"])
def test_nothing_outside_the_buffers_is_touched(ops, dev, data, call):
    """The entry through the C ABI with every buffer inside one poisoned allocation (tests/guard_arena.py), under both
    poisons: sums is fully assigned and does not depend on the poison, the workspace's guards hold, the three arenas and the
    plan are unchanged -- and the sums are the references."""
    from curl_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(9)
    a, b, m, want = _batch(ops, data, dev, call, list(range(B)), g)
    host = _plan_words(lib, SHAPES, int(m is not None))
    ws_bytes = lib.curl_ragged_score_workspace_bytes(host.data_ptr())
    assert ws_bytes == 8 * (int(host[8]) + int(host[10])) > 0
    bufs = [GA.Buf("a", GA.IN, data=a.arena.cpu()), GA.Buf("b", GA.IN, data=b.arena.cpu()), GA.Buf("plan", GA.IN, data=host, grid=16),
            GA.Buf("sums", GA.OUT, shape=(B, 2), dtype=torch.int64), GA.Buf("ws", GA.WORK, nbytes=ws_bytes, grid=16)]
    if m is not None:
        bufs.append(GA.Buf("mask", GA.IN, data=m.arena.cpu()))

    def run(arena):
        rc = lib.curl_sse_ragged_u8hwc(arena.ptr("a"), arena.nbytes("a"), arena.ptr("b"), arena.nbytes("b"), arena.ptr("mask"),
                                       arena.nbytes("mask"), arena.ptr("sums"), arena.nbytes("sums"), arena.ptr("ws"), arena.nbytes("ws"),
                                       host.data_ptr(), arena.ptr("plan"), arena.nbytes("plan"), 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.curl_last_error()
    done = GA.run_both(bufs, "16", dev, run)
    assert [tuple(int(v) for v in row) for row in done.read("sums").cpu()] == want


# ------------------------------------------------------------------ 4. a foreign plan writes nothing
def test_a_foreign_plan_writes_nothing(ops, dev, data):
    """The device plan of the same shapes in another order (another hash) beside the host plan of the call: every workgroup of
    all three launches returns at its first comparison; sums and the workspace keep their fill and the entry returns CURL_OK."""
    from curl_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(10)
    a, b, m, _ = _batch(ops, data, dev, CALLS[11], list(range(B)), g)
    host, foreign = _plan_words(lib, SHAPES, 1), _plan_words(lib, SHAPES[::-1], 1)
    assert host.numel() == foreign.numel() and not torch.equal(host[18:20], foreign[18:20])
    ws_bytes = lib.curl_ragged_score_workspace_bytes(host.data_ptr())
    sums = torch.full((B, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    ws = torch.full((ws_bytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    plan_dev = foreign.to(dev)
    rc = lib.curl_sse_ragged_u8hwc(a.arena.data_ptr(), a.arena.numel(), b.arena.data_ptr(), b.arena.numel(), m.arena.data_ptr(),
                                   m.arena.numel(), sums.data_ptr(), sums.numel() * 8, ws.data_ptr(), ws_bytes, host.data_ptr(),
                                   plan_dev.data_ptr(), plan_dev.numel() * 4, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.curl_last_error()
    assert bool((sums == 0x5A5A5A5A5A5A5A5A).all()) and bool((ws == 0x5A5A5A5A5A5A5A5A).all())
    assert torch.equal(plan_dev.cpu(), foreign)


# ------------------------------------------------------------------ 5. infer.enhance_and_score_many and the folder CLI
def _targets(files):
    g = torch.Generator().manual_seed(31)
    tg = [_rand_u8(g, h, w, 3).numpy() for h, w, _ in files]
    tg[0] = np.concatenate([tg[0], _rand_u8(g, *files[0][:2], 1).numpy()], axis=2)  # an RGBA target: alpha is dropped
    return tg


def _same_scores(got, outs, targets, masks):
    ref = psnr_ref(*zip(*[sse_ref(o, t[..., :3], m) for o, t, m in zip(outs, targets, masks)]))
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    ok = np.isfinite(ref)
    assert ok.any() and np.all(np.abs(got[ok] - ref[ok]) <= 1e-9), (got, ref)


@pytest.mark.parametrize("arch", ["trispace", "curl"])
def test_enhance_and_score_many(dev, arch):
    """The outputs are enhance_many's (foreground=True: enhance_many_foreground's) byte for byte, the PSNRs are psnr_ref of
    those outputs and the targets under the white masks."""
    from curl_amd import infer
    from test_gpu_ragged_fg import FILES, _files, _net  # three small images and a net whose encoder is given per image
    imgs, masks = _files()
    targets = _targets(FILES)
    net = _net(arch, dev)
    for foreground, batch_size in ((False, 3), (True, 2)):
        want = (infer.enhance_many_foreground if foreground else infer.enhance_many)(net, imgs, masks, dev, batch_size=batch_size)
        outs, psnr = infer.enhance_and_score_many(net, imgs, masks, targets, dev, batch_size=batch_size, foreground=foreground)
        assert len(outs) == len(want) == len(FILES)
        for o, w in zip(outs, want):
            assert o.dtype == np.uint8 and o.shape == w.shape and np.array_equal(o, w), (foreground, o.shape)
        _same_scores(psnr, outs, targets, masks)
    _, psnr = infer.enhance_and_score_many(net, imgs, masks, want, dev)  # every output scored against itself
    assert np.isposinf(psnr).all()
    with pytest.raises(ValueError, match="target 2"):
        infer.enhance_and_score_many(net, imgs, masks, targets[:2] + [targets[2][:-1]], dev)


def test_infer_dir_gt_dir_scores_the_files_it_writes(dev, tmp_path, monkeypatch, capsys):
    """python -m curl_amd.infer_dir --gt_dir on a folder of three PNGs writes the files of the run without it and prints the
    PSNR of every written file against its target, then the mean."""
    from PIL import Image
    from curl_amd import infer_dir
    from test_gpu_ragged_fg import FILES, _files, _net
    imgs, masks = _files()
    targets = [t[..., :3] for t in _targets(FILES)]
    for d in ("in", "masks", "gt", "plain", "scored"):
        (tmp_path / d).mkdir()
    names = ["a", "b", "c"]
    for name, img, mask, tgt in zip(names, imgs, masks, targets):
        Image.fromarray(img[..., 0] if name == "c" else img).save(tmp_path / "in" / f"{name}.png")  # c: an 'L' file
        Image.fromarray(mask).save(tmp_path / "masks" / f"{name}.png")
        Image.fromarray(tgt).save(tmp_path / "gt" / f"{name}.png")
    net = _net("trispace", dev)
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: net)
    base = ["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random", "--encoder_view", "pil",
            "--batch_size", "2"]
    assert infer_dir.main(base + ["--out_dir", str(tmp_path / "plain")]) == 0
    assert capsys.readouterr().out == ""
    scores = tmp_path / "scores.tsv"
    assert infer_dir.main(base + ["--out_dir", str(tmp_path / "scored"), "--gt_dir", str(tmp_path / "gt"), "--scores_file", str(scores)]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert scores.read_text().splitlines() == lines and [ln.split("\t")[0] for ln in lines] == names + ["mean"]
    outs = []
    for name in names:
        assert (tmp_path / "plain" / f"{name}.png").read_bytes() == (tmp_path / "scored" / f"{name}.png").read_bytes()
        outs.append(np.asarray(Image.open(tmp_path / "scored" / f"{name}.png")))
    got = np.array([float(ln.split("\t")[1]) for ln in lines[:3]])
    _same_scores(got, outs, targets, masks)
    assert np.isfinite(got).all() and abs(float(lines[3].split("\t")[1]) - got.mean()) <= 1e-9 and lines[3].split("\t")[2] == "0"
