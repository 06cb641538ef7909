"""The ragged MS-SSIM entry on the GPU (curl_msssim_ragged_u8hwc, include/curl_hip_ragged_msssim.h) against the oracle in
float64 (tests/ragged_msssim_ref.py: criterion_check.MsssimReference on bytes.float() / 255 times mask > 0), to its own
stats_bound = max(2e-6, 4 r32_stats).

One batch of eight images (ragged_msssim_ref.SHAPES).  Six kinds of content and five kinds of mask, rotated over the images
across the calls: in call (r, q) image j takes content (j + r) mod 6 and, with a mask arena, mask (j + q) mod 4 -- over the
thirty calls every image meets every pair.  The arenas are filled with random bytes before the images go in (a read of
padding or of the neighbouring image changes a halo), the workspace and stats with NaN bits before every call (a read of a
cell nobody wrote shows as a NaN).
  content  r random against random   e equal (every statistic is exactly 1)   n target + noise of +-12
           s a ramp + noise of +-3   x all 0 against all 255                   f flat 100 against 101
  mask     - no mask arena   f all 255   z all 0 (every statistic is exactly 1)   c random over {0, 1, 128, 255}   l left half 0
r, n and s are the evidence (bounds of 2e-6 .. 2.2e-5); x and f have r32 up to 1.7e-4 -- the ill-conditioning of a float32
variance -- and stand for finiteness and for the places of 0 and 1."""
import numpy as np
import pytest
import torch

import guard_arena as GA
from ragged_msssim_ref import CONTENTS, MASKS, SHAPES, TIGHT, float_images, make_data, msssim_formula, reference

pytestmark = pytest.mark.gpu

B = len(SHAPES)
HEADER_WORDS, DESC_WORDS = 32, 64
CALLS = [(r, None) for r in range(6)] + [(r, q) for q in range(4) for r in range(6)]  # (content rotation, mask rotation or None)
NAN64 = -1  # int64 all ones: a NaN as float64 and as two float32


def _id(call):
    return f"c{call[0]}-" + ("nomask" if call[1] is None else f"m{call[1]}")


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


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def data():
    """(pairs, masks, memo of references): host tensors, made once, never changed; a reference is computed once and shared."""
    return (*make_data(), {})


def _rand_u8(g, *shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)


def _kinds(call):
    r, q = call
    return [(CONTENTS[(j + r) % 6], None if q is None else MASKS[(j + q) % 4]) for j in range(B)]


def _ref(data, j, ck, mk, window=11):
    pairs, masks, memo = data
    if (j, ck, mk, window) not in memo:
        a, b = pairs[ck][j]
        memo[j, ck, mk, window] = reference(a, b, None if mk is None else masks[mk][j], window)
    return memo[j, ck, mk, window]


def _noisy(ops, tensors, dev, g):
    """RaggedBytes.pack, but into an arena of random bytes: the padding between the images is not zero."""
    shapes, channels = [tuple(t.shape[:2]) for t in tensors], [t.shape[2] if t.dim() == 3 else 1 for t in tensors]
    offsets, nbytes = ops.RaggedBytes.layout(shapes, channels)
    arena = _rand_u8(g, nbytes)
    for t, o in zip(tensors, offsets):
        arena[o:o + t.numel()] = t.reshape(-1)
    return ops.RaggedBytes(arena.to(dev), shapes, offsets, channels)


def _batch(ops, data, dev, call, order, g):
    """-> (a, b, masks or None) as noisy arenas of the images `order` of the call."""
    pairs, masks, _ = data
    kinds = _kinds(call)
    a = _noisy(ops, [pairs[kinds[j][0]][j][0] for j in order], dev, g)
    b = _noisy(ops, [pairs[kinds[j][0]][j][1] for j in order], dev, g)
    m = None if call[1] is None else _noisy(ops, [masks[kinds[j][1]][j] for j in order], dev, g)
    return a, b, m


_plans = {}


def _plan(lib, shapes, has_mask, dev):
    """(host plan words, their upload, workspace bytes) of a shape list, through the C ABI."""
    key = (tuple(shapes), has_mask)
    if key not in _plans:
        n = len(shapes)
        hs, ws = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(2))
        nbytes = lib.curl_msssim_ragged_plan_bytes(n)
        host = torch.zeros(nbytes // 4, dtype=torch.int32)
        rc = lib.curl_msssim_ragged_plan(n, hs.ctypes.data, ws.ctypes.data, has_mask, host.data_ptr(), nbytes)
        assert rc == 0, lib.curl_last_error()
        _plans[key] = (host, host.to(dev), lib.curl_msssim_ragged_workspace_bytes(host.data_ptr()))
    return _plans[key]


def _entry(lib, a, b, m, window, dev, plan_dev=None, want_ws=False):
    """curl_msssim_ragged_u8hwc through the C ABI with stats and the workspace filled with NaN bits -> stats [n,2,5] float64."""
    host, up, ws_bytes = _plan(lib, a.shapes, int(m is not None), dev)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    stats = torch.full((len(a), 2, 5), NAN64, dtype=torch.int64, device=dev)
    ws = torch.full((ws_bytes // 8,), NAN64, dtype=torch.int64, device=dev)
    pd = up if plan_dev is None else plan_dev
    rc = lib.curl_msssim_ragged_u8hwc(a.arena.data_ptr(), a.arena.numel(), b.arena.data_ptr(), b.arena.numel(),
                                      m.arena.data_ptr() if m is not None else None, m.arena.numel() if m is not None else 0,
                                      stats.data_ptr(), stats.numel() * 8, ws.data_ptr(), ws_bytes, host.data_ptr(), pd.data_ptr(),
                                      pd.numel() * 4, window, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.curl_last_error()
    return (stats.view(torch.float64), ws) if want_ws else stats.view(torch.float64)


def _hold(got, data, call, order, window, label=""):
    """Every statistic finite and within the reference's stats_bound of stats64 -> the largest error / bound over the tight
    contents (printed by the callers: a figure beside the assertion)."""
    kinds = _kinds(call)
    got = got.cpu().numpy()
    assert got.shape == (len(order), 2, 5) and np.isfinite(got).all(), (label, call, got)
    share = 0.0
    for k, j in enumerate(order):
        ref = _ref(data, j, *kinds[j], window)
        want = ref.stats64[:, 0].numpy()
        err = float(np.abs(got[k] - want).max())
        print(f"{label} window {window} {SHAPES[j]} {kinds[j]}: err {err:.3g} bound {ref.stats_bound:.3g}")
        assert err <= ref.stats_bound, (label, call, SHAPES[j], kinds[j], err, ref.stats_bound, got[k], want)
        if kinds[j][0] in TIGHT and kinds[j][1] != "z":
            share = max(share, err / ref.stats_bound)
    return share


def test_the_inputs_reach_what_they_are_for(data):
    """Conditions on the inputs and on the oracle, not on the code under test."""
    seen = {(j, k) for call in CALLS for j, k in enumerate(_kinds(call))}
    assert seen == {(j, (c, m)) for j in range(B) for c in CONTENTS for m in list(MASKS) + [None]}  # every image, every pair
    for j in (0, 1, 5):
        assert bool((_ref(data, j, "e", "c").stats64 == 1).all()) and bool((_ref(data, j, "r", "z").stats64 == 1).all())
        assert _ref(data, j, "r", None).stats_bound <= 2.2e-5 and _ref(data, j, "n", "c").stats_bound <= 2.2e-5  # the tight cases
        assert _ref(data, j, "s", "l").stats_bound <= 2.2e-5
    assert float(_ref(data, 5, "x", None).stats64[0].max()) < 0.1  # 0 against 255: no SSIM to speak of
    for h, w in SHAPES:
        assert min(h, w) >= 32 and min(h, w) >> 4 >= 2


# ------------------------------------------------------------------ 1. the statistics, in any order and on every call
@pytest.mark.parametrize("call", CALLS, ids=_id)
def test_stats_window_11(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(7 + 10 * call[0] + (0 if call[1] is None else call[1] + 1))
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    stats = _entry(lib, a, b, m, 11, dev)
    share = _hold(stats, data, call, everyone, 11, "batch")
    print(f"largest err / bound over the tight contents: {share:.3f}")
    assert torch.equal(_entry(lib, a, b, m, 11, dev), stats)  # a repeated call: the same bits
    ra, rb_, rm = _batch(ops, data, dev, call, everyone[::-1], g)  # the batch reversed (other padding bytes too)
    assert torch.equal(_entry(lib, ra, rb_, rm, 11, dev).flip(0), stats)
    got = ops.msssim_stats_u8hwc_ragged(a, b, m)  # the wrapper: the entry's bits
    assert got.dtype == torch.float64 and got.device == a.device and torch.equal(got, stats)


@pytest.mark.parametrize("call", [(0, None), (1, 0), (2, 1), (3, 2), (4, 3), (5, 0)], ids=_id)
def test_stats_window_3(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(70 + call[0])
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    stats = _entry(lib, a, b, m, 3, dev)
    _hold(stats, data, call, everyone, 3, "batch")
    assert torch.equal(ops.msssim_stats_u8hwc_ragged(a, b, m, window_size=3), stats)
    ra, rb_, rm = _batch(ops, data, dev, call, everyone[::-1], g)
    assert torch.equal(_entry(lib, ra, rb_, rm, 3, dev).flip(0), stats)


def test_stats_window_1_on_two_images(ops, lib, dev, data):
    g = torch.Generator().manual_seed(71)
    for call in ((0, None), (1, 1)):  # image 1: equal | near, image 5: flat | random; the second call with masks c and f
        order = [1, 5]
        a, b, m = _batch(ops, data, dev, call, order, g)
        stats = _entry(lib, a, b, m, 1, dev)
        _hold(stats, data, call, order, 1, "two")
        assert torch.equal(ops.msssim_stats_u8hwc_ragged(a, b, m, window_size=1), stats)


@pytest.mark.parametrize("call", [CALLS[2], CALLS[15]], ids=_id)
def test_an_image_alone_gives_its_batch_bits(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(72)
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    stats = _entry(lib, a, b, m, 11, dev)
    for j in everyone:
        ja, jb, jm = _batch(ops, data, dev, call, [j], g)
        alone = _entry(lib, ja, jb, jm, 11, dev)
        assert alone.shape == (1, 2, 5) and torch.equal(alone[0], stats[j]), (call, SHAPES[j])
    # lists of device tensors and of host arrays give the arenas' bits, on the cached plan of the shape list
    pairs, masks, _ = data
    kinds = _kinds(call)
    la, lb = [pairs[kinds[j][0]][j][0] for j in everyone], [pairs[kinds[j][0]][j][1] for j in everyone]
    lm = None if call[1] is None else [masks[kinds[j][1]][j] for j in everyone]
    assert torch.equal(ops.msssim_stats_u8hwc_ragged(a, b, m), stats)
    n = len(ops._msssim_ragged_plans)
    for x, y, z in (([t.to(dev) for t in la], [t.to(dev) for t in lb], None if lm is None else [t.to(dev) for t in lm]),
                    ([t.to(dev) for t in la], [t.numpy() for t in lb], lm)):
        assert torch.equal(ops.msssim_stats_u8hwc_ragged(x, y, z), stats)
    assert len(ops._msssim_ragged_plans) == n
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.msssim_stats_u8hwc_ragged(ops.RaggedBytes.pack(la, dev), ops.RaggedBytes.pack(lb), None)


# ------------------------------------------------------------------ 2. beside the float entry
@pytest.mark.parametrize("call,window", [(CALLS[1], 11), (CALLS[9], 11), (CALLS[22], 3)], ids=["nomask-11", "masks-11", "masks-3"])
def test_agrees_with_msssim_stats_of_the_float_images(ops, lib, dev, data, call, window):
    """ops.msssim_stats of the same float image (u8hwc_to_f32chw times mask > 0) gives the statistics to the same bound; the two
    need not be bit-equal (float32 means there, another summation order)."""
    g = torch.Generator().manual_seed(73)
    pairs, masks, _ = data
    kinds = _kinds(call)
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    stats = _entry(lib, a, b, m, window, dev).cpu().numpy()
    for j in everyone:
        fa, fb = ops.u8hwc_to_f32chw(a.image(j)[None]), ops.u8hwc_to_f32chw(b.image(j)[None])
        if m is not None:
            keep = (m.image(j) > 0)[None, None].float()
            fa, fb = fa * keep, fb * keep
        want = float_images(pairs[kinds[j][0]][j][0], pairs[kinds[j][0]][j][1], None if m is None else masks[kinds[j][1]][j])
        assert torch.equal(fa.cpu(), want[0]) and torch.equal(fb.cpu(), want[1])  # the float images ARE the reference's
        ssims, mcs = ops.msssim_stats(fa, fb, window)
        theirs = torch.stack((ssims[0], mcs[0])).double().cpu().numpy()
        bound = _ref(data, j, *kinds[j], window).stats_bound
        err = float(np.abs(stats[j] - theirs).max())
        print(f"{SHAPES[j]} {kinds[j]} window {window}: |ragged - float entry| {err:.3g} bound {bound:.3g}")
        assert np.isfinite(theirs).all() and err <= bound, (SHAPES[j], kinds[j], err, bound)


# ------------------------------------------------------------------ 3. a foreign plan writes nothing
def test_a_foreign_plan_writes_nothing(ops, lib, dev, data):
    """The device plan of the same shapes in another order (another hash) beside the host plan of the call: every workgroup of
    all six launches returns at its first comparison; stats and the workspace keep their fill and the entry returns CURL_OK."""
    g = torch.Generator().manual_seed(74)
    a, b, m = _batch(ops, data, dev, CALLS[11], list(range(B)), g)
    host, _, _ = _plan(lib, SHAPES, 1, dev)
    foreign, foreign_dev, _ = _plan(lib, SHAPES[::-1], 1, dev)
    assert host.numel() == foreign.numel() and not torch.equal(host[18:20], foreign[18:20])
    stats, ws = _entry(lib, a, b, m, 11, dev, plan_dev=foreign_dev, want_ws=True)
    assert bool((stats.view(torch.int64) == NAN64).all()) and bool((ws == NAN64).all())
    assert torch.equal(foreign_dev.cpu(), foreign)


# ------------------------------------------------------------------ 4. nothing outside the buffers is touched
@pytest.mark.parametrize("call", [CALLS[3], CALLS[16]], ids=["no_masks", "masks"])
def test_nothing_outside_the_buffers_is_touched(ops, lib, dev, data, call):
    """The entry through the C ABI with every buffer inside one poisoned allocation (tests/guard_arena.py), under both
    poisons: stats is fully assigned and does not depend on the poison, the workspace's guards hold, the three arenas and the
    plan are unchanged -- and the statistics are the references'."""
    g = torch.Generator().manual_seed(75)
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    host, _, ws_bytes = _plan(lib, SHAPES, int(m is not None), dev)
    bufs = [GA.Buf("a", GA.IN, data=a.arena.cpu()), GA.Buf("b", GA.IN, data=b.arena.cpu()), GA.Buf("plan", GA.IN, data=host, grid=16),
            GA.Buf("stats", GA.OUT, shape=(B, 2, 5), dtype=torch.float64), GA.Buf("ws", GA.WORK, nbytes=ws_bytes, grid=16)]
    if m is not None:
        bufs.append(GA.Buf("mask", GA.IN, data=m.arena.cpu()))

    def run(arena):
        rc = lib.curl_msssim_ragged_u8hwc(arena.ptr("a"), arena.nbytes("a"), arena.ptr("b"), arena.nbytes("b"), arena.ptr("mask"),
                                          arena.nbytes("mask"), arena.ptr("stats"), arena.nbytes("stats"), arena.ptr("ws"),
                                          arena.nbytes("ws"), host.data_ptr(), arena.ptr("plan"), arena.nbytes("plan"), 11, 0,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.curl_last_error()
    done = GA.run_both(bufs, "16", dev, run)
    _hold(done.read("stats"), data, call, everyone, 11, "guarded")


# ------------------------------------------------------------------ 5. the MS-SSIM of the statistics
def test_msssim_is_the_formula_and_the_oracles(ops, lib, dev, data):
    """ops.msssim_u8hwc_ragged against metric.py:200-207 in numpy float64 on the entry's own statistics, to 1e-12; and, for the
    contents whose float64 statistics are all >= 0 (random and near: asserted), against the oracle's msssim in float64 to
    2 stats_bound: there |d/dx ((x + 1) / 2)^w| <= w, and the weights sum to 1.4 with the last factor four times."""
    import curl_oracle as O
    g = torch.Generator().manual_seed(76)
    pairs, masks, _ = data
    everyone = list(range(B))
    checked = 0
    for call in (CALLS[0], CALLS[5], CALLS[8], CALLS[20]):
        kinds = _kinds(call)
        a, b, m = _batch(ops, data, dev, call, everyone, g)
        stats = _entry(lib, a, b, m, 11, dev)
        got = ops.msssim_u8hwc_ragged(a, b, m)
        assert got.shape == (B,) and got.dtype == torch.float64 and got.device == a.device
        got = got.cpu().numpy()
        assert np.isfinite(got).all() and np.abs(got - msssim_formula(stats.cpu().numpy())).max() <= 1e-12
        for j in everyone:
            ck, mk = kinds[j]
            if ck not in "rn":
                continue
            ref = _ref(data, j, ck, mk)
            assert float(ref.stats64.min()) >= 0.0, (SHAPES[j], ck, mk)
            fa, fb = float_images(pairs[ck][j][0], pairs[ck][j][1], None if mk is None else masks[mk][j])
            want = float(O.msssim(fa.double(), fb.double())[0])
            print(f"{SHAPES[j]} {ck} {mk}: msssim {got[j]:.9f} oracle {want:.9f} bound {2 * ref.stats_bound:.3g}")
            assert abs(got[j] - want) <= 2 * ref.stats_bound, (SHAPES[j], ck, mk, got[j], want)
            checked += 1
    assert checked >= 8
    assert 0.0448 + 0.2856 + 0.3001 + 0.2363 + 4 * 0.1333 <= 2.0  # 1.4: ten statistics off by a bound each move the value by 1.4 bounds


# ------------------------------------------------------------------ 6. infer.enhance_and_score_many_msssim and the folder CLI
FILES = [(20, 50, 3), (33, 65, 4), (40, 64, 3), (32, 48, 3)]  # the first has no five-level pyramid


def _files():
    g = torch.Generator().manual_seed(98)
    imgs = [_rand_u8(g, h, w, c).numpy() for h, w, c in FILES]
    masks = []
    for h, w, _ in FILES:
        mk = _rand_u8(g, h, w)
        mk[: h // 3] = 0
        mk[-h // 3:] = 255
        masks.append(mk.numpy())
    targets = [np.clip(x[..., :3].astype(np.int16) + torch.randint(-20, 21, x[..., :3].shape, generator=g).numpy(), 0, 255).astype(np.uint8)
               for x in imgs]
    return imgs, masks, targets


def _net(dev):
    """A TriSpaceRegNet whose coefficients are one fixed row for every image: no batched convolution decides an output byte."""
    from curl_amd import model as M
    from test_gpu_ragged_fg import _TinyBackbone
    torch.manual_seed(5)
    net = M.TriSpaceRegNet(polynomial_order=4, spatial=True, is_train=False, backbone=_TinyBackbone(), feature_width=16).to(dev).eval()
    row = (torch.randn(1, 3, 3, 126, generator=torch.Generator().manual_seed(6)) * 0.05).to(dev)
    net.generate_coefficients = lambda img, mask: tuple(row[:, k].expand(img.shape[0], 3, 126).contiguous() for k in range(3))
    return net


def _same_msssim(ops, got, outs, targets, masks, dev):
    """got against ONE ops call on the images of 32 pixels and more, nan for the others."""
    keep = [i for i, o in enumerate(outs) if min(o.shape[:2]) >= 32]
    assert 0 < len(keep) < len(outs)
    want = np.full(len(outs), np.nan)
    want[keep] = ops.msssim_u8hwc_ragged([torch.from_numpy(outs[i]).to(dev) for i in keep],
                                         [torch.from_numpy(np.ascontiguousarray(targets[i][..., :3])).to(dev) for i in keep],
                                         [torch.from_numpy(masks[i]).to(dev) for i in keep]).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[keep], want[keep]) and np.all((got[keep] > 0) & (got[keep] < 1)), (got, want)


def test_enhance_and_score_many_msssim(ops, dev):
    from curl_amd import infer
    imgs, masks, targets = _files()
    net = _net(dev)
    want = infer.enhance_many(net, imgs, masks, dev)
    for foreground, batch_size in ((False, 4), (True, 3), (False, 1)):
        plain, psnr = infer.enhance_and_score_many(net, imgs, masks, targets, dev, batch_size=batch_size, foreground=foreground)
        outs, psnr2, msssim = infer.enhance_and_score_many_msssim(net, imgs, masks, targets, dev, batch_size=batch_size, foreground=foreground)
        assert len(outs) == len(FILES) and np.array_equal(psnr, psnr2)
        for o, p, w in zip(outs, plain, want):
            assert o.dtype == np.uint8 and np.array_equal(o, p) and np.array_equal(o, w)
        assert np.isnan(msssim[0]) and msssim.shape == (len(FILES),)  # 20 x 50: nan, and the batch did not fail
        _same_msssim(ops, msssim, outs, targets, masks, dev)
    _, _, same = infer.enhance_and_score_many_msssim(net, imgs, masks, want, dev)  # every output scored against itself
    assert np.isnan(same[0]) and np.abs(same[1:] - 1).max() <= 1e-5


def test_infer_dir_msssim_scores_the_files_it_writes(ops, dev, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from curl_amd import infer_dir
    imgs, masks, targets = _files()
    for d in ("in", "masks", "gt", "plain", "scored"):
        (tmp_path / d).mkdir()
    names = ["a", "b", "c", "d"]
    for name, img, mask, tgt in zip(names, imgs, masks, targets):
        Image.fromarray(img).save(tmp_path / "in" / f"{name}.png")
        Image.fromarray(mask).save(tmp_path / "masks" / f"{name}.png")
        Image.fromarray(tgt).save(tmp_path / "gt" / f"{name}.png")
    net = _net(dev)
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: net)
    base = ["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random", "--encoder_view", "pil",
            "--batch_size", "3", "--gt_dir", str(tmp_path / "gt")]
    assert infer_dir.main(base + ["--out_dir", str(tmp_path / "plain")]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert infer_dir.main(base + ["--out_dir", str(tmp_path / "scored"), "--msssim"]) == 0
    rows = [ln.split("\t") for ln in capsys.readouterr().out.splitlines()]
    assert [r[0] for r in rows] == names + ["mean"] and [len(r) for r in rows] == [3, 3, 3, 3, 5]
    assert ["\t".join(r[:2]) for r in rows[:4]] == plain[:4]  # the PSNR column is the run's without the flag
    outs = []
    for name in names:
        assert (tmp_path / "plain" / f"{name}.png").read_bytes() == (tmp_path / "scored" / f"{name}.png").read_bytes()
        outs.append(np.asarray(Image.open(tmp_path / "scored" / f"{name}.png")))
    got = np.array([float(r[2]) for r in rows[:4]])
    _same_msssim(ops, got, outs, targets, masks, dev)
    assert abs(float(rows[4][2]) - got[1:].mean()) <= 1e-12 and rows[4][4] == "1"
