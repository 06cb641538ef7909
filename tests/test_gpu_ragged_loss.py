"""The ragged CURLLoss entry on the GPU (curl_loss_ragged_u8hwc, include/curl_hip_ragged_loss.h) against the oracle in float64
(tests/ragged_loss_ref.py: curl_loss_terms / msssim / curl_loss on bytes.float() / 255 with the bool mask, one image at a time)
and against float-path code that existed before this entry (ops.loss_term_sums + model._loss_terms: the cosine's own deviation,
and the float32 L planes test_gpu_parity pins to the oracle at 1e-6).  The entry under test is never its own yardstick.

Inputs and their rotation are tests/test_gpu_ragged_msssim.py's: one batch of eight images (ragged_msssim_ref.SHAPES), six
contents and five masks rotated over thirty calls so that every image meets every pair; arenas padded with random bytes; stats
and the workspace filled with NaN bits before every call.

Bounds.  N: exact.  rgb, lab, hsv: S / (3 N) within 3e-6 of the oracle (the project's figure for loss_terms on the float path,
test_gpu_parity).  cosine: max(3e-6, 2 d), d the float entry's own deviation from the oracle on that image (two float32
summation orders are compared).  L statistics: criterion_check.MsssimReference(Lp, Lt).stats_bound = max(2e-6, 4 r32), r32 from
the oracle alone; for the tight contents that bound is asserted to stay <= 2.2e-5, the MS-SSIM test's cap.  The tight set was
meant to be random, near and smooth under every window.  On the one-channel L planes two of those bounds exceed the cap (worked
out from the oracle's float32 planes, before any kernel ran): smooth under window 11 (3.2e-5 on the 40 x 160 image: the ramp's
L is nearly flat inside a window, and a float32 variance of a flat patch is ill-conditioned) and random under window 3 (5.7e-5
on the 70 x 97 image); on the float entry's planes on the device near under window 11 does too (2.35e-5 on the 97 x 129 image
under the all-255 mask).  So smooth and near are in the loose set under window 11 and random under window 3 (TIGHT below);
nothing is widened: every content under every window is still held to its own stats_bound.  The loss of the random and near
contents: (3 * 3e-6 + bound_cos) / 5 + 4 stats_bound -- the MS-SSIM value moves by at most 2 stats_bound
(test_gpu_ragged_msssim's argument) and enters with weight 10 / 5.

Measured on an MI355X: all 81 tests pass; the largest L-statistics error is 0.035 of its bound (7.0e-8 at level 3, random
content under window 3), the largest cosine error 6.0e-8, the largest loss error 0.001 of its bound.  (With the MS-SSIM
kernels' float32 window passes and ssim_window's weights the L statistics missed this bound in 14 of the 36 level cases, by
up to 8.3e-6 on random content and 1.6e-5 on flat planes: the entry's passes are float64 with the reference's own window for
that reason, curl_amd/csrc/kernels/loss_ragged.inc.)"""
import numpy as np
import pytest
import torch

import guard_arena as GA
from ragged_loss_ref import LossReference, float_pair, loss_formula
from ragged_msssim_ref import SHAPES
from test_gpu_ragged_msssim import CALLS, NAN64, _batch, _files, _id, _kinds, _net

pytestmark = pytest.mark.gpu

B = len(SHAPES)
TERM_BOUND, TIGHT_CAP = 3e-6, 2.2e-5
TIGHT = {11: "r", 3: "ns", 1: "rns"}  # window -> the contents whose stats_bound is asserted to stay under the cap (docstring)


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
    from ragged_msssim_ref import make_data
    return (*make_data(), {})


class _Ref:
    """One image's yardsticks: .oracle (LossReference, float64), .cos32 (the float entry's cosine term), .d (its deviation from
    the oracle's), .bound_cos, and .level(window) -> MsssimReference on the float entry's float32 L planes."""

    def __init__(self, ops, dev, a, b, mask):
        from curl_amd import model as M
        self.oracle = LossReference(a, b, mask)
        pred, target, keep = float_pair(a, b, mask)
        sums, Lp, Lt = ops.loss_term_sums(pred.to(dev), target.to(dev), keep.to(dev), want_L=True)
        self.cos32 = float(M._loss_terms(sums, keep.to(dev), pred.shape)[1])
        self.d = abs(self.cos32 - self.oracle.terms[1])
        self.bound_cos = max(TERM_BOUND, 2.0 * self.d)
        self.Lp, self.Lt = Lp.cpu(), Lt.cpu()
        # the planes ARE the oracle's to test_gpu_parity's 1e-6 (a condition on the yardstick)
        assert float((self.Lp.double() - self.oracle.Lp).abs().max()) <= 1e-6 and float((self.Lt.double() - self.oracle.Lt).abs().max()) <= 1e-6
        self._levels = {}

    def level(self, window):
        import criterion_check as CC
        if window not in self._levels:
            self._levels[window] = CC.MsssimReference(self.Lp, self.Lt, window)
        return self._levels[window]


def _ref(ops, dev, data, j, ck, mk):
    pairs, masks, memo = data
    if (j, ck, mk) not in memo:
        a, b = pairs[ck][j]
        memo[j, ck, mk] = _Ref(ops, dev, a, b, None if mk is None else masks[mk][j])
    return memo[j, ck, mk]


_plans = {}


def _plan(lib, shapes, has_mask, dev):
    """(host plan words, their upload, workspace bytes) of a shape list, through the C ABI."""
    key = (tuple(shapes), has_mask)
    if key not in _plans:
        n = len(shapes)
        hs, ws = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(2))
        nbytes = lib.curl_loss_ragged_plan_bytes(n)
        host = torch.zeros(nbytes // 4, dtype=torch.int32)
        rc = lib.curl_loss_ragged_plan(n, hs.ctypes.data, ws.ctypes.data, has_mask, host.data_ptr(), nbytes)
        assert rc == 0, lib.curl_last_error()
        _plans[key] = (host, host.to(dev), lib.curl_loss_ragged_workspace_bytes(host.data_ptr()))
    return _plans[key]


def _entry(lib, a, b, m, window, dev, plan_dev=None, want_ws=False):
    """curl_loss_ragged_u8hwc through the C ABI with stats and the workspace filled with NaN bits -> stats [n,3,5] float64."""
    host, up, ws_bytes = _plan(lib, a.shapes, int(m is not None), dev)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    stats = torch.full((len(a), 3, 5), NAN64, dtype=torch.int64, device=dev)
    ws = torch.full((ws_bytes // 8,), NAN64, dtype=torch.int64, device=dev)
    pd = up if plan_dev is None else plan_dev
    rc = lib.curl_loss_ragged_u8hwc(a.arena.data_ptr(), a.arena.numel(), b.arena.data_ptr(), b.arena.numel(),
                                    m.arena.data_ptr() if m is not None else None, m.arena.numel() if m is not None else 0,
                                    stats.data_ptr(), stats.numel() * 8, ws.data_ptr(), ws_bytes, host.data_ptr(), pd.data_ptr(),
                                    pd.numel() * 4, window, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.curl_last_error()
    return (stats.view(torch.float64), ws) if want_ws else stats.view(torch.float64)


def _hold(ops, dev, got, data, call, order, label=""):
    """Row 0 (items 1-3): every figure of the statistics finite; N exact; the three L1 terms and the cosine within their bounds
    -> the largest cosine error / d, printed by the callers beside the assertions."""
    kinds = _kinds(call)
    got = got.cpu().numpy()
    assert got.shape == (len(order), 3, 5) and np.isfinite(got).all(), (label, call, got)
    cos_ratio = 0.0
    for k, j in enumerate(order):
        ck, mk = kinds[j]
        ref = _ref(ops, dev, data, j, ck, mk)
        o, (h, w), what = ref.oracle, SHAPES[j], (label, call, SHAPES[j], kinds[j])
        row = got[k, 0]
        assert row[4] == o.n, what  # 1. the count, exactly
        if o.n == 0:
            assert (row[:4] == 0).all(), what  # nothing under an all-zero mask: exact zeros
        else:
            for t in (0, 2, 3):  # 2. rgb, lab, hsv
                err = abs(row[t] / (3.0 * o.n) - o.terms[t])
                assert err <= TERM_BOUND, (*what, t, err)
        if ck == "e":
            assert row[0] == 0 and row[2] == 0 and row[3] == 0, what  # equal images: exact zeros
        cosine = 1.0 - (row[1] + (h * w - o.n)) / (h * w)  # 3. the cosine
        err = abs(cosine - o.terms[1])
        print(f"{label} {SHAPES[j]} {kinds[j]}: cosine err {err:.3g} d {ref.d:.3g} bound {ref.bound_cos:.3g}")
        assert err <= ref.bound_cos, (*what, err, ref.d)
        if ref.d > 0:
            cos_ratio = max(cos_ratio, err / ref.d)
    return cos_ratio


def _hold_levels(ops, dev, got, data, call, order, window, label=""):
    """Rows 1, 2 (item 4): every L statistic within the reference's stats_bound of its float64 value.  Every image is looked
    at and every figure printed before the one assertion, so that a run shows all of a call's misses at once -> the largest
    error / bound over the tight contents."""
    kinds = _kinds(call)
    got = got.cpu().numpy()
    share, missed = 0.0, []
    for k, j in enumerate(order):
        ck, mk = kinds[j]
        lv = _ref(ops, dev, data, j, ck, mk).level(window)
        errs = np.abs(got[k, 1:] - lv.stats64[:, 0].numpy()).max(0)  # per level
        err = float(errs.max())
        print(f"{label} window {window} {SHAPES[j]} {kinds[j]}: L stats err {err:.3g} (level {int(errs.argmax())}) bound {lv.stats_bound:.3g}")
        if not err <= lv.stats_bound:
            missed.append((SHAPES[j], kinds[j], f"err {err:.3g} at level {int(errs.argmax())}", f"bound {lv.stats_bound:.3g}"))
        if ck in TIGHT[window] and mk != "z":
            assert lv.stats_bound <= TIGHT_CAP, (label, call, SHAPES[j], kinds[j], lv.stats_bound)  # a condition on the inputs
            share = max(share, err / lv.stats_bound)
    assert not missed, (label, call, window, missed)
    return share


# ------------------------------------------------------------------ 1-3. count and terms, in any order and on every call
@pytest.mark.parametrize("call", CALLS, ids=_id)
def test_stats_window_11(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(7 + 10 * call[0] + (0 if call[1] is None else call[1] + 1))
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    stats = _entry(lib, a, b, m, 11, dev)
    cos_ratio = _hold(ops, dev, stats, data, call, everyone, "batch")
    print(f"largest cosine err / d: {cos_ratio:.3f}")
    assert torch.equal(_entry(lib, a, b, m, 11, dev), stats)  # a repeated call: the same bits
    ra, rb_, rm = _batch(ops, data, dev, call, everyone[::-1], g)  # the batch reversed (other padding bytes too)
    assert torch.equal(_entry(lib, ra, rb_, rm, 11, dev).flip(0), stats)
    got = ops.loss_stats_u8hwc_ragged(a, b, m)  # the wrapper: the entry's bits
    assert got.dtype == torch.float64 and got.device == a.device and torch.equal(got, stats)


@pytest.mark.parametrize("call", [(0, None), (1, 0), (2, 1), (3, 2), (4, 3), (5, 0)], ids=_id)
def test_stats_window_3(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(70 + call[0])
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    stats = _entry(lib, a, b, m, 3, dev)
    _hold(ops, dev, stats, data, call, everyone, "batch")
    assert torch.equal(ops.loss_stats_u8hwc_ragged(a, b, m, window_size=3), stats)
    assert torch.equal(stats[:, 0], _entry(lib, a, b, m, 11, dev)[:, 0])  # the terms do not know the window
    ra, rb_, rm = _batch(ops, data, dev, call, everyone[::-1], g)
    assert torch.equal(_entry(lib, ra, rb_, rm, 3, dev).flip(0), stats)


def test_stats_window_1_on_two_images(ops, lib, dev, data):
    g = torch.Generator().manual_seed(71)
    for call in ((0, None), (1, 1)):  # image 1: equal | near, image 5: flat | random; the second call with masks c and f
        order = [1, 5]
        a, b, m = _batch(ops, data, dev, call, order, g)
        stats = _entry(lib, a, b, m, 1, dev)
        _hold(ops, dev, stats, data, call, order, "two")
        _hold_levels(ops, dev, stats, data, call, order, 1, "two")
        assert torch.equal(ops.loss_stats_u8hwc_ragged(a, b, m, window_size=1), stats)


# ------------------------------------------------------------------ 4. the L statistics (the same calls and arenas as above)
@pytest.mark.parametrize("call", CALLS, ids=_id)
def test_level_stats_window_11(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(7 + 10 * call[0] + (0 if call[1] is None else call[1] + 1))
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    share = _hold_levels(ops, dev, _entry(lib, a, b, m, 11, dev), data, call, everyone, 11, "batch")
    print(f"largest L stats err / bound over the tight contents: {share:.3f}")


@pytest.mark.parametrize("call", [(0, None), (1, 0), (2, 1), (3, 2), (4, 3), (5, 0)], ids=_id)
def test_level_stats_window_3(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(70 + call[0])
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    _hold_levels(ops, dev, _entry(lib, a, b, m, 3, dev), data, call, everyone, 3, "batch")


# ------------------------------------------------------------------ 5. the loss
def test_the_loss_is_the_formula_and_the_oracles(ops, lib, dev, data):
    """ops.curl_loss_u8hwc_ragged against model.py:89-116 in numpy float64 on the entry's own statistics, to 1e-12; and, for the
    contents whose float64 L statistics are all >= 0 (random and near: asserted), against the oracle's loss in float64 (its
    terms plus its one-channel msssim of its L planes) to (3 * 3e-6 + bound_cos) / 5 + 4 stats_bound.  An all-zero mask gives nan."""
    g = torch.Generator().manual_seed(76)
    everyone = list(range(B))
    checked = zero_masks = 0
    for call in (CALLS[0], CALLS[5], CALLS[8], CALLS[20]):
        kinds = _kinds(call)
        a, b, m = _batch(ops, data, dev, call, everyone, g)
        stats = _entry(lib, a, b, m, 11, dev)
        got = ops.curl_loss_u8hwc_ragged(a, b, m)
        assert got.shape == (B,) and got.dtype == torch.float64 and got.device == a.device
        got, want = got.cpu().numpy(), loss_formula(stats.cpu().numpy(), SHAPES)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.abs(got - want)[np.isfinite(want)].max() <= 1e-12
        composed = ops.curl_loss_from_stats(ops.loss_stats_u8hwc_ragged(a, b, m), SHAPES).cpu().numpy()
        assert np.array_equal(composed, got, equal_nan=True)
        for j in everyone:
            ck, mk = kinds[j]
            assert np.isnan(got[j]) == (mk == "z"), (SHAPES[j], ck, mk, got[j])  # N = 0: the reference's 0 / 0
            zero_masks += mk == "z"
            if ck not in "rn" or mk == "z":
                continue
            ref = _ref(ops, dev, data, j, ck, mk)
            lv = ref.level(11)
            assert float(lv.stats64.min()) >= 0.0, (SHAPES[j], ck, mk)
            bound = (3 * TERM_BOUND + ref.bound_cos) / 5 + 4 * lv.stats_bound
            print(f"{SHAPES[j]} {ck} {mk}: loss {got[j]:.9f} oracle {ref.oracle.loss:.9f} err {abs(got[j] - ref.oracle.loss):.3g} bound {bound:.3g}")
            assert abs(got[j] - ref.oracle.loss) <= bound, (SHAPES[j], ck, mk, got[j], ref.oracle.loss, bound)
            checked += 1
    assert checked >= 8 and zero_masks >= 2


# ------------------------------------------------------------------ 6. determinism and isolation
@pytest.mark.parametrize("call", [CALLS[2], CALLS[15]], ids=_id)
def test_an_image_alone_gives_its_batch_bits(ops, lib, dev, data, call):
    g = torch.Generator().manual_seed(72)
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    stats = _entry(lib, a, b, m, 11, dev)
    for j in everyone:
        ja, jb, jm = _batch(ops, data, dev, call, [j], g)
        alone = _entry(lib, ja, jb, jm, 11, dev)
        assert alone.shape == (1, 3, 5) and torch.equal(alone[0], stats[j]), (call, SHAPES[j])
    # lists of device tensors and of host arrays give the arenas' bits, on the cached plan of the shape list
    pairs, masks, _ = data
    kinds = _kinds(call)
    la, lb = [pairs[kinds[j][0]][j][0] for j in everyone], [pairs[kinds[j][0]][j][1] for j in everyone]
    lm = None if call[1] is None else [masks[kinds[j][1]][j] for j in everyone]
    assert torch.equal(ops.loss_stats_u8hwc_ragged(a, b, m), stats)
    n = len(ops._loss_ragged_plans)
    for x, y, z in (([t.to(dev) for t in la], [t.to(dev) for t in lb], None if lm is None else [t.to(dev) for t in lm]),
                    ([t.to(dev) for t in la], [t.numpy() for t in lb], lm)):
        assert torch.equal(ops.loss_stats_u8hwc_ragged(x, y, z), stats)
    assert len(ops._loss_ragged_plans) == n
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.loss_stats_u8hwc_ragged(ops.RaggedBytes.pack(la, dev), ops.RaggedBytes.pack(lb), None)


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


@pytest.mark.parametrize("call", [CALLS[3], CALLS[16]], ids=["no_masks", "masks"])
def test_nothing_outside_the_buffers_is_touched(ops, lib, dev, data, call):
    """The entry through the C ABI with every buffer inside one poisoned allocation (tests/guard_arena.py), under both
    poisons: stats is fully assigned and does not depend on the poison, the workspace's guards hold, the three arenas and the
    plan are unchanged -- and the statistics are, bit for bit, those of the plain call, whose count and terms are the
    references' (its L statistics are held in test_level_stats_window_11, on the same call)."""
    g = torch.Generator().manual_seed(75)
    everyone = list(range(B))
    a, b, m = _batch(ops, data, dev, call, everyone, g)
    host, _, ws_bytes = _plan(lib, SHAPES, int(m is not None), dev)
    bufs = [GA.Buf("a", GA.IN, data=a.arena.cpu()), GA.Buf("b", GA.IN, data=b.arena.cpu()), GA.Buf("plan", GA.IN, data=host, grid=16),
            GA.Buf("stats", GA.OUT, shape=(B, 3, 5), dtype=torch.float64), GA.Buf("ws", GA.WORK, nbytes=ws_bytes, grid=16)]
    if m is not None:
        bufs.append(GA.Buf("mask", GA.IN, data=m.arena.cpu()))

    def run(arena):
        rc = lib.curl_loss_ragged_u8hwc(arena.ptr("a"), arena.nbytes("a"), arena.ptr("b"), arena.nbytes("b"), arena.ptr("mask"),
                                        arena.nbytes("mask"), arena.ptr("stats"), arena.nbytes("stats"), arena.ptr("ws"),
                                        arena.nbytes("ws"), host.data_ptr(), arena.ptr("plan"), arena.nbytes("plan"), 11, 0,
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.curl_last_error()
    done = GA.run_both(bufs, "16", dev, run)
    stats = done.read("stats").to(dev)
    _hold(ops, dev, stats, data, call, everyone, "guarded")
    assert torch.equal(stats, _entry(lib, a, b, m, 11, dev))


# ------------------------------------------------------------------ 7. infer.enhance_and_evaluate_many and the folder CLI
def _same_loss(ops, got, outs, targets, masks, dev):
    """got against ONE ops call on the images of 32 pixels and more, nan for the others."""
    keep = [i for i, o in enumerate(outs) if min(o.shape[:2]) >= 32]
    assert 0 < len(keep) < len(outs)
    want = np.full(len(outs), np.nan)
    want[keep] = ops.curl_loss_u8hwc_ragged([torch.from_numpy(outs[i]).to(dev) for i in keep],
                                            [torch.from_numpy(np.ascontiguousarray(targets[i][..., :3])).to(dev) for i in keep],
                                            [torch.from_numpy(masks[i]).to(dev) for i in keep]).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[keep], want[keep]) and np.all((got[keep] > 0) & (got[keep] < 3)), (got, want)


def test_enhance_and_evaluate_many(ops, dev):
    from curl_amd import infer
    imgs, masks, targets = _files()
    net = _net(dev)
    want = infer.enhance_many(net, imgs, masks, dev)
    for foreground, batch_size in ((False, 4), (True, 3), (False, 1)):
        plain, psnr, msssim = infer.enhance_and_score_many_msssim(net, imgs, masks, targets, dev, batch_size=batch_size, foreground=foreground)
        outs, psnr2, msssim2, loss = infer.enhance_and_evaluate_many(net, imgs, masks, targets, dev, batch_size=batch_size, foreground=foreground)
        assert len(outs) == len(imgs) and np.array_equal(psnr, psnr2) and np.array_equal(msssim, msssim2, equal_nan=True)
        for o, p, w in zip(outs, plain, want):
            assert o.dtype == np.uint8 and np.array_equal(o, p) and np.array_equal(o, w)
        assert np.isnan(loss[0]) and loss.shape == (len(imgs),)  # 20 x 50: nan, and the batch did not fail
        _same_loss(ops, loss, outs, targets, masks, dev)
    # Every output scored against itself: rgb = lab = hsv = 0 exactly, the MS-SSIM term 0 to float32, and the cosine term 0 --
    # but for the unmasked pixels the net left BLACK: cosine_similarity of two zero vectors is 0, not 1 (model.py:97, its eps
    # clamp), so each of them adds 1 / (H W) to the cosine term and a fifth of that to the loss, in the reference as here.  The
    # issue's 1e-5 is held beside that count, which is 0 for an output without such pixels.
    _, _, _, same = infer.enhance_and_evaluate_many(net, imgs, masks, want, dev)
    assert np.isnan(same[0])
    for i in range(1, len(imgs)):
        black = int(((want[i].max(axis=2) == 0) & (masks[i] > 0)).sum())
        h, w = want[i].shape[:2]
        print(f"self-score {h}x{w}: loss {same[i]:.3g}, {black} unmasked black pixels -> {black / (5.0 * h * w):.3g}")
        assert abs(same[i] - black / (5.0 * h * w)) <= 1e-5, (i, same[i], black)


def test_infer_dir_loss_scores_the_files_it_writes(ops, dev, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from curl_amd import infer_dir
    imgs, masks, targets = _files()
    for d in ("in", "masks", "gt", "plain", "scored", "both"):
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
    assert infer_dir.main(base + ["--out_dir", str(tmp_path / "plain"), "--msssim"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert infer_dir.main(base + ["--out_dir", str(tmp_path / "both"), "--msssim", "--loss"]) == 0
    both = [ln.split("\t") for ln in capsys.readouterr().out.splitlines()]
    assert infer_dir.main(base + ["--out_dir", str(tmp_path / "scored"), "--loss"]) == 0
    rows = [ln.split("\t") for ln in capsys.readouterr().out.splitlines()]
    assert [r[0] for r in rows] == names + ["mean"] and [len(r) for r in rows] == [3, 3, 3, 3, 5]
    assert [len(r) for r in both] == [4, 4, 4, 4, 7]
    assert ["\t".join(r[:3]) for r in both[:4]] == plain[:4]  # the psnr and msssim columns are the run's without the flag
    assert [r[1] for r in rows[:4]] == [r[1] for r in both[:4]] and [r[2] for r in rows[:4]] == [r[3] for r in both[:4]]
    outs = []
    for name in names:
        for d in ("scored", "both"):
            assert (tmp_path / "plain" / f"{name}.png").read_bytes() == (tmp_path / d / f"{name}.png").read_bytes()
        outs.append(np.asarray(Image.open(tmp_path / "scored" / f"{name}.png")))
    got = np.array([float(r[2]) for r in rows[:4]])
    _same_loss(ops, got, outs, targets, masks, dev)
    assert abs(float(rows[4][2]) - got[1:].mean()) <= 1e-12 and rows[4][4] == "1"  # the mean over the finite ones
    assert both[4][3] == rows[4][2] and both[4][6] == "1"
