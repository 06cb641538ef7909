"""The byte edge at the sizes and batch counts its headers admit (the float32 kernels' counterpart is tests/test_gpu_scale.py):
2^30 pixels per image, 65535 images per call, arena offsets past 2^32.  Every test asserts from its layout alone that the
inputs reach what they are for, before a kernel runs; every test makes its own tensors on the device and frees them.

* test_score_second_pass_beyond_256_tiles: sse_ragged_final_kernel's loop over an image's tiles makes a second trip (259 and
  257 tiles) and six (1465 tiles, the 1500 x 1000 photograph), against numpy int64.
* test_65535_images_in_one_call: the limit of every ragged entry -- a descriptor search 15 levels deep in each class, the layer's knot set-up
  and pass 2 of the score with 65535 rows / workgroups -- against the uniform-batch entries, one call per shape.
* test_uniform_rgba_batch_past_2_to_32_bytes, test_uniform_rgb_batch_past_2_to_32_bytes: the uniform byte entries, the
  foreground entries and the single-image encoder view where `img * channels * plane` passes 2^32 bytes (and, for the masks,
  2^32 pixels): images before, past and at the end equal the image alone.
* test_ragged_arenas_past_2_to_32: one ragged batch of 4.3 Gpx -- the high words of the plan's 64-bit image, mask and out
  offsets, three images of 2^30 pixels and one of the byte class beside them (in-image byte offsets up to 2^32 - 4) -- through
  the forward, foreground, score and view entries.

Smallest first; peak device memory 45 GB (the last test), 34 GB in test_uniform_rgb_batch_past_2_to_32_bytes.
"""
import numpy as np
import pytest
import torch

import scale_bytes as SB
from ragged_score_ref import sse_ref

pytestmark = pytest.mark.gpu

KNOTS = (48, 48, 64)


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


def _rows(sums):
    return [tuple(int(v) for v in row) for row in sums.cpu()]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ 3. the score's second pass beyond 256 tiles per image
SCORE_SHAPES = [(257, 257), (512, 514), (1000, 1500), (1, 1)]
SCORE_CONTENTS, SCORE_MASKS = "rxt", "fzcl"  # tests/test_gpu_ragged_score.py's kinds


def _score_data():
    """content kind -> the (a, b) pairs; mask kind -> the masks; host tensors, as tests/test_gpu_ragged_score.py makes them."""
    g = torch.Generator().manual_seed(2911)

    def rnd(*shape):
        return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)
    pairs, masks = {k: [] for k in SCORE_CONTENTS}, {k: [] for k in SCORE_MASKS}
    for h, w in SCORE_SHAPES:
        a = rnd(h, w, 3)
        pairs["r"].append((a, rnd(h, w, 3)))
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
        masks["c"].append(torch.tensor(SB.MASK_LEVELS, dtype=torch.uint8)[torch.randint(0, 4, (h, w), generator=g)])
        masks["l"].append(last)
    return pairs, masks


def _noisy(ops, tensors, dev, g):
    """RaggedBytes.pack into an arena of random bytes: the padding between the images is not zero."""
    shapes, channels = [tuple(t.shape[:2]) for t in tensors], [t.shape[2] if t.dim() == 3 else 1 for t in tensors]
    offsets, nbytes = ops.RaggedBytes.layout(shapes, channels)
    arena = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.int32).to(torch.uint8)
    for t, o in zip(tensors, offsets):
        arena[o:o + t.numel()] = t.reshape(-1)
    return ops.RaggedBytes(arena.to(dev), shapes, offsets, channels)


def test_score_second_pass_beyond_256_tiles(ops, dev):
    """Pass 2 sums an image's per-workgroup pairs 256 at a time.  (257, 257) is the byte class with 259 tiles, (512, 514) the
    dword class with 257, (1000, 1500) has 1465 -- six trips -- and (1, 1) one.  In call (r, m) image j takes content
    (j + r) mod 3 and mask (j + m) mod 4 (m None: no mask arena), so every image meets every pair; each call in this order and
    reversed, two of them image by image, all EXACTLY numpy int64's sums."""
    n = len(SCORE_SHAPES)
    want_tiles = [("byte", 259), ("dword", 257), ("dword", 1465), ("byte", 1)]
    assert [SB.score_tiles(h, w) for h, w in SCORE_SHAPES] == want_tiles
    assert SB.plan_tiles(ops, SCORE_SHAPES) == [t for _, t in want_tiles]  # ... and they are the library's counts
    assert [t > 256 for _, t in want_tiles] == [True, True, True, False] and -(-1465 // 256) == 6
    pairs, masks = _score_data()
    memo = {}

    def ref(j, ck, mk):
        if (j, ck, mk) not in memo:
            a, b = pairs[ck][j]
            memo[j, ck, mk] = sse_ref(a.numpy(), b.numpy(), None if mk is None else masks[mk][j].numpy())
        return memo[j, ck, mk]
    j = SCORE_SHAPES.index((1000, 1500))
    assert ref(j, "x", None) == (1500000 * 3 * 255 * 255, 1500000) and ref(j, "x", None)[0] > 2 ** 32
    assert ref(j, "t", "f") == (2, 1500000) and ref(j, "t", "l") == (1, 1) and ref(j, "r", "z") == (0, 0)

    g = torch.Generator().manual_seed(12)
    calls = [(r, m) for r in range(3) for m in (None, 0, 1, 2, 3)]
    seen = set()
    for r, m in calls:
        kinds = [(SCORE_CONTENTS[(i + r) % 3], None if m is None else SCORE_MASKS[(i + m) % 4]) for i in range(n)]
        seen |= {(i, k) for i, k in enumerate(kinds)}
        want = [ref(i, *kinds[i]) for i in range(n)]
        orders = [list(range(n)), list(range(n))[::-1]] + ([[i] for i in range(n)] if (r, m) in ((1, None), (2, 2)) else [])
        for order in orders:
            a = _noisy(ops, [pairs[kinds[i][0]][i][0] for i in order], dev, g)
            b = _noisy(ops, [pairs[kinds[i][0]][i][1] for i in order], dev, g)
            mm = None if m is None else _noisy(ops, [masks[kinds[i][1]][i] for i in order], dev, g)
            got = _rows(ops.sse_u8hwc_ragged(a, b, mm))
            assert got == [want[i] for i in order], ((r, m), order, got, want)
    assert seen == {(i, (c, k)) for i in range(n) for c in SCORE_CONTENTS for k in list(SCORE_MASKS) + [None]}


# ------------------------------------------------------------------ 2. 65535 images in one call
MANY = 65535
MANY_SHAPES = [(1, 1, 3), (2, 2, 4), (3, 5, 3), (4, 8, 4), (1, 257, 3), (4, 257, 4), (7, 9, 4), (8, 8, 3)]
MANY_VIEW_SHAPES = [(8, 8, 3), (9, 12, 4), (16, 8, 3), (12, 20, 4)]


def _many_masks(lay, g):
    """A mask arena of random bytes; every third image's mask is all 0, every third one's drawn from {0, 1, 128, 255}."""
    arena = SB.rand_u8(g, lay.dev, lay.mask_bytes)
    for key in lay.groups:
        idx, ids = lay.index(key, "mask"), lay.ids(key)
        arena[idx[ids % 3 == 0]] = 0
        some = idx[ids % 3 == 1]
        arena[some] = SB.level_bytes(g, lay.dev, *some.shape)
    return arena


def test_65535_images_in_one_call(ops, dev):
    """B = 65535, the limit: eight shapes in turn (both classes, RGB and RGBA in each), per-image coefficients, knots and masks,
    arenas of random bytes.  Per shape ONE call of the uniform-batch entry on the stack of that shape's 8192 images is the
    reference; the ragged bytes are gathered from the out arena with one index tensor per shape."""
    shapes = [MANY_SHAPES[i % 8] for i in range(MANY)]
    lay = SB.Layout(ops, shapes, dev)
    assert len(shapes) == MANY == 65535 and len(lay.groups) == 8 and max(len(v) for v in lay.groups.values()) <= 8192
    classes = {(SB.score_tiles(h, w)[0], c) for h, w, c in MANY_SHAPES}
    assert classes == {("dword", 3), ("dword", 4), ("byte", 3), ("byte", 4)}
    n_dword = sum(SB.score_tiles(h, w)[0] == "dword" for h, w, _ in shapes)
    assert min(n_dword, MANY - n_dword) > 2 ** 14  # each class's descriptor search is 15 levels deep (3 in the other tests)
    g = torch.Generator(device=dev).manual_seed(65535)
    img = lay.ragged(SB.rand_u8(g, dev, lay.img_bytes), "img")
    masks = lay.ragged(_many_masks(lay, g), "mask")
    coeffs = {nc: torch.randn(MANY, 3, 3, nc, device=dev, generator=g) * 0.2 for nc in (35, 126)}
    knots = [torch.randn(MANY, n, device=dev, generator=g) * 0.1 for n in KNOTS]
    pad = lay.padding("out")
    assert pad.numel() > MANY // 2

    stacks = {}  # shape -> (ids, RGB stack [n,h,w,3], mask stack [n,h,w], out index)
    for key in lay.groups:
        h, w, c = key
        n = len(lay.groups[key])
        stacks[key] = (lay.ids(key), img.arena[lay.index(key, "img")].view(n, h, w, c)[..., :3].contiguous(),
                       masks.arena[lay.index(key, "mask")].view(n, h, w), lay.index(key, "out"))

    def check(out, want_of, name):
        assert out.offsets == lay.out_off and out.arena.numel() == lay.out_bytes, name
        for key, (ids, rgb, m, oidx) in stacks.items():
            want = want_of(ids, rgb, m)
            got = out.arena[oidx].view(want.shape)
            assert torch.equal(got, want), (name, key, int((got != want).sum()))
        assert bool((out.arena[pad] == SB.POISON).all()), name

    def check_reg(reg, want_of, name):
        assert reg.shape == (MANY,)
        for key, (ids, rgb, m, _) in stacks.items():
            assert _same_bits(reg[ids], want_of(ids, rgb, m)), (name, key)

    with SB.prefilled_out(ops):
        outs = {}
        for nc in (35, 126):
            for wm in (masks, None):
                out = ops.trispace_forward_u8hwc_ragged(img, coeffs[nc], wm)
                check(out, lambda ids, rgb, m: ops.trispace_forward_u8hwc(rgb, coeffs[nc][ids], m if wm is not None else None),
                      ("trispace", nc, wm is not None))
                outs[nc, wm is not None] = out
            fg = ops.trispace_foreground_u8hwc_ragged(img, coeffs[nc], masks)
            assert torch.equal(fg.arena, outs[nc, True].arena), ("trispace foreground", nc)
        for wm in (masks, None):
            def layer(ids, rgb, m):
                return ops.curl_layer_forward_u8hwc(rgb, None, *(k[ids] for k in knots), m if wm is not None else None)
            out, reg = ops.curl_layer_forward_u8hwc_ragged(img, *knots, wm)
            check(out, lambda ids, rgb, m: layer(ids, rgb, m)[0], ("layer", wm is not None))
            check_reg(reg, lambda ids, rgb, m: layer(ids, rgb, m)[1], ("layer", wm is not None))
            outs["layer", wm is not None] = out, reg
        fg, fg_reg = ops.curl_layer_foreground_u8hwc_ragged(img, *knots, masks)
        assert torch.equal(fg.arena, outs["layer", True][0].arena) and _same_bits(fg_reg, outs["layer", True][1])
        del fg, fg_reg

    # the score of (the images' RGB, the 35-coefficient outputs) under the masks and without: numpy int64 per shape
    b = outs[35, True]
    a = lay.ragged(SB.rand_u8(g, dev, lay.out_bytes), "out")
    for key, (ids, rgb, m, oidx) in stacks.items():
        a.arena[oidx] = rgb.view(len(ids), -1)
    for mm in (masks, None):
        sums = ops.sse_u8hwc_ragged(a, b, mm)
        assert sums.shape == (MANY, 2)
        got = sums.cpu().numpy()
        for key, (ids, rgb, m, oidx) in stacks.items():
            x, y = rgb.cpu().numpy().astype(np.int64), b.arena[oidx].view(rgb.shape).cpu().numpy().astype(np.int64)
            keep = (m.cpu().numpy() != 0).astype(np.int64) if mm is not None else np.ones(x.shape[:3], dtype=np.int64)
            want = np.stack([(keep[..., None] * (x - y) ** 2).sum(axis=(1, 2, 3)), keep.sum(axis=(1, 2))], axis=1)
            assert np.array_equal(got[ids.cpu().numpy()], want), (key, mm is not None)
            if key == (8, 8, 3):
                i = lay.groups[key][0]  # ... and one image through the module's own reference
                assert tuple(got[i]) == sse_ref(a.image(i).cpu().numpy(), b.image(i).cpu().numpy(),
                                                None if mm is None else masks.image(i).cpu().numpy())
    del outs, a, b, stacks, img, masks

    # the views, on shapes the view admits at size 8
    vshapes = [MANY_VIEW_SHAPES[i % 4] for i in range(MANY)]
    vlay = SB.Layout(ops, vshapes, dev)
    assert all(min(h, w) / 8 <= 64 for h, w, _ in MANY_VIEW_SHAPES)
    vimg = vlay.ragged(SB.rand_u8(g, dev, vlay.img_bytes), "img")
    vmask = vlay.ragged(_many_masks(vlay, g), "mask")
    view, mview = ops.encoder_view_u8hwc_ragged(vimg, vmask, size=8)
    assert view.shape == (MANY, 3, 8, 8) and mview.shape == (MANY, 1, 8, 8)
    for key in vlay.groups:
        h, w, c = key
        ids, n = vlay.ids(key), len(vlay.groups[key])
        want, want_m = ops.encoder_view_u8hwc(vimg.arena[vlay.index(key, "img")].view(n, h, w, c),
                                              vmask.arena[vlay.index(key, "mask")].view(n, h, w), size=8)
        assert torch.equal(view[ids], want) and torch.equal(mview[ids], want_m), key
    del vimg, vmask, view, mview

    # one image more is refused, with the limit in the message
    with pytest.raises(ValueError, match="65535"):
        ops.RaggedBytes.layout([(1, 1)] * 65536, [3] * 65536)
    small = torch.zeros(65536 * 16, dtype=torch.uint8, device=dev)
    too_many = ops.RaggedBytes(small, [(1, 1)] * 65536, [16 * i for i in range(65536)], [3] * 65536)
    with pytest.raises(ValueError, match="65535"):
        ops.trispace_forward_u8hwc_ragged(too_many, torch.zeros(65536, 3, 3, 35, device=dev))
    with pytest.raises(ValueError, match="65535"):
        ops.encoder_view_u8hwc_ragged(too_many, None, size=8)
    ops._ragged_plans.clear()        # (the plans of 65535 images: 4 MB each on the host and on the device)
    ops._view_ragged_plans.clear()
    del small, too_many
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4. uniform byte batches past 2^32
def _alone_fg(ops, img, fg, coeffs, knots, picks, outs):
    """Images `picks` of the two foreground entries' batch results equal the entries on the image alone."""
    for b in picks:
        s = slice(b, b + 1)
        for nc, got in outs["tri"].items():
            assert torch.equal(ops.trispace_foreground_u8hwc(img[s], coeffs[nc][s], fg[s])[0], got[b]), ("tri", nc, b)
        o1, r1 = ops.curl_layer_foreground_u8hwc(img[s], *(k[s] for k in knots), fg[s])
        assert torch.equal(o1[0], outs["layer"][0][b]) and _same_bits(r1, outs["layer"][1][s]), ("layer", b)


def test_uniform_rgba_batch_past_2_to_32_bytes(ops, dev):
    """[270, 1999, 2001, 4]: RGBA and the byte class (H*W is odd), 4.32 GB in -- image 269 starts past 2^32 bytes.  Both
    foreground entries and the single-image encoder view at size 64: images 0 and 269 equal the image alone."""
    B, H, W = 270, 1999, 2001
    assert (H * W) % 4 != 0 and (B - 1) * H * W * 4 >= 2 ** 32 and min(H, W) / 64 <= 64
    g = torch.Generator(device=dev).manual_seed(270)
    img = SB.rand_u8(g, dev, B, H, W, 4)
    fg = SB.banded_mask(g, dev, B, H, W)
    assert not fg[:, 0::8].any() and bool((fg[:, 2::8] == 255).all())
    coeffs = {nc: torch.randn(B, 3, 3, nc, device=dev, generator=g) * 0.2 for nc in (35, 126)}
    knots = [torch.randn(B, n, device=dev, generator=g) * 0.1 for n in KNOTS]
    picks = (0, B - 1)
    outs = {"tri": {nc: ops.trispace_foreground_u8hwc(img, coeffs[nc], fg) for nc in (35, 126)},
            "layer": ops.curl_layer_foreground_u8hwc(img, *knots, fg)}
    _alone_fg(ops, img, fg, coeffs, knots, picks, outs)
    del outs
    view, mview = ops.encoder_view_u8hwc(img, fg, size=64)
    assert view.shape == (B, 3, 64, 64) and mview.shape == (B, 1, 64, 64)
    for b in picks:
        v1, m1 = ops.encoder_view_u8hwc(img[b:b + 1], fg[b:b + 1], size=64)
        assert torch.equal(v1[0], view[b]) and torch.equal(m1[0], mview[b]), b
    del img, fg, view, mview
    torch.cuda.empty_cache()


def test_uniform_rgb_batch_past_2_to_32_bytes(ops, dev):
    """[1075, 2000, 2000, 3]: 12.9 GB in and out, the dword class; the white mask and the bool layer mask are 4.3 Gpx each, so
    the MASK index passes 2^32 at image 1074.  The row-tiled operator with a white mask, the layer with both masks and the two
    foreground entries, one after another: images 0, 358 (the first wholly past 2^32 bytes) and 1074 equal the image alone."""
    B, H, W = 1075, 2000, 2000
    picks = (0, 358, B - 1)
    assert (H * W) % 4 == 0 and 357 * H * W * 3 < 2 ** 32 <= 358 * H * W * 3
    assert (B - 2) * H * W < 2 ** 32 <= (B - 1) * H * W
    g = torch.Generator(device=dev).manual_seed(1075)
    img = SB.rand_u8(g, dev, B, H, W, 3)
    white = SB.banded_mask(g, dev, B, H, W)
    lmask = SB.rand_u8(g, dev, B, 1, H, W) > 63
    coeffs = {nc: torch.randn(B, 3, 3, nc, device=dev, generator=g) * 0.2 for nc in (35, 126)}
    knots = [torch.randn(B, n, device=dev, generator=g) * 0.1 for n in KNOTS]

    out = ops.trispace_forward_u8hwc(img, coeffs[126], white)
    for b in picks:
        s = slice(b, b + 1)
        assert torch.equal(ops.trispace_forward_u8hwc(img[s], coeffs[126][s], white[s])[0], out[b]), b
    del out
    out, reg = ops.curl_layer_forward_u8hwc(img, lmask, *knots, white)
    for b in picks:
        s = slice(b, b + 1)
        o1, r1 = ops.curl_layer_forward_u8hwc(img[s], lmask[s], *(k[s] for k in knots), white[s])
        assert torch.equal(o1[0], out[b]) and _same_bits(r1, reg[s]), b
    del out, reg, lmask
    for nc in (126, 35):
        out = ops.trispace_foreground_u8hwc(img, coeffs[nc], white)
        for b in picks:
            s = slice(b, b + 1)
            assert torch.equal(ops.trispace_foreground_u8hwc(img[s], coeffs[nc][s], white[s])[0], out[b]), (nc, b)
        del out
    out, reg = ops.curl_layer_foreground_u8hwc(img, *knots, white)
    for b in picks:
        s = slice(b, b + 1)
        o1, r1 = ops.curl_layer_foreground_u8hwc(img[s], *(k[s] for k in knots), white[s])
        assert torch.equal(o1[0], out[b]) and _same_bits(r1, reg[s]), b
    del out, reg, img, white
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 1. ragged arenas whose offsets need their high words
BIG = [(512, 514, 3), (32768, 32768, 3), (32768, 32768, 3), (32768, 32768, 3), (32767, 32767, 3), (12, 20, 4), (33, 65, 3), (1, 1, 3)]
BIG_IMAGES, SMALL_IMAGES = (1, 2, 3, 4), (0, 5, 6, 7)
# the rows of a big image's mask tile: 0 from end to end, 255 from end to end, or drawn from {0, 1, 128, 255}
MASK_TILE_ROWS = ("zero", "full", "levels", "levels", "zero", "levels", "full", "levels")
BAND_SHARE_INSIDE, BAND_SHARE_EXEMPT, BYTE_TOL = 0.40, 0.015, 2e-5


def big_batch_host(seed=4295):
    """What the big batch is made from, on the host (a few MB): per big image one [8,W,C] tile of random bytes and one [8,W]
    mask tile, the small images and masks whole, per-image coefficients (randn * 0.05) and knots (randn * 0.1)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)
    levels = torch.tensor(SB.MASK_LEVELS, dtype=torch.uint8)
    imgs, masks = {}, {}
    for i, (h, w, c) in enumerate(BIG):
        rows = 8 if i in BIG_IMAGES else h
        imgs[i] = rnd(rows, w, c)
        m = levels[torch.randint(0, 4, (rows, w), generator=g)]
        if i in BIG_IMAGES:
            for r, kind in enumerate(MASK_TILE_ROWS):
                if kind != "levels":
                    m[r] = 0 if kind == "zero" else 255
        masks[i] = m
    coeffs = {nc: torch.randn(len(BIG), 3, 3, nc, generator=g) * 0.05 for nc in (35, 126)}
    knots = [torch.randn(len(BIG), n, generator=g) * 0.1 for n in KNOTS]
    return imgs, masks, coeffs, knots


def oracle_band(band_u8, coeffs, r0, H):
    """The oracle's float32 result [1,3,8,W] of the 126-coefficient operator on rows [r0, r0 + 8) of an image H rows high."""
    import curl_oracle as O
    x = O.u8hwc_to_f32chw(band_u8.numpy())[None]
    c = coeffs[None]
    return O.generate_image(x, O.trispace_residual(x, c[:, 0], c[:, 1], c[:, 2], rows=(r0, H)))


def band_shares(ref):
    """-> (share of the band's bytes strictly inside (0, 1), share of those within BYTE_TOL of a byte boundary, that mask)"""
    v = ref.numpy().astype(np.float64)
    inside = (v > 0.0) & (v < 1.0)
    near = np.abs(v * 255.0 - np.round(v * 255.0)) <= BYTE_TOL * 255.0
    return inside.mean(), (near & inside).sum() / max(inside.sum(), 1), near


def test_ragged_arenas_past_2_to_32(ops, dev):
    """One batch of 4.3 Gpx: a small dword-class image, three of 32768 x 32768 (the API limit), one of 32767 x 32767 (the byte
    class for every operator) and three small images whose image, out AND mask offsets lie past 2^32.  The big images and their
    masks repeat a tile of eight rows, so the pointwise operators' outputs must repeat theirs: every byte of the batch is pinned
    to a call at a size the suite already pins.  Peak device memory 45 GB (image, RGB copy and out arenas of 12.9 GB, masks 4.3,
    the integer sums' temporaries).  6 s on the MI355X, most of it the host's: four oracle bands of 8 x 32768 pixels and the
    device-side integer sums; no kernel call takes more than tens of milliseconds."""
    from PIL import Image
    import encoder_view_cases as cases
    lay = SB.Layout(ops, BIG, dev)
    B = len(BIG)
    for i in (5, 6, 7):
        assert min(lay.img_off[i], lay.out_off[i], lay.mask_off[i]) >= 2 ** 32, i
    assert sum(h * w for h, w, _ in BIG[:5]) == 4295164929 and 32767 * 32767 == 1073676289 <= 2 ** 30 == 32768 * 32768
    assert all(SB.score_tiles(h, w)[0] == "dword" for h, w, _ in BIG[:4]) and 32767 % 4 != 0 and (32767 * 32767) % 4 != 0
    tiles, mtiles, coeffs_h, knots_h = big_batch_host()
    for i in BIG_IMAGES:
        assert not mtiles[i][0].any() and bool((mtiles[i][1] == 255).all()) and set(mtiles[i][2].tolist()) == set(SB.MASK_LEVELS)

    # the oracle's bands of the 126-coefficient operator, and the two conditions on them, before any kernel runs
    bands = {}
    for i, r0 in ((4, 0), (4, 16380), (4, 32767 - 8), (3, 32768 - 8)):
        H = BIG[i][0]
        band = torch.stack([tiles[i][(r0 + k) % 8] for k in range(8)])
        ref = oracle_band(band, coeffs_h[126][i], r0, H)
        inside, exempt, near = band_shares(ref)
        print(f"oracle band image {i} rows {r0}..{r0 + 7}: {inside:.4f} of the bytes inside (0, 1), {exempt:.4f} of those exemptible")
        assert inside >= BAND_SHARE_INSIDE and exempt <= BAND_SHARE_EXEMPT, (i, r0, inside, exempt)
        bands[i, r0] = band, ref, near
    # Pillow's coefficients at the integer scale 64 do not depend on where the window lies
    head, tail, cut = cases.axis_rows(32768, 512, 0, 5), cases.axis_rows(32768, 512, 507, 5), cases.axis_rows(384, 6)
    assert np.array_equal(head, cut[:5]) and np.array_equal(tail[:, 1:], cut[1:, 1:])
    assert np.array_equal(tail[:, 0] - (32768 - 384), cut[1:, 0]) and int(cut[5, 1]) < int(cut[4, 1])  # row 5: the cut clips it

    g = torch.Generator(device=dev).manual_seed(1)
    img = lay.ragged(SB.rand_u8(g, dev, lay.img_bytes), "img")
    masks = lay.ragged(SB.rand_u8(g, dev, lay.mask_bytes), "mask")
    for i in range(B):
        if i in BIG_IMAGES:
            SB.fill_periodic(img.image(i), tiles[i].to(dev))
            SB.fill_periodic(masks.image(i)[:, :, None], mtiles[i].to(dev)[:, :, None])
        else:
            img.image(i).copy_(tiles[i])
            masks.image(i).copy_(mtiles[i])
    for i in BIG_IMAGES:
        assert SB.differs_from_periodic(masks.image(i)) == 0
    coeffs = {nc: c.to(dev) for nc, c in coeffs_h.items()}
    knots = [k.to(dev) for k in knots_h]
    pad = lay.padding("out")
    assert pad.numel() > 0

    def first_rows(i):
        """image i alone where it is small, else its first eight rows as an image of their own: (RGB [1,h,W,3], mask [1,h,W])"""
        rows = slice(0, 8) if i in BIG_IMAGES else slice(None)
        return img.image(i)[rows][None, ..., :3].contiguous(), masks.image(i)[rows][None].contiguous()

    def check_pointwise(out, alone, name):
        assert out.offsets == lay.out_off and out.arena.numel() == lay.out_bytes
        for i in range(B):
            got = out.image(i)
            if i in BIG_IMAGES:
                assert SB.differs_from_periodic(got) == 0, (name, i)
                got = got[:8]
            want = alone(i, *first_rows(i))
            assert torch.equal(got, want), (name, i, int((got != want).sum()))
        assert bool((out.arena[pad] == SB.POISON).all()), name

    with SB.prefilled_out(ops):
        # 35 coefficients (pointwise), its foreground entry, and the score of its output
        out35 = ops.trispace_forward_u8hwc_ragged(img, coeffs[35], masks)
        check_pointwise(out35, lambda i, x, m: ops.trispace_forward_u8hwc(x, coeffs[35][i:i + 1], m)[0], "35")
        fg = ops.trispace_foreground_u8hwc_ragged(img, coeffs[35], masks)
        assert torch.equal(fg.arena, out35.arena)
        del fg
        torch.cuda.empty_cache()
        rgb = lay.ragged(img.arena[:lay.out_bytes].clone(), "out")  # the images in the RGB layout (only (12, 20, 4) is RGBA)
        for i in (5, 6, 7):
            rgb.image(i).copy_(img.image(i)[..., :3])
        for i in range(5):
            assert lay.img_off[i] == lay.out_off[i]
        for flipped in (False, True):
            if flipped:  # per-image sums far past 2^32
                rgb.image(4).copy_(255 - out35.image(4))
            want_m = [SB.int_sse(rgb.image(i), out35.image(i), masks.image(i)) for i in range(B)]
            want = [SB.int_sse(rgb.image(i), out35.image(i)) for i in range(B)]
            assert not flipped or want[4][0] > 2 ** 40
            assert _rows(ops.sse_u8hwc_ragged(rgb, out35, masks)) == want_m, flipped
            assert _rows(ops.sse_u8hwc_ragged(rgb, out35, None)) == want, flipped
        del rgb, out35
        torch.cuda.empty_cache()

        # the layer and its foreground entry
        def layer_alone(i, x, m):
            return ops.curl_layer_forward_u8hwc(x, None, *(k[i:i + 1] for k in knots), m)
        out, reg = ops.curl_layer_forward_u8hwc_ragged(img, *knots, masks)
        check_pointwise(out, lambda i, x, m: layer_alone(i, x, m)[0][0], "layer")
        for i in range(B):
            assert _same_bits(reg[i:i + 1], layer_alone(i, *first_rows(i))[1]), i
        fg, fg_reg = ops.curl_layer_foreground_u8hwc_ragged(img, *knots, masks)
        assert torch.equal(fg.arena, out.arena) and _same_bits(fg_reg, reg)
        del fg, fg_reg, out, reg
        torch.cuda.empty_cache()

        # 126 coefficients (row-tiled, spatial): under the masks against the uniform entry on an image alone ...
        out = ops.trispace_forward_u8hwc_ragged(img, coeffs[126], masks)
        for i in (3, 4) + SMALL_IMAGES:
            want = ops.trispace_forward_u8hwc(img.image(i)[None, ..., :3].contiguous(), coeffs[126][i:i + 1], masks.image(i)[None])[0]
            assert torch.equal(out.image(i), want), i
            del want
        assert bool((out.arena[pad] == SB.POISON).all())
        del out
        torch.cuda.empty_cache()
        # ... and without them against the oracle's bands: bytes differ by at most 1, and only beside a byte boundary
        out = ops.trispace_forward_u8hwc_ragged(img, coeffs[126], None)
        for (i, r0), (band, ref, near) in bands.items():
            assert torch.equal(img.image(i)[r0:r0 + 8].cpu(), band), (i, r0)
            got = out.image(i)[r0:r0 + 8].cpu().numpy().astype(np.int64)
            want = (ref.numpy()[0] * np.float32(255)).astype("uint8").transpose(1, 2, 0).astype(np.int64)
            diff = got != want
            assert np.abs(got - want).max() <= 1 and (~diff | near[0].transpose(1, 2, 0)).all(), (i, r0, int(diff.sum()))
        assert bool((out.arena[pad] == SB.POISON).all())
        del out
        torch.cuda.empty_cache()

    # the views at size 512, the least the 64x limit admits for 32768 rows
    assert 32768 / 512 == 64
    view, mview = ops.encoder_view_u8hwc_ragged(img, masks, size=512)
    assert view.shape == (B, 3, 512, 512) and mview.shape == (B, 1, 512, 512)
    for i in range(B):
        v1, m1 = ops.encoder_view_u8hwc(img.image(i)[None], masks.image(i)[None], size=512)
        assert torch.equal(v1[0], view[i]) and torch.equal(m1[0], mview[i]), i
    view3 = view[3].cpu().numpy()
    got = np.rint(view3 * 255.0).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(got.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0), view3)  # the view is bytes / 255
    top = np.asarray(Image.fromarray(img.image(3)[:384].cpu().numpy()).resize((512, 6), Image.BILINEAR))
    bottom = np.asarray(Image.fromarray(img.image(3)[-384:].cpu().numpy()).resize((512, 6), Image.BILINEAR))
    assert np.array_equal(got[:5], top[:5]) and np.array_equal(got[-5:], bottom[1:])
    del img, masks, view, mview
    ops._ragged_plans.clear()
    ops._view_ragged_plans.clear()
    torch.cuda.empty_cache()
