"""The encoder views of a ragged batch on the GPU (curl_encoder_view_ragged_u8hwc, ops.encoder_view_u8hwc_ragged,
infer.enhance_many(view="pil")): every image's view in one launch, against Pillow's own output (tests/golden/encoder_view.npz;
the cases and what each exercises: tests/encoder_view_cases.py) and against the single-image entry.  Equality is exact
everywhere -- torch.equal -- because the arithmetic is integer, byte / 255 is correctly rounded and one copy of the tile code
serves both kernels.

Batch 1 (size 32, ten images): 40x56, 56x40 (both crop axes), 32x33, 32x35 (both half-margin roundings), the two 37x37 (row
pitch 111: no row dword aligned), 20x27 (up-scaling), 641x481 (15x down-scaling: a tiling of its own), rgba_40x56 (RGBA beside
RGB), sparse_56x40 (a mask whose `> 0` sits on a rounded byte)."""
import random

import numpy as np
import pytest
import torch

import encoder_view_cases as cases
import guard_arena as GA

pytestmark = pytest.mark.gpu

BATCH1 = [("40x56", 0), ("56x40", 0), ("32x33", 0), ("32x35", 0), ("37x37_b2", 0), ("37x37_b2", 1), ("20x27", 0), ("641x481", 0),
          ("rgba_40x56", 0), ("sparse_56x40", 0)]
HEADER_WORDS, DESC_WORDS = 32, 32


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
def golden():
    return np.load(cases.GOLDEN)


def _item(golden, name, b=0):
    """(img u8 [H,W,C], mask u8 [H,W], want view f32 [3,S,S], want mask view f32 [1,S,S]) of image b of a case; CPU tensors"""
    img, mask = cases.inputs(name, golden)
    want = torch.from_numpy(golden[f"{name}/view"].astype(np.float32) / np.float32(255.0))
    want_m = torch.from_numpy((golden[f"{name}/mask_view"] > 0).astype(np.float32))[:, None]
    return torch.from_numpy(img[b]), torch.from_numpy(mask[b]), want[b], want_m[b]


@pytest.fixture(scope="module")
def batch1(golden, dev):
    """The ten images and masks on the device and Pillow's views of them (made once, never changed)."""
    items = [_item(golden, name, b) for name, b in BATCH1]
    return ([t[0].to(dev) for t in items], [t[1].to(dev) for t in items], torch.stack([t[2] for t in items]), torch.stack([t[3] for t in items]))


def _shapes(imgs):
    return [tuple(t.shape) for t in imgs]


def _host_plan(lib, shapes, size, has_mask=1):
    B = len(shapes)
    hs, ws, cs = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(3))
    nbytes = lib.curl_encoder_view_ragged_plan_bytes(B, hs.ctypes.data, ws.ctypes.data, size)
    assert nbytes > 0
    host = torch.zeros(nbytes // 4, dtype=torch.int32)
    rc = lib.curl_encoder_view_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, size, host.data_ptr(), nbytes)
    assert rc == 0, lib.curl_last_error()
    return host


def _desc(host):
    B = int(host[1])
    return host.numpy()[HEADER_WORDS:HEADER_WORDS + B * DESC_WORDS].reshape(B, DESC_WORDS)


def _offsets(host):
    """-> (img_off, mask_off per image, [image arena bytes, mask arena bytes])"""
    off = np.ascontiguousarray(_desc(host)[:, 20:24]).view(np.int64)
    sizes = np.ascontiguousarray(host.numpy()[8:12]).view(np.int64)
    return [int(v) for v in off[:, 0]], [int(v) for v in off[:, 1]], [int(v) for v in sizes]


def _arena_of(parts, offsets, nbytes, fill):
    """The images at their offsets; every byte between them holds `fill`."""
    a = torch.full((nbytes,), fill, dtype=torch.uint8)
    for t, o in zip(parts, offsets):
        a[o:o + t.numel()] = t.cpu().reshape(-1)
    return a


# ------------------------------------------------------------------ 1. Pillow's values
def test_batch_of_ten_at_32_is_pillows(ops, dev, batch1):
    from curl_amd import _lib
    imgs, masks, want, want_m = batch1
    assert len(imgs) == 10 and {t.shape[2] for t in imgs} == {3, 4}
    d = _desc(_host_plan(_lib.load(), _shapes(imgs), 32))
    assert len({(int(r[8]), int(r[9])) for r in d}) > 1 and len({int(r[15]) for r in d}) > 1  # tilings differ inside the batch
    view, mview = ops.encoder_view_u8hwc_ragged(imgs, masks, size=32)
    assert view.dtype == mview.dtype == torch.float32 and view.shape == (10, 3, 32, 32) and mview.shape == (10, 1, 32, 32)
    assert torch.equal(view.cpu(), want), (view.cpu() != want).nonzero()[:4]
    assert torch.equal(mview.cpu(), want_m), (mview.cpu() != want_m).nonzero()[:4]
    v2, m2 = ops.encoder_view_u8hwc_ragged(imgs, None, size=32)  # without masks: the same view, no mask view
    assert m2 is None and torch.equal(v2, view)
    # the arena form: packed RaggedBytes in, the same bits out
    v3, m3 = ops.encoder_view_u8hwc_ragged(ops.RaggedBytes.pack(imgs), ops.RaggedBytes.pack(masks), size=32)
    assert torch.equal(v3, view) and torch.equal(m3, mview)


@pytest.mark.parametrize("name,size,other", [("1000x1500_s320", 320, "12x20"), ("97x1003_s16", 16, "40x56")])
def test_batches_at_320_and_16(ops, dev, golden, name, size, other):
    """The golden case beside a small image of another tiling (12x20: up-scaling at 320; a formula image of 40x56 at 16): the
    first against Pillow, the second against the single-image entry."""
    img, mask, want, want_m = _item(golden, name)
    h, w = (int(v) for v in other.split("x"))
    img2 = torch.from_numpy(cases.formula_image(1, h, w, 3, seed=5)[0]).to(dev)
    mask2 = torch.from_numpy(cases.formula_mask(1, h, w, seed=5)[0]).to(dev)
    view, mview = ops.encoder_view_u8hwc_ragged([img.to(dev), img2], [mask.to(dev), mask2], size=size)
    assert torch.equal(view[0].cpu(), want) and torch.equal(mview[0].cpu(), want_m)
    alone, alone_m = ops.encoder_view_u8hwc(img2[None], mask2[None], size=size)
    assert torch.equal(view[1], alone[0]) and torch.equal(mview[1], alone_m[0])
    view, mview = ops.encoder_view_u8hwc_ragged([img2, img.to(dev)], None, size=size)
    assert mview is None and torch.equal(view[1].cpu(), want) and torch.equal(view[0], alone[0])


# ------------------------------------------------------------------ 2. order and company do not matter
def test_order_and_company_do_not_matter(ops, dev, batch1):
    imgs, masks, want, want_m = batch1

    def run(sel):
        return ops.encoder_view_u8hwc_ragged([imgs[i] for i in sel], [masks[i] for i in sel], size=32)
    everyone = list(range(len(imgs)))
    shuffled = list(everyone)
    random.Random(7).shuffle(shuffled)
    assert shuffled != everyone
    for sel in (everyone[::-1], shuffled, [0, 7, 4, 7, 2, 7]):  # (the last: one image three times -- one shared table)
        view, mview = run(sel)
        for k, i in enumerate(sel):
            assert torch.equal(view[k].cpu(), want[i]) and torch.equal(mview[k].cpu(), want_m[i]), (sel, k, i)
    for i in everyone:  # each image alone (B = 1)
        view, mview = run([i])
        assert view.shape[0] == 1 and torch.equal(view[0].cpu(), want[i]) and torch.equal(mview[0].cpu(), want_m[i]), i


# ------------------------------------------------------------------ 3. repeatable, on any stream
def test_repeatable_and_on_any_stream(ops, dev, batch1):
    imgs, masks, _, _ = batch1
    rb, wm = ops.RaggedBytes.pack(imgs), ops.RaggedBytes.pack(masks)
    v, m = ops.encoder_view_u8hwc_ragged(rb, wm, size=32)
    v2, m2 = ops.encoder_view_u8hwc_ragged(rb, wm, size=32)
    assert torch.equal(v2, v) and torch.equal(m2, m)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        vs, ms = ops.encoder_view_u8hwc_ragged(rb, wm, size=32)
    s.synchronize()
    assert torch.equal(vs, v) and torch.equal(ms, m)


# ------------------------------------------------------------------ 4. nothing outside the buffers is touched
def _bufs(host, imgs, masks, fill, plan=None):
    """Every buffer of the call exactly as long as the plan says: the two arenas (padding bytes: `fill`), the uploaded plan
    (on the 8-byte grid in both classes, as the header demands) and the two outputs."""
    B, size = int(host[1]), int(host[2])
    img_off, mask_off, (img_bytes, mask_bytes) = _offsets(host)
    return [GA.Buf("img", GA.IN, data=_arena_of(imgs, img_off, img_bytes, fill)), GA.Buf("mask", GA.IN, data=_arena_of(masks, mask_off, mask_bytes, fill)),
            GA.Buf("plan", GA.IN, data=host if plan is None else plan, grid=16),
            GA.Buf("view", GA.OUT, dtype=torch.float32, shape=(B, 3, size, size)), GA.Buf("mview", GA.OUT, dtype=torch.float32, shape=(B, 1, size, size))]


def _call(lib, host, expect=0):
    size = int(host[2])

    def call(a):
        rc = lib.curl_encoder_view_ragged_u8hwc(a.ptr("img"), a.nbytes("img"), a.ptr("mask"), a.nbytes("mask"), host.data_ptr(), a.ptr("plan"),
                                                a.nbytes("plan"), a.ptr("view"), a.ptr("mview"), size, 0, torch.cuda.current_stream(a.device).cuda_stream)
        assert rc == expect, lib.curl_last_error()
    return call


@pytest.mark.parametrize("cls", GA.CLASSES)
def test_nothing_outside_the_buffers_is_touched(dev, batch1, cls):
    """Through the C ABI with the two arenas, the uploaded plan and the two outputs inside one poisoned allocation
    (tests/guard_arena.py), at both alignment classes (the arenas on the 16-byte grid, and one byte past it): every band is
    intact, the arenas and the plan are unchanged, every output element is assigned and does not depend on the poison -- nor on
    what the padding between the images holds -- and is Pillow's."""
    from curl_amd import _lib
    lib = _lib.load()
    imgs, masks, want, want_m = batch1
    host = _host_plan(lib, _shapes(imgs), 32)
    img_off, mask_off, (img_bytes, mask_bytes) = _offsets(host)
    assert any(img_off[i] + imgs[i].numel() < img_off[i + 1] for i in range(9))     # there IS padding between images ...
    assert any(mask_off[i] + masks[i].numel() < mask_off[i + 1] for i in range(9))  # ... and between masks
    assert host.numel() * 4 == int(np.ascontiguousarray(host.numpy()[14:16]).view(np.int64)[0])
    for fill in (0x00, 0xC7):
        A = GA.run_both(_bufs(host, imgs, masks, fill), cls, dev, _call(lib, host))
        assert torch.equal(A.read("view").cpu(), want) and torch.equal(A.read("mview").cpu(), want_m), fill


# ------------------------------------------------------------------ 5. a foreign device plan writes nothing
def _run_once(bufs, cls, dev, call):
    """One poisoned run without run_both's demand that the outputs be assigned -> the arena, guards and inputs checked."""
    a = GA.Arena(bufs, cls, dev, GA.POISON_A)
    call(a)
    torch.cuda.synchronize(dev)
    a.check()
    return a


@pytest.mark.parametrize("cls", GA.CLASSES)
def test_a_foreign_device_plan_writes_nothing(dev, batch1, cls):
    """The host plan of batch 1 beside the uploaded plan of a list with the same B and sizes but one W changed (another hash),
    and beside a device plan of all zeros (no stamp): every workgroup returns at its first comparison -- both outputs keep their
    poison, the guards are intact."""
    from curl_amd import _lib
    lib = _lib.load()
    imgs, masks, _, _ = batch1
    shapes = _shapes(imgs)
    host = _host_plan(lib, shapes, 32)
    other = _host_plan(lib, [shapes[0], (56, 41, 3)] + shapes[2:], 32)
    assert other[0] == host[0] and other[1] == host[1] and not torch.equal(other[12:14], host[12:14])
    n = max(host.numel(), other.numel())
    foreign = torch.cat([other, torch.zeros(n - other.numel(), dtype=torch.int32)])  # (the call checks the length it is told)
    for plan in (foreign, torch.zeros(n, dtype=torch.int32)):
        a = _run_once(_bufs(host, imgs, masks, 0, plan=plan), cls, dev, _call(lib, host))
        for name in ("view", "mview"):
            assert bool(a.stale(name)[0].all()), name


# ------------------------------------------------------------------ 6. stale tables under a valid header stay inside
@pytest.mark.parametrize("cls", GA.CLASSES)
def test_stale_tables_under_a_valid_header_stay_inside(dev, batch1, cls):
    """The right header, hash and descriptors, every table word overwritten with those of 640x900 (a plan that went stale in
    place): wrong values at worst -- every index is clamped to the tile's window and to the image -- in [0, 1], the guards
    intact, nothing read from outside the images into a result (poison)."""
    from curl_amd import _lib
    lib = _lib.load()
    imgs, masks, want, _ = batch1
    host = _host_plan(lib, _shapes(imgs), 32)
    n = lib.curl_encoder_view_plan_bytes(640, 900, 32)
    single = torch.zeros(n // 4, dtype=torch.int32)
    assert lib.curl_encoder_view_plan(640, 900, 32, single.data_ptr(), n) == 0
    stale = host.clone()
    t0 = HEADER_WORDS + 10 * DESC_WORDS
    words = stale.numel() - t0
    stale[t0:] = single[16:].repeat(-(-words // (single.numel() - 16)))[:words]
    assert not torch.equal(stale[t0:], host[t0:]) and torch.equal(stale[:t0], host[:t0])
    A = GA.run_both(_bufs(host, imgs, masks, 0, plan=stale), cls, dev, _call(lib, host))
    v, m = A.read("view"), A.read("mview")
    assert bool(((v >= 0) & (v <= 1)).all()) and bool(((m == 0) | (m == 1)).all())
    assert not torch.equal(v.cpu(), want)  # (the tables were read: the values are not Pillow's)


# ------------------------------------------------------------------ 7. infer.enhance_many takes it
@pytest.mark.parametrize("arch", ["trispace", "curl"])
def test_enhance_many_makes_its_views_in_one_ragged_call(dev, arch, monkeypatch):
    """enhance_many(view="pil") with the single-image op taken away: the three files of tests/test_gpu_ragged.py's kind (12x20
    RGB, 33x65 RGBA, 40x64 grey) still come out as enhance(view="pil") writes each of them, byte for byte.  The net is that
    file's: its encoder recognises the views it is handed, so no batched convolution stands between the two routes."""
    import test_gpu_ragged as R
    from curl_amd import infer, ops
    imgs, masks = R._files()
    net = R._net(arch, dev)
    want = [infer.enhance(net, img, mask, dev, view="pil") for img, mask in zip(imgs, masks)]
    calls = []
    real = ops.encoder_view_u8hwc_ragged

    def gone(*a, **k):
        raise AssertionError("enhance_many made a view with the single-image op")

    def counted(*a, **k):
        calls.append(len(a[0]))
        return real(*a, **k)
    monkeypatch.setattr(ops, "encoder_view_u8hwc", gone)
    monkeypatch.setattr(ops, "encoder_view_u8hwc_ragged", counted)
    for batch_size, per_call in ((32, [3]), (2, [2, 1])):
        del calls[:]
        got = infer.enhance_many(net, imgs, masks, dev, view="pil", batch_size=batch_size)
        assert calls == per_call  # one ragged call per batch
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), (batch_size, g.shape)


def test_python_surface_checks_its_arguments(ops, dev, batch1):
    imgs, masks, _, _ = batch1
    three, m3 = imgs[:3], masks[:3]
    for bad in (m3[:2], [m3[0], m3[1], m3[1]], [m3[0], m3[1], three[2]], [m3[0], m3[1], m3[2].float()]):
        with pytest.raises(ValueError):
            ops.encoder_view_u8hwc_ragged(three, bad, size=32)
    with pytest.raises(RuntimeError):  # all inputs on one device
        ops.encoder_view_u8hwc_ragged(three, ops.RaggedBytes.pack([m.cpu() for m in m3]), size=32)
    rb = ops.RaggedBytes.pack(three)
    moved = ops.RaggedBytes(rb.arena, rb.shapes, [o + 16 for o in rb.offsets], rb.channels)
    with pytest.raises(ValueError, match="offsets"):  # arena offsets are the plan's
        ops.encoder_view_u8hwc_ragged(moved, None, size=32)
    strided = ops.RaggedBytes(torch.zeros(2 * rb.arena.numel(), dtype=torch.uint8, device=dev)[::2], rb.shapes, rb.offsets, rb.channels)
    with pytest.raises(ValueError, match="contiguous"):
        ops.encoder_view_u8hwc_ragged(strided, None, size=32)
    with pytest.raises(ValueError):  # beyond 64x at size 8: the library's code, raised
        ops.encoder_view_u8hwc_ragged([torch.zeros(513, 600, 3, dtype=torch.uint8, device=dev)], None, size=8)
    view, mview = ops.encoder_view_u8hwc_ragged(ops.RaggedBytes.pack([], dev), None, size=32)
    assert view.shape == (0, 3, 32, 32) and view.device.type == "cuda" and mview is None
    # host arrays go up with the call
    view, _ = ops.encoder_view_u8hwc_ragged([t.cpu().numpy() for t in three] + [imgs[3]], None, size=32)
    assert torch.equal(view, ops.encoder_view_u8hwc_ragged(imgs[:4], None, size=32)[0])
