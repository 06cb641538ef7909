"""The foreground-aware ragged byte entries on the GPU (curl_trispace_fwd_ragged_fg_u8hwc, curl_layer_fwd_ragged_fg_u8hwc;
include/curl_hip_ragged_fg.h): every output byte against the merged ragged entry on the same arenas, torch.equal.

One batch of seven images, the smallest shapes that reach every path:
  (1,1,3)     an image smaller than a lane group
  (3,1024,3)  row tiles (126), dword path
  (5,520,4)   row tiles, dword path, RGBA
  (5,515,3)   row tiles, byte path
  (2,1028,3)  a row's last workgroup with ONE storing lane
  (6,512,4)   flat dword tiles that cross rows
  (5,103,3)   the flat byte path, a ragged last workgroup

Five kinds of mask, laid out on the kernel's own wavefronts (their spans are read from the plan: header words 7 and 9 for the
block sizes, the descriptors' groups per row and workgroups per row):
  a  the left part zero: whole waves dead beside live ones
  b  all zero but a byte of value 1 at one wave's first pixel and one at the next wave's last pixel
  c  a random mix of 0 / 1 / 128 / 255
  d  all 255
  z  all zero
In call r = 0..4 image j takes kind (j + r) mod 5: every image meets every kind, every call holds a dead image and a full one."""
import numpy as np
import pytest
import torch

import guard_arena as GA

pytestmark = pytest.mark.gpu

BATCH = [(1, 1, 3), (3, 1024, 3), (5, 520, 4), (5, 515, 3), (2, 1028, 3), (6, 512, 4), (5, 103, 3)]
KINDS = "abcdz"
KNOTS = (48, 48, 64)  # K = 16 per curve
OPS = {"126": 126, "35": 35, "56": 56 | (3 << 16), "10": 10 | (2 << 16), "layer": 0}  # the entries' num_coeffs; 0: the layer
HEADER_WORDS, DESC_WORDS = 32, 16


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


# ------------------------------------------------------------------ the plan, and the wavefronts it gives every image
def _plan_words(lib, shapes, op, has_mask=1):
    B = len(shapes)
    hs, ws, cs = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(3))
    nbytes = lib.curl_ragged_plan_bytes(B, op)
    host = torch.zeros(nbytes // 4, dtype=torch.int32)
    rc = lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, op, host.data_ptr(), nbytes)
    assert rc == 0, lib.curl_last_error()
    return host


def _wave_spans(host):
    """image index -> (class: 0 dword / 1 byte, row-tiled?, [workgroup: [wave: (first pixel, one past the last) of its storing
    lanes, None for a wave without any]]), from the plan alone.  A lane's group is chunk * threads + lane (flat tiles) or
    row * units + seg * threads + lane (row tiles; it stores iff seg * threads + lane < units); a group is 4 pixels in the
    dword class and 1 in the byte class."""
    w = host.numpy()
    B, n_dword = int(w[1]), int(w[5])
    desc = w[HEADER_WORDS:HEADER_WORDS + DESC_WORDS * B].reshape(B, DESC_WORDS)
    out = {}
    for cls, (lo, hi) in enumerate(((0, n_dword), (n_dword, B))):
        threads, vec = int(w[7 + 2 * cls]), 4 if cls == 0 else 1
        for d in desc[lo:hi]:
            index, n, units, segs, tiles = (int(d[k]) for k in (1, 5, 6, 7, 8))
            wgs = []
            for chunk in range(tiles):
                if units:
                    row, seg = divmod(chunk, segs)
                    first, stop, g0 = seg * threads, min(seg * threads + threads, units), row * units
                else:
                    first, stop, g0 = chunk * threads, min(chunk * threads + threads, n), 0
                waves = []
                for k in range(threads // 64):
                    a, b = first + 64 * k, min(first + 64 * k + 64, stop)
                    waves.append(((g0 + a) * vec, (g0 + b) * vec) if a < b else None)
                wgs.append(waves)
            out[index] = (cls, units > 0, wgs)
    assert sorted(out) == list(range(B))
    return out


def _mask_of(kind, h, w, wgs, g):
    m = torch.zeros(h * w, dtype=torch.uint8)
    if kind == "a":  # the columns of the image's first wave, when the first workgroup has a second one: that wave is dead in
        first = [s for s in wgs[0] if s]  # every workgroup that starts a row (or a flat tile at a row's start)
        c = first[0][1] if len(first) > 1 and first[0][1] < w else w // 2
        m = m.view(h, w)
        m[:, c:] = 255
    elif kind == "b":
        waves = [s for wg in wgs for s in wg if s]
        k = (len(waves) - 1) // 2
        m[waves[k][0]] = 1
        m[waves[min(k + 1, len(waves) - 1)][1] - 1] = 1
    elif kind == "c":
        m = torch.tensor([0, 1, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (h * w,), generator=g)]
    elif kind == "d":
        m[:] = 255
    return m.view(h, w).contiguous()


def _tiling(op):
    return "rows" if op == "126" else "flat"


@pytest.fixture(scope="module")
def spans():
    """tiling -> the wave spans of BATCH: 'rows' from the plan of the 126-coefficient model, 'flat' from every other
    operator's (they tile alike: held here).  The plan functions make no HIP call."""
    from curl_amd import _lib
    lib = _lib.load()
    out = {"rows": _wave_spans(_plan_words(lib, BATCH, 126)), "flat": _wave_spans(_plan_words(lib, BATCH, 35))}
    for name in ("56", "10", "layer"):
        assert _wave_spans(_plan_words(lib, BATCH, OPS[name])) == out["flat"], name
    return out


@pytest.fixture(scope="module")
def masks_cpu(spans):
    """tiling -> kind -> the seven masks (host tensors, made once, never changed)."""
    g = torch.Generator().manual_seed(515)
    return {t: {kind: [_mask_of(kind, h, w, spans[t][j][2], g) for j, (h, w, _) in enumerate(BATCH)] for kind in KINDS} for t in spans}


def _kinds_of_call(r):
    return [KINDS[(j + r) % 5] for j in range(len(BATCH))]


def _dead(mask, span):
    return not bool(mask.reshape(-1)[span[0]:span[1]].any())


def test_the_masks_reach_what_they_are_for(spans, masks_cpu):
    """Conditions on the inputs, not on the code under test: in each of the four paths kind `a` gives a workgroup with a dead
    wave beside a live one, kind `b` an image with fully dead workgroups beside live ones, and the batch holds a row whose
    last workgroup has ONE storing lane."""
    for tiling, rows in (("rows", True), ("flat", False)):
        for cls in (0, 1):
            images = [j for j in range(len(BATCH)) if spans[tiling][j][0] == cls]
            assert images and all(spans[tiling][j][1] == rows for j in images), (tiling, cls)
            mixed = dead_beside_live = 0
            for j in images:
                wgs = spans[tiling][j][2]
                for kind in "ab":
                    m = masks_cpu[tiling][kind][j]
                    verdicts = [[_dead(m, s) for s in wg if s] for wg in wgs]
                    if kind == "a":
                        mixed += sum(1 for v in verdicts if any(v) and not all(v))
                    else:
                        dead_beside_live += any(all(v) for v in verdicts) and any(not all(v) for v in verdicts)
            assert mixed >= 1, (tiling, cls, "kind a: no workgroup with a dead wave beside a live one")
            assert dead_beside_live >= 1, (tiling, cls, "kind b: no image with dead workgroups beside live ones")
    cls, rows, wgs = spans["rows"][4]  # (2,1028,3): 257 groups per row
    assert cls == 0 and rows and [s for s in wgs[-1] if s] == [(2 * 1028 - 4, 2 * 1028)]
    # every call holds a dead image and a full one, every image meets every kind
    assert all({"d", "z"} <= set(_kinds_of_call(r)) for r in range(5))
    assert all({_kinds_of_call(r)[j] for r in range(5)} == set(KINDS) for j in range(len(BATCH)))


@pytest.fixture(scope="module")
def batch(dev, masks_cpu):
    """The seven images, the masks of the five calls per tiling and the operators' inputs for B = 7, on the device (made once,
    never changed)."""
    g = torch.Generator().manual_seed(2025)
    imgs = [_rand_u8(g, h, w, c).to(dev) for h, w, c in BATCH]
    masks = {t: [[masks_cpu[t][kind][j].to(dev) for j, kind in enumerate(_kinds_of_call(r))] for r in range(5)] for t in masks_cpu}
    coeffs = {nc: (torch.randn(len(BATCH), 3, 3, nc, generator=g) * 0.2).to(dev) for nc in (126, 35, 56, 10)}
    knots = [(torch.randn(len(BATCH), n, generator=g) * 0.1).to(dev) for n in KNOTS]
    return imgs, masks, coeffs, knots


def _plain(ops, op, imgs, masks, coeffs, knots, sel=None):
    """The merged ragged entry -> (RaggedBytes, reg or None); sel: the images' rows of the operator's inputs."""
    idx = slice(None) if sel is None else torch.tensor(sel, device=imgs[0].device if isinstance(imgs, list) else imgs.device)
    if op == "layer":
        return ops.curl_layer_forward_u8hwc_ragged(imgs, *(k[idx] for k in knots), masks)
    return ops.trispace_forward_u8hwc_ragged(imgs, coeffs[int(op)][idx], masks), None


def _fg(ops, op, imgs, masks, coeffs, knots, sel=None):
    idx = slice(None) if sel is None else torch.tensor(sel, device=imgs[0].device if isinstance(imgs, list) else imgs.device)
    if op == "layer":
        return ops.curl_layer_foreground_u8hwc_ragged(imgs, *(k[idx] for k in knots), masks)
    return ops.trispace_foreground_u8hwc_ragged(imgs, coeffs[int(op)][idx], masks), None


def _same_images(got, want):
    assert len(got) == len(want) and got.shapes == want.shapes and got.offsets == want.offsets and got.channels == want.channels
    for i, (a, b) in enumerate(zip(got.images(), want.images())):
        assert a.shape == b.shape and torch.equal(a, b), (i, got.shapes[i], int((a != b).sum()))


# ------------------------------------------------------------------ 1. the bytes are the merged ragged entry's
@pytest.mark.parametrize("op", list(OPS))
def test_foreground_equals_the_ragged_entry(ops, dev, batch, op):
    imgs, masks, coeffs, knots = batch
    for r in range(5):
        m = masks[_tiling(op)][r]
        want, want_reg = _plain(ops, op, imgs, m, coeffs, knots)
        got, reg = _fg(ops, op, imgs, m, coeffs, knots)
        assert got.shapes == [(h, w) for h, w, _ in BATCH] and got.channels == [3] * len(BATCH)
        _same_images(got, want)
        if op == "layer":
            assert reg.shape == (len(BATCH),) and torch.equal(reg.view(torch.int32), want_reg.view(torch.int32)), r
        z = _kinds_of_call(r).index("z")
        assert bool((got.image(z) == 255).all())  # the dead image is white


# ------------------------------------------------------------------ 2. order and company do not matter
@pytest.mark.parametrize("op", ["126", "35", "layer"])
def test_order_and_company_do_not_matter(ops, dev, batch, op):
    imgs, masks, coeffs, knots = batch
    m = masks[_tiling(op)][1]

    def run(sel):
        return _fg(ops, op, [imgs[i] for i in sel], [m[i] for i in sel], coeffs, knots, sel)[0]
    everyone = list(range(len(BATCH)))
    first = run(everyone)
    _same_images(first, _plain(ops, op, imgs, m, coeffs, knots)[0])
    again = run(everyone)
    assert all(torch.equal(a, b) for a, b in zip(first.images(), again.images()))  # a repeated call
    backwards = run(everyone[::-1])
    for k, i in enumerate(everyone[::-1]):
        assert torch.equal(backwards.image(k), first.image(i)), (k, i)
    for i in (1, 3):  # one image alone (a tiling of its own: the block size of its rows alone)
        alone = run([i])
        assert len(alone) == 1 and torch.equal(alone.image(0), first.image(i)), i
    # the arena form: packed RaggedBytes in, the same bytes out
    packed = _fg(ops, op, ops.RaggedBytes.pack(imgs), ops.RaggedBytes.pack(m), coeffs, knots)[0]
    _same_images(packed, first)


# ------------------------------------------------------------------ 3. what need not be read is not part of the result
@pytest.mark.parametrize("op", ["126", "35", "layer"])
def test_alpha_and_the_pixels_under_a_zero_mask_do_not_matter(ops, dev, batch, op):
    imgs, masks, coeffs, knots = batch
    g = torch.Generator().manual_seed(7)
    for r in range(5):
        m = masks[_tiling(op)][r]
        want = _fg(ops, op, imgs, m, coeffs, knots)[0]
        other_alpha = [torch.cat([t[..., :3], _rand_u8(g, *t.shape[:2], 1).to(dev)], 2) if t.shape[2] == 4 else t for t in imgs]
        assert any(not torch.equal(a, b) for a, b in zip(other_alpha, imgs))
        _same_images(_fg(ops, op, other_alpha, m, coeffs, knots)[0], want)
        # other bytes wherever the mask is 0 (whole dead waves and single pixels of live ones alike)
        junk = [torch.where((mk == 0)[..., None], _rand_u8(g, *t.shape).to(dev), t) for t, mk in zip(imgs, m)]
        assert any(not torch.equal(a, b) for a, b in zip(junk, imgs))
        _same_images(_fg(ops, op, junk, m, coeffs, knots)[0], want)


# ------------------------------------------------------------------ 4. nothing outside the images is touched
def _offsets(host, B):
    d = host.numpy()[HEADER_WORDS:HEADER_WORDS + DESC_WORDS * B].reshape(B, DESC_WORDS)
    off = np.ascontiguousarray(d[:, 10:16]).view(np.int64)
    by_image = np.empty_like(off)
    by_image[d[:, 1]] = off
    sizes = np.ascontiguousarray(host.numpy()[12:18]).view(np.int64)
    return by_image, [int(v) for v in sizes]


def _arena_of(parts, offsets, nbytes):
    a = torch.zeros(nbytes, dtype=torch.uint8)
    for t, o in zip(parts, offsets):
        a[o:o + t.numel()] = t.cpu().reshape(-1)
    return a


def _call(lib, op, fg, ptr, sizes, host, plan_ptr, plan_bytes, nc, extra):
    """Either entry through the C ABI; ptr(name) -> device address."""
    s = torch.cuda.current_stream().cuda_stream
    img_bytes, mask_bytes, out_bytes = sizes
    if op == "layer":
        fn = lib.curl_layer_fwd_ragged_fg_u8hwc if fg else lib.curl_layer_fwd_ragged_u8hwc
        return fn(ptr("img"), img_bytes, ptr("L"), ptr("R"), ptr("H"), ptr("mask"), mask_bytes, ptr("out"), out_bytes, ptr("reg"),
                  ptr("ws"), extra, host.data_ptr(), plan_ptr, plan_bytes, 16, 16, 16, 0, s)
    fn = lib.curl_trispace_fwd_ragged_fg_u8hwc if fg else lib.curl_trispace_fwd_ragged_u8hwc
    return fn(ptr("img"), img_bytes, ptr("coeffs"), ptr("mask"), mask_bytes, ptr("out"), out_bytes, host.data_ptr(), plan_ptr,
              plan_bytes, nc, 0, s)


@pytest.mark.parametrize("op", ["126", "35", "layer"])
def test_nothing_outside_the_images_is_touched(dev, batch, op):
    """Both entries through the C ABI with the three arenas and the uploaded plan inside one poisoned allocation
    (tests/guard_arena.py): every band and the padding between the output images still hold the poison, the image arena, the
    mask arena and the plan are unchanged, every output byte is written and does not depend on the poison -- and the
    foreground entry leaves the sibling's bits in the out arena, in reg and in the workspace."""
    from curl_amd import _lib
    lib = _lib.load()
    imgs, masks, coeffs, knots = batch
    m = masks[_tiling(op)][0]
    B, nc = len(BATCH), OPS[op]
    host = _plan_words(lib, BATCH, nc)
    off, sizes = _offsets(host, B)
    out_bytes = sizes[2]
    ends = [int(off[i, 2]) + h * w * 3 for i, (h, w, _) in enumerate(BATCH)]
    padding = [(ends[i], int(off[i + 1, 2])) for i in range(B - 1) if ends[i] < int(off[i + 1, 2])]
    assert padding and ends[-1] == out_bytes
    bufs = [GA.Buf("img", GA.IN, data=_arena_of(imgs, off[:, 0], sizes[0])), GA.Buf("mask", GA.IN, data=_arena_of(m, off[:, 1], sizes[1])),
            GA.Buf("plan", GA.IN, data=host, grid=16), GA.Buf("out", GA.OUT, nbytes=out_bytes, keep=padding)]
    if op == "layer":
        bufs += [GA.Buf(n, GA.IN, data=k.cpu()) for n, k in zip(("L", "R", "H"), knots)]
        bufs += [GA.Buf("reg", GA.OUT, shape=(B,), dtype=torch.float32),
                 GA.Buf("ws", GA.WORK, nbytes=lib.curl_workspace_bytes(B, sum(KNOTS)), grid=16)]
    else:
        bufs.append(GA.Buf("coeffs", GA.IN, data=coeffs[int(op)].cpu(), grid=16))
    arenas = {}
    for fg in (False, True):
        def call(a):
            rc = _call(lib, op, fg, a.ptr, sizes, host, a.ptr("plan"), a.nbytes("plan"), nc, a.nbytes("ws"))
            assert rc == 0, lib.curl_last_error()
        arenas[fg] = GA.run_both(bufs, "16", dev, call)
    assert torch.equal(arenas[True].read("out"), arenas[False].read("out"))  # (the padding: the same poison in both)
    if op == "layer":
        assert torch.equal(arenas[True].read("reg").view(torch.int32), arenas[False].read("reg").view(torch.int32))
        assert torch.equal(arenas[True].read("ws"), arenas[False].read("ws"))  # the workspace rows, bit for bit
    # ... and the bytes are the ones of the ops route
    from curl_amd import ops
    got, ops_out = arenas[True].read("out"), _fg(ops, op, imgs, m, coeffs, knots)[0]
    for i, (h, w, _) in enumerate(BATCH):
        assert torch.equal(got[int(off[i, 2]):ends[i]].view(h, w, 3), ops_out.image(i)), i


# ------------------------------------------------------------------ 5. a foreign plan writes nothing
@pytest.mark.parametrize("op", ["126", "35", "layer"])
def test_a_foreign_plan_writes_nothing(dev, batch, op):
    """The device plan of the same shapes in another order (another hash) beside the host plan of the call: every workgroup
    returns at its first comparison, the out arena keeps its fill whatever the entry returns."""
    from curl_amd import _lib
    lib = _lib.load()
    imgs, masks, coeffs, knots = batch
    m = masks[_tiling(op)][0]
    B, nc = len(BATCH), OPS[op]
    host, foreign = _plan_words(lib, BATCH, nc), _plan_words(lib, BATCH[::-1], nc)
    assert host.numel() == foreign.numel() and not torch.equal(host[18:20], foreign[18:20])
    off, sizes = _offsets(host, B)
    t = {"img": _arena_of(imgs, off[:, 0], sizes[0]).to(dev), "mask": _arena_of(m, off[:, 1], sizes[1]).to(dev),
         "out": torch.full((sizes[2] + 4096,), 0xA5, dtype=torch.uint8, device=dev)}
    plan_dev = foreign.to(dev)
    nbytes = 0
    if op == "layer":
        nbytes = lib.curl_workspace_bytes(B, sum(KNOTS))
        t.update(L=knots[0], R=knots[1], H=knots[2], reg=torch.empty(B, dtype=torch.float32, device=dev),
                 ws=torch.empty(nbytes // 4, dtype=torch.float32, device=dev))
    else:
        t["coeffs"] = coeffs[int(op)]
    _call(lib, op, True, lambda name: t[name].data_ptr(), sizes, host, plan_dev.data_ptr(), plan_dev.numel() * 4, nc, nbytes)
    torch.cuda.synchronize()
    assert bool((t["out"] == 0xA5).all())
    assert torch.equal(plan_dev.cpu(), foreign)


# ------------------------------------------------------------------ the Python surface's own checks on a device
def test_python_surface_checks_its_arguments(ops, dev, batch):
    imgs, masks, coeffs, knots = batch
    m = masks["rows"][2]
    three, m3 = imgs[:3], m[:3]
    c, k = coeffs[126][:3], [t[:3] for t in knots]
    for bad in (None, m3[:2], [m3[0], m3[1], m3[1]], [m3[0], m3[1], three[2]], [m3[0], m3[1], m3[2].float()]):
        with pytest.raises(ValueError):
            ops.trispace_foreground_u8hwc_ragged(three, c, bad)
        with pytest.raises(ValueError):
            ops.curl_layer_foreground_u8hwc_ragged(three, *k, bad)
    with pytest.raises(ValueError):
        ops.trispace_foreground_u8hwc_ragged(three, coeffs[126][:2], m3)  # one coefficient row per image
    with pytest.raises(RuntimeError):
        ops.trispace_foreground_u8hwc_ragged(three, c, ops.RaggedBytes.pack([t.cpu() for t in m3]))
    assert len(ops.trispace_foreground_u8hwc_ragged([], c[:0], [])) == 0
    # host arrays go up with the call; the cached plan of the shape list is the plain call's
    out = ops.trispace_foreground_u8hwc_ragged([t.cpu().numpy() for t in three], c, [t.cpu() for t in m3])
    n = len(ops._ragged_plans)
    _same_images(out, ops.trispace_forward_u8hwc_ragged(three, c, m3))
    assert len(ops._ragged_plans) == n


# ------------------------------------------------------------------ 6. infer.enhance_many_foreground and the folder CLI
class _TinyBackbone(torch.nn.Module):
    """A pooled-feature encoder with a `.classifier` slot (the heads of TriSpaceRegNet and GCURLNet go there)."""

    def __init__(self, width=16, n_out=None):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, width, 3, stride=2, padding=1)
        self.classifier = torch.nn.Identity() if n_out is None else torch.nn.Linear(width, n_out)

    def forward(self, x):
        return self.classifier(torch.tanh(self.conv(x)).mean((2, 3)))


FILES = [(12, 20, 3), (33, 65, 4), (40, 64, 3)]  # at least 8 pixels on the short side: the view's limits


def _file_mask(g, H, W):
    """A third zeros, a third 255, random between."""
    m = _rand_u8(g, H, W)
    m[: H // 3] = 0
    m[-H // 3:] = 255
    return m


def _files():
    g = torch.Generator().manual_seed(99)
    imgs = [_rand_u8(g, h, w, c).numpy() for h, w, c in FILES]
    imgs[2] = np.repeat(imgs[2][..., :1], 3, axis=2)  # a grey image, as both CLIs repeat a one-channel file
    masks = [_file_mask(g, h, w).numpy() for h, w, _ in FILES]
    return imgs, masks


def _net(arch, dev):
    """A net whose encoder's output is GIVEN per image: generate_coefficients / predict_knots recognise the 320 x 320 view
    they are handed (each view is made from one image alone on every route, so it is the same tensor bit for bit) and return
    that image's fixed row -- no batched convolution stands between the routes that are compared."""
    from curl_amd import infer, model as M, ops
    imgs, masks = _files()
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(6)
    if arch == "trispace":
        net = M.TriSpaceRegNet(polynomial_order=4, spatial=True, is_train=False, backbone=_TinyBackbone(), feature_width=16).to(dev).eval()
        rows = (torch.randn(len(FILES), 3, 3, 126, generator=g) * 0.2).to(dev)
    else:
        net = M.GCURLNet(backbone=_TinyBackbone(n_out=160), encoder_size=320).to(dev).eval()
        rows = (torch.randn(len(FILES), 160, generator=g) * 0.1).to(dev)
    known = []  # (the encoder's input, row): both view= routes
    for i, (img, mask) in enumerate(zip(imgs, masks)):
        rgb = torch.from_numpy(np.ascontiguousarray(img[..., :3])).to(dev)[None]
        white = torch.from_numpy(mask).to(dev)[None]
        pil = ops.encoder_view_u8hwc(rgb, white)
        flt = infer.encoder_view(ops.u8hwc_to_f32chw(rgb), white[:, None].float() / 255.0)
        for small, msmall in (pil, flt):
            known.append(((small, msmall) if arch == "trispace" else (small * msmall,), i))

    def row_of(*given):
        out = []
        for b in range(given[0].shape[0]):
            hits = {i for ref, i in known if all(torch.equal(x[b], r[0]) for x, r in zip(given, ref))}
            assert len(hits) == 1, "the encoder was handed a view of none of the test's images"
            out.append(rows[hits.pop()])
        return torch.stack(out)
    if arch == "trispace":
        def generate_coefficients(img, mask):
            c = row_of(img, mask)
            return c[:, 0], c[:, 1], c[:, 2]
        net.generate_coefficients = generate_coefficients
    else:
        net.predict_knots = lambda x: row_of(x)
    return net


@pytest.mark.parametrize("arch", ["trispace", "curl"])
def test_enhance_many_foreground_is_enhance_many(dev, arch):
    from curl_amd import infer
    imgs, masks = _files()
    net = _net(arch, dev)
    for view in ("pil", "float"):
        for batch_size in (1, 3):
            want = infer.enhance_many(net, imgs, masks, dev, view=view, batch_size=batch_size)
            got = infer.enhance_many_foreground(net, imgs, masks, dev, view=view, batch_size=batch_size)
            assert len(got) == len(want) == len(FILES)
            for g, w in zip(got, want):
                assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), (view, batch_size, g.shape)
    assert infer.enhance_many_foreground(net, [], [], dev) == []
    with pytest.raises(ValueError):
        infer.enhance_many_foreground(net, imgs, masks[:2], dev)


def test_infer_dir_foreground_masks_writes_the_same_files(dev, tmp_path, monkeypatch):
    """python -m curl_amd.infer_dir --foreground_masks on a folder of three PNGs (RGB, RGBA and grey) writes the files of the
    run without the flag, byte for byte."""
    from PIL import Image
    from curl_amd import infer_dir
    imgs, masks = _files()
    for d in ("in", "masks", "plain", "fg"):
        (tmp_path / d).mkdir()
    names = ["a", "b", "c"]
    for name, img, mask in zip(names, imgs, masks):
        Image.fromarray(img[..., 0] if name == "c" else img).save(tmp_path / "in" / f"{name}.png")  # c: an 'L' file
        Image.fromarray(mask).save(tmp_path / "masks" / f"{name}.png")
    net = _net("trispace", dev)
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: net)
    used = []
    for name in ("enhance_many", "enhance_many_foreground"):
        def spy(*a, _fn=getattr(infer_dir, name), _name=name, **k):
            used.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(infer_dir, name, spy)
    base = ["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random", "--encoder_view", "pil"]
    for batch_size in ("1", "3"):
        assert infer_dir.main(base + ["--out_dir", str(tmp_path / "plain"), "--batch_size", batch_size]) == 0
        assert infer_dir.main(base + ["--out_dir", str(tmp_path / "fg"), "--batch_size", batch_size, "--foreground_masks"]) == 0
        for name in names:
            a, b = (tmp_path / "plain" / f"{name}.png").read_bytes(), (tmp_path / "fg" / f"{name}.png").read_bytes()
            assert a == b and len(a) > 0, (name, batch_size)
            assert np.asarray(Image.open(tmp_path / "fg" / f"{name}.png")).shape == imgs[names.index(name)].shape[:2] + (3,)
    assert set(used) == {"enhance_many", "enhance_many_foreground"}
