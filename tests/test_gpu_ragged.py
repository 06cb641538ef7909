"""The ragged byte entries on the GPU (curl_trispace_fwd_ragged_u8hwc, curl_layer_fwd_ragged_u8hwc;
include/curl_hip_ragged.h): a batch of images of different sizes in one launch per class, every output byte against the
single-image entry on that image alone, torch.equal.

One mixed batch of nine images, the smallest shapes that reach every path:
  (1,1,3)     smaller than a lane group, byte class
  (3,5,3)     byte class, a ragged tile
  (4,8,4)     RGBA, dword class, one partial wavefront
  (7,9,4)     RGBA, byte class
  (12,20,3)   dword class
  (2,1028,3)  dword class; row tiles (126): 257 groups per row = several segments, ONE live lane in the last
  (3,1500,4)  RGBA, dword class, flat tiles of two workgroups; row tiles: 375 groups per row = several segments
  (33,65,3)   byte class, flat tiles of nine workgroups
  (40,64,3)   dword class, flat tiles of three workgroups"""
import numpy as np
import pytest
import torch

import guard_arena as GA

pytestmark = pytest.mark.gpu

BATCH = [(1, 1, 3), (3, 5, 3), (4, 8, 4), (7, 9, 4), (12, 20, 3), (2, 1028, 3), (3, 1500, 4), (33, 65, 3), (40, 64, 3)]
KNOTS = (48, 48, 64)  # K = 16 per curve


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


def _mask(g, H, W):
    """tests/test_gpu_parity.py's pattern -- a third zeros, a third 255, random between -- from three rows on; else random."""
    m = _rand_u8(g, H, W)
    if H >= 3:
        m[: H // 3] = 0
        m[-H // 3:] = 255
    return m


@pytest.fixture(scope="module")
def batch(dev):
    """The nine images and masks on the device, and the operators' inputs for B = 9 (made once, never changed)."""
    g = torch.Generator().manual_seed(2024)
    imgs = [_rand_u8(g, h, w, c).to(dev) for h, w, c in BATCH]
    masks = [_mask(g, h, w).to(dev) for h, w, _ in BATCH]
    coeffs = {nc: (torch.randn(len(BATCH), 3, 3, nc, generator=g) * 0.2).to(dev) for nc in (126, 35, 56, 10)}
    knots = [(torch.randn(len(BATCH), n, generator=g) * 0.1).to(dev) for n in KNOTS]
    return imgs, masks, coeffs, knots


def _rgb(img):
    return img[None, ..., :3].contiguous()


def _tri_alone(ops, img, coeffs, i, mask):
    return ops.trispace_forward_u8hwc(_rgb(img), coeffs[i:i + 1], None if mask is None else mask[None])[0]


def _layer_alone(ops, img, knots, i, mask):
    out, reg = ops.curl_layer_forward_u8hwc(_rgb(img), None, *(k[i:i + 1] for k in knots), None if mask is None else mask[None])
    return out[0], reg


# ------------------------------------------------------------------ 1. bytes equal the sibling's, image by image
@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("nc", [126, 35, 56, 10])
def test_trispace_ragged_equals_the_single_image_entry(ops, dev, batch, nc, with_masks):
    imgs, masks, coeffs, _ = batch
    out = ops.trispace_forward_u8hwc_ragged(imgs, coeffs[nc], masks if with_masks else None)
    assert len(out) == len(BATCH) and out.channels == [3] * len(BATCH) and out.shapes == [(h, w) for h, w, _ in BATCH]
    for i, img in enumerate(imgs):
        want = _tri_alone(ops, img, coeffs[nc], i, masks[i] if with_masks else None)
        got = out.image(i)
        assert got.shape == want.shape and torch.equal(got, want), (i, BATCH[i], int((got != want).sum()))


@pytest.mark.parametrize("with_masks", [False, True])
def test_layer_ragged_equals_the_single_image_entry(ops, dev, batch, with_masks):
    imgs, masks, _, knots = batch
    out, reg = ops.curl_layer_forward_u8hwc_ragged(imgs, *knots, masks if with_masks else None)
    assert reg.shape == (len(BATCH),)
    for i, img in enumerate(imgs):
        want, want_reg = _layer_alone(ops, img, knots, i, masks[i] if with_masks else None)
        got = out.image(i)
        assert torch.equal(got, want), (i, BATCH[i], int((got != want).sum()))
        assert torch.equal(reg[i:i + 1].view(torch.int32), want_reg.view(torch.int32)), i


# ------------------------------------------------------------------ 2. order and company do not matter
@pytest.mark.parametrize("op", ["126", "35", "layer"])
def test_order_and_company_do_not_matter(ops, dev, batch, op):
    imgs, masks, coeffs, knots = batch

    def run(sel):
        ii, mm = [imgs[i] for i in sel], [masks[i] for i in sel]
        idx = torch.tensor(sel, device=dev)
        if op == "layer":
            return ops.curl_layer_forward_u8hwc_ragged(ii, *(k[idx] for k in knots), mm)[0]
        return ops.trispace_forward_u8hwc_ragged(ii, coeffs[int(op)][idx], mm)
    everyone = list(range(len(BATCH)))
    first = run(everyone)
    again = run(everyone)
    assert all(torch.equal(a, b) for a, b in zip(first.images(), again.images()))  # a repeated call
    backwards = run(everyone[::-1])
    for k, i in enumerate(everyone[::-1]):
        assert torch.equal(backwards.image(k), first.image(i)), (k, i)
    alone = run([4])
    assert len(alone) == 1 and torch.equal(alone.image(0), first.image(4))
    # the arena form: a packed RaggedBytes in, the same bytes out
    packed = ops.RaggedBytes.pack(imgs), ops.RaggedBytes.pack(masks)
    if op == "layer":
        out = ops.curl_layer_forward_u8hwc_ragged(packed[0], *knots, packed[1])[0]
    else:
        out = ops.trispace_forward_u8hwc_ragged(packed[0], coeffs[int(op)], packed[1])
    assert all(torch.equal(a, b) for a, b in zip(out.images(), first.images()))


# ------------------------------------------------------------------ 3. nothing outside the images is touched
def _plan_words(lib, shapes, op, has_mask=1):
    B = len(shapes)
    hs, ws, cs = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(3))
    nbytes = lib.curl_ragged_plan_bytes(B, op)
    host = torch.zeros(nbytes // 4, dtype=torch.int32)
    rc = lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, op, host.data_ptr(), nbytes)
    assert rc == 0, lib.curl_last_error()
    return host


def _offsets(host, B):
    d = host.numpy()[32:32 + 16 * B].reshape(B, 16)
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


@pytest.mark.parametrize("op", ["126", "35", "layer"])
def test_nothing_outside_the_images_is_touched(dev, batch, op):
    """Both entries through the C ABI with the three arenas and the uploaded plan inside one poisoned allocation
    (tests/guard_arena.py): every band and the padding between the output images still hold the poison, the image arena,
    the mask arena and the plan are unchanged, every output byte is written and does not depend on the poison."""
    from curl_amd import _lib
    lib = _lib.load()
    imgs, masks, coeffs, knots = batch
    B = len(BATCH)
    nc = 0 if op == "layer" else int(op)
    host = _plan_words(lib, BATCH, nc)
    off, (img_bytes, mask_bytes, out_bytes) = _offsets(host, B)
    ends = [int(off[i, 2]) + h * w * 3 for i, (h, w, _) in enumerate(BATCH)]
    padding = [(ends[i], int(off[i + 1, 2])) for i in range(B - 1) if ends[i] < int(off[i + 1, 2])]
    assert padding and ends[-1] == out_bytes
    bufs = [GA.Buf("img", GA.IN, data=_arena_of(imgs, off[:, 0], img_bytes)), GA.Buf("mask", GA.IN, data=_arena_of(masks, off[:, 1], mask_bytes)),
            GA.Buf("plan", GA.IN, data=host, grid=16), GA.Buf("out", GA.OUT, nbytes=out_bytes, keep=padding)]
    if op == "layer":
        bufs += [GA.Buf(n, GA.IN, data=k.cpu()) for n, k in zip(("L", "R", "H"), knots)]
        bufs += [GA.Buf("reg", GA.OUT, shape=(B,), dtype=torch.float32),
                 GA.Buf("ws", GA.WORK, nbytes=lib.curl_workspace_bytes(B, sum(KNOTS)), grid=16)]
    else:
        bufs.append(GA.Buf("coeffs", GA.IN, data=coeffs[nc].cpu(), grid=16))

    def call(a):
        s = torch.cuda.current_stream().cuda_stream
        if op == "layer":
            rc = lib.curl_layer_fwd_ragged_u8hwc(a.ptr("img"), img_bytes, a.ptr("L"), a.ptr("R"), a.ptr("H"), a.ptr("mask"), mask_bytes,
                                                 a.ptr("out"), out_bytes, a.ptr("reg"), a.ptr("ws"), a.nbytes("ws"), host.data_ptr(),
                                                 a.ptr("plan"), a.nbytes("plan"), 16, 16, 16, 0, s)
        else:
            rc = lib.curl_trispace_fwd_ragged_u8hwc(a.ptr("img"), img_bytes, a.ptr("coeffs"), a.ptr("mask"), mask_bytes, a.ptr("out"),
                                                    out_bytes, host.data_ptr(), a.ptr("plan"), a.nbytes("plan"), nc, 0, s)
        assert rc == 0, lib.curl_last_error()
    arena = GA.run_both(bufs, "16", dev, call)
    # ... and the bytes are the ones of the ops route
    got = arena.read("out")
    ops_out = _ops_route(op, batch)
    for i, (h, w, _) in enumerate(BATCH):
        assert torch.equal(got[int(off[i, 2]):ends[i]].view(h, w, 3), ops_out.image(i)), i


def _ops_route(op, batch):
    from curl_amd import ops
    imgs, masks, coeffs, knots = batch
    if op == "layer":
        return ops.curl_layer_forward_u8hwc_ragged(imgs, *knots, masks)[0]
    return ops.trispace_forward_u8hwc_ragged(imgs, coeffs[int(op)], masks)


# ------------------------------------------------------------------ 4. a foreign plan writes nothing
@pytest.mark.parametrize("op", ["126", "35", "layer"])
def test_a_foreign_plan_writes_nothing(dev, batch, op):
    """The device plan of the same shapes in another order (another hash) beside the host plan of the call: every workgroup
    returns at its first comparison, the out arena keeps its poison whatever the entry returns."""
    from curl_amd import _lib
    lib = _lib.load()
    imgs, masks, coeffs, knots = batch
    B = len(BATCH)
    nc = 0 if op == "layer" else int(op)
    host, foreign = _plan_words(lib, BATCH, nc), _plan_words(lib, BATCH[::-1], nc)
    assert host.numel() == foreign.numel() and not torch.equal(host[18:20], foreign[18:20])
    off, (img_bytes, mask_bytes, out_bytes) = _offsets(host, B)
    img, mask = _arena_of(imgs, off[:, 0], img_bytes).to(dev), _arena_of(masks, off[:, 1], mask_bytes).to(dev)
    out = torch.full((out_bytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    plan_dev = foreign.to(dev)
    s = torch.cuda.current_stream().cuda_stream
    if op == "layer":
        reg = torch.empty(B, dtype=torch.float32, device=dev)
        nbytes = lib.curl_workspace_bytes(B, sum(KNOTS))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        lib.curl_layer_fwd_ragged_u8hwc(img.data_ptr(), img_bytes, *(k.data_ptr() for k in knots), mask.data_ptr(), mask_bytes,
                                        out.data_ptr(), out_bytes, reg.data_ptr(), ws.data_ptr(), nbytes, host.data_ptr(),
                                        plan_dev.data_ptr(), plan_dev.numel() * 4, 16, 16, 16, 0, s)
    else:
        lib.curl_trispace_fwd_ragged_u8hwc(img.data_ptr(), img_bytes, coeffs[nc].data_ptr(), mask.data_ptr(), mask_bytes, out.data_ptr(),
                                           out_bytes, host.data_ptr(), plan_dev.data_ptr(), plan_dev.numel() * 4, nc, 0, s)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert torch.equal(plan_dev.cpu(), foreign)


# ------------------------------------------------------------------ 5. one direct pin: the oracle's chain
EDGE_SHAPES = [(36, 52), (33, 65), (7, 9)]  # tests/test_gpu_parity.py's file-edge shapes, one image each


def _edge_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in EDGE_SHAPES]
    whites = []
    for h, w in EDGE_SHAPES:
        m = torch.randint(0, 256, (h, w), dtype=torch.uint8, generator=g)
        m[: h // 3] = 0
        m[-h // 3:] = 255
        whites.append(m)
    return g, imgs, whites


def _pooled(gots, wants):
    d = np.concatenate([np.abs(g.cpu().numpy().astype(int) - w.astype(int)).reshape(-1) for g, w in zip(gots, wants)])
    print("max grey-level difference", d.max(), "share of differing bytes", (d > 0).mean())
    return d


@pytest.mark.parametrize("nc", [126, 35])
def test_trispace_ragged_against_the_oracle(ops, dev, nc):
    """test_trispace_u8hwc_fused_file_edge's chain and criterion, pooled over the batch: no byte differs by more than 1 and
    fewer than 1 % differ."""
    import curl_oracle as O
    g, imgs, whites = _edge_inputs(1000 + nc)
    coeffs = torch.randn(len(imgs), 3, 3, nc, generator=g) * 0.2
    for wm in (None, whites):
        out = ops.trispace_forward_u8hwc_ragged([t.to(dev) for t in imgs], coeffs.to(dev), None if wm is None else [m.to(dev) for m in wm])
        wants = []
        for i, img in enumerate(imgs):
            xo = O.u8hwc_to_f32chw(img.numpy())[None]
            c = coeffs[i:i + 1]
            yo = O.generate_image(xo, O.trispace_residual(xo, c[:, 0], c[:, 1], c[:, 2], spatial=(nc == 126)))
            if wm is not None:
                yo = O.white_background(yo, (wm[i].float() / 255)[None, None])
            wants.append(O.f32chw_to_u8hwc(yo[0]))
        d = _pooled(out.images(), wants)
        assert d.max() <= 1 and (d > 0).mean() < 0.01


def test_layer_ragged_against_the_oracle(ops, dev):
    """test_curl_layer_u8hwc_fused_file_edge's chain (no layer mask) and criterion, pooled over the batch."""
    import curl_oracle as O
    g, imgs, whites = _edge_inputs(77)
    B = len(imgs)
    L, R, Hk = torch.randn(B, 48, generator=g) * 0.1, torch.randn(B, 48, generator=g) * 0.1, torch.randn(B, 64, generator=g) * 0.1
    for wm in (None, whites):
        out, _ = ops.curl_layer_forward_u8hwc_ragged([t.to(dev) for t in imgs], L.to(dev), R.to(dev), Hk.to(dev),
                                                     None if wm is None else [m.to(dev) for m in wm])
        wants = []
        for i, img in enumerate(imgs):
            xo = O.u8hwc_to_f32chw(img.numpy())[None]
            h, w = EDGE_SHAPES[i]
            yo, _ = O.curl_layer(xo, torch.ones(1, 1, h, w), L[i:i + 1], R[i:i + 1], Hk[i:i + 1])
            if wm is not None:
                yo = O.white_background(yo, (wm[i].float() / 255)[None, None])
            wants.append(O.f32chw_to_u8hwc(yo[0]))
        d = _pooled(out.images(), wants)
        assert d.max() <= 1 and (d > 0).mean() < 0.01


# ------------------------------------------------------------------ the Python surface's own checks
def test_python_surface_checks_its_arguments(ops, dev, batch):
    imgs, masks, coeffs, knots = batch
    three, m3 = imgs[:3], masks[:3]
    c, k = coeffs[126][:3], [t[:3] for t in knots]
    for bad in (m3[:2], [m3[0], m3[1], m3[1]], [m3[0], m3[1], three[2]], [m3[0], m3[1], m3[2].float()]):
        with pytest.raises(ValueError):
            ops.trispace_forward_u8hwc_ragged(three, c, bad)
        with pytest.raises(ValueError):
            ops.curl_layer_forward_u8hwc_ragged(three, *k, bad)
    with pytest.raises(ValueError):
        ops.trispace_forward_u8hwc_ragged(three[:2] + [three[2][:0]], c)
    with pytest.raises(ValueError):
        ops.trispace_forward_u8hwc_ragged(three, coeffs[126][:2])  # one coefficient row per image
    with pytest.raises(ValueError):
        ops.curl_layer_forward_u8hwc_ragged(three, k[0][:2], k[1], k[2])
    with pytest.raises(RuntimeError):
        ops.trispace_forward_u8hwc_ragged(three, c.cpu())
    with pytest.raises(RuntimeError):
        ops.trispace_forward_u8hwc_ragged(three, c, ops.RaggedBytes.pack([m.cpu() for m in m3]))
    assert len(ops.trispace_forward_u8hwc_ragged([], c[:0])) == 0
    # host arrays go up with the call; image(i)[None] is what the encoder view takes
    out = ops.trispace_forward_u8hwc_ragged([t.cpu().numpy() for t in three], c, [m.cpu() for m in m3])
    assert all(torch.equal(a, b) for a, b in zip(out.images(), ops.trispace_forward_u8hwc_ragged(three, c, m3).images()))
    rb = ops.RaggedBytes.pack(imgs, dev)
    view, _ = ops.encoder_view_u8hwc(rb.image(8)[None])
    assert torch.equal(view, ops.encoder_view_u8hwc(imgs[8][None])[0])


# ------------------------------------------------------------------ 6. infer.enhance_many and the folder CLI
class _TinyBackbone(torch.nn.Module):
    """A pooled-feature encoder with a `.classifier` slot (the heads of TriSpaceRegNet and GCURLNet go there)."""

    def __init__(self, width=16, n_out=None):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, width, 3, stride=2, padding=1)
        self.classifier = torch.nn.Identity() if n_out is None else torch.nn.Linear(width, n_out)

    def forward(self, x):
        return self.classifier(torch.tanh(self.conv(x)).mean((2, 3)))


FILES = [(12, 20, 3), (33, 65, 4), (40, 64, 3)]  # at least 8 pixels on the short side: the view's limits


def _files():
    g = torch.Generator().manual_seed(99)
    imgs = [_rand_u8(g, h, w, c).numpy() for h, w, c in FILES]
    imgs[2] = np.repeat(imgs[2][..., :1], 3, axis=2)  # a grey image, as both CLIs repeat a one-channel file
    masks = [_mask(g, h, w).numpy() for h, w, _ in FILES]
    return imgs, masks


def _net(arch, dev):
    """A net whose encoder's output is GIVEN per image: generate_coefficients / predict_knots recognise the 320 x 320 view
    they are handed (each view is made from one image alone on both routes, so it is the same tensor bit for bit) and return
    that image's fixed row -- no batched convolution stands between enhance and enhance_many."""
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
def test_enhance_many_is_enhance_of_each_image(dev, arch):
    from curl_amd import infer
    imgs, masks = _files()
    net = _net(arch, dev)
    for view in ("pil", "float"):
        want = [infer.enhance(net, img, mask, dev, view=view) for img, mask in zip(imgs, masks)]
        for batch_size in (32, 2):
            got = infer.enhance_many(net, imgs, masks, dev, view=view, batch_size=batch_size)
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), (view, batch_size, g.shape)
    assert infer.enhance_many(net, [], [], dev) == []
    with pytest.raises(ValueError):
        infer.enhance_many(net, imgs, masks[:2], dev)


def test_infer_dir_writes_the_single_image_cli_files(dev, tmp_path, monkeypatch):
    """python -m curl_amd.infer_dir on a folder of three PNGs (RGB, RGBA and grey) == three runs of python -m curl_amd.infer."""
    from PIL import Image
    from curl_amd import infer, infer_dir
    imgs, masks = _files()
    for d in ("in", "masks", "single", "many"):
        (tmp_path / d).mkdir()
    names = ["a", "b", "c"]
    for name, img, mask in zip(names, imgs, masks):
        Image.fromarray(img[..., 0] if name == "c" else img).save(tmp_path / "in" / f"{name}.png")  # c: an 'L' file
        Image.fromarray(mask).save(tmp_path / "masks" / f"{name}.png")
    net = _net("trispace", dev)
    monkeypatch.setattr(infer, "build_net", lambda *a, **k: net)
    monkeypatch.setattr(infer_dir, "build_net", lambda *a, **k: net)
    for name in names:
        infer.infer(["--img_path", str(tmp_path / "in" / f"{name}.png"), "--mask_path", str(tmp_path / "masks" / f"{name}.png"),
                     "--model_file", "random", "--out_path", str(tmp_path / "single" / f"{name}.png"), "--encoder_view", "pil"])
    assert infer_dir.main(["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random",
                           "--out_dir", str(tmp_path / "many"), "--encoder_view", "pil", "--batch_size", "2"]) == 0
    for name in names:
        a, b = np.asarray(Image.open(tmp_path / "single" / f"{name}.png")), np.asarray(Image.open(tmp_path / "many" / f"{name}.png"))
        assert a.shape == b.shape and np.array_equal(a, b), name
    (tmp_path / "masks" / "b.png").unlink()
    with pytest.raises(FileNotFoundError, match="b.png"):
        infer_dir.main(["--img_dir", str(tmp_path / "in"), "--mask_dir", str(tmp_path / "masks"), "--model_file", "random",
                        "--out_dir", str(tmp_path / "many")])
