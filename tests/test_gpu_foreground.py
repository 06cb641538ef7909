"""The foreground-aware byte entries on the GPU (curl_trispace_fwd_fg_u8hwc, curl_layer_fwd_fg_u8hwc; include/curl_hip_fg.h):
every output byte against the existing entry on img[..., :3].contiguous() with white_mask = fg_mask, torch.equal.

B = 2 everywhere.  Image 1's mask is all zero: every workgroup of it is dead.  Image 0 takes four masks in turn, laid out on
the kernel's own wavefronts (64 lanes x 4 pixels on the dword path, 64 pixels on the byte path; row tiles never cross a row):
  a  the left part zero: whole wavefronts dead beside live ones of the same workgroup
  b  zero, but for a byte of value 1 at one wavefront's first pixel and one at the next wavefront's last pixel
  c  a random mix of 0, 1, 128, 255
  d  all 255
Shapes are the smallest that reach each path (the tables of the issue):
  126 coefficients (row tiles)   (3, 1024) dword, one workgroup of four wavefronts per row
                                 (5, 520)  dword, a 192-lane workgroup whose last wavefront has two valid lanes
                                 (5, 515)  byte, W % 4 != 0, three workgroups per row
  flat tiles (the other seven counts, the layer)
                                 (6, 512)  dword, three 1024-pixel tiles that cross rows
                                 (5, 103)  byte, a ragged last workgroup"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW_SHAPES = [(3, 1024), (5, 520), (5, 515)]
FLAT_SHAPES = [(6, 512), (5, 103)]
FLAT_COUNTS = (35, 56, 20, 21, 10, 6, 4)
# all eight counts at one shape; 126, 35 and one lower order per variable count (56: 5 variables, 10: 3) everywhere
TRI_CASES = [(126, s) for s in ROW_SHAPES] + [(nc, FLAT_SHAPES[0]) for nc in FLAT_COUNTS] + [(nc, FLAT_SHAPES[1]) for nc in (35, 56, 10)]
LAYER_CASES = [("even", s) for s in FLAT_SHAPES] + [("uneven", FLAT_SHAPES[1])]
KNOTS = {"even": (48, 48, 64), "uneven": (47, 48, 62)}  # K = 16; uneven: the last curves hold 15 and 14 knots (CURL_K_UNEVEN)


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


def _wave_spans(H, W, rows):
    """(workgroup, lo, hi) of every wavefront of one image in launch order: its workgroup's number and its flat pixel range"""
    vec = 4 if (W % 4 == 0 if rows else (H * W) % 4 == 0) else 1
    px = 64 * vec
    if not rows:
        return [(lo // (4 * px), lo, min(lo + px, H * W)) for lo in range(0, H * W, px)]
    units = W // vec
    best_t, best_waste = 64, None
    for t in (64, 128, 192, 256):  # host_api.inc row_blocks: the fewest idle lanes, the larger block on a tie
        waste = -(-units // t) * t - units
        if best_waste is None or waste <= best_waste:
            best_t, best_waste = t, waste
    segs = -(-units // best_t)
    spans = []
    for r in range(H):
        for lane0 in range(0, segs * best_t, 64):
            if lane0 < units:
                spans.append((r * segs + lane0 // best_t, r * W + lane0 * vec, r * W + min((lane0 + 64) * vec, W)))
    return spans


# mask a: the columns left of this are zero -- a whole number of wavefronts of the row's (the tile's) first workgroup
LEFT = {(3, 1024): 512, (5, 520): 256, (5, 515): 128, (6, 512): 256, (5, 103): 64}


def _masks(g, H, W, rows):
    """name -> fg_mask uint8 [2,H,W]; image 1 all zero"""
    spans = _wave_spans(H, W, rows)
    assert len(spans) >= 4
    a = torch.full((H, W), 255, dtype=torch.uint8)
    a[:, :LEFT[(H, W)]] = 0
    a = a.view(-1)
    dead = {}
    for wg, lo, hi in spans:
        dead.setdefault(wg, set()).add(not bool(a[lo:hi].any()))
    assert any(v == {True, False} for v in dead.values()), "mask a: no workgroup with a dead wavefront beside a live one"
    b = torch.zeros(H * W, dtype=torch.uint8)
    assert spans[0][0] == spans[1][0] == spans[2][0]  # the two marked wavefronts share a workgroup with a dead one
    b[spans[1][1]] = 1
    b[spans[2][2] - 1] = 1
    c = torch.tensor([0, 1, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (H * W,), generator=g)]
    d = torch.full((H * W,), 255, dtype=torch.uint8)
    return {k: torch.stack([m.view(H, W), torch.zeros(H, W, dtype=torch.uint8)]) for k, m in (("a", a), ("b", b), ("c", c), ("d", d))}


def _rgba(rgb, g):
    return torch.cat([rgb, _rand_u8(g, *rgb.shape[:3], 1)], dim=3)


def _misaligned(t):
    """The same bytes in a tensor whose storage starts one byte past an allocation boundary (tests/test_gpu_parity.py)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 4 != 0 and view.is_contiguous()
    return view


def _check_all(new, old, rgb, masks, g, dev):
    """new(img, fg, b) against old(rgb, fg) for every mask (b: None for the batch, or the one image the call is given): RGB,
    two RGBA images that differ in alpha only, a repeated call, image alone against image in the batch, and the image / the
    mask one byte off the dword grid."""
    for name, fg in masks.items():
        fg = fg.to(dev)
        want = old(rgb, fg)
        got = new(rgb, fg, None)
        assert torch.equal(got, want), (name, int((got != want).sum()))
        assert bool((got[1] == 255).all()) and bool((got[0][fg[0] == 0] == 255).all()), name
        a1, a2 = _rgba(rgb.cpu(), g).to(dev), _rgba(rgb.cpu(), g).to(dev)
        g1, g2 = new(a1, fg, None), new(a2, fg, None)
        assert torch.equal(g1, g2) and torch.equal(g1, want), name
        assert torch.equal(new(rgb, fg, None), got), name  # a repeated call
        for b in range(2):
            assert torch.equal(new(a1[b:b + 1], fg[b:b + 1], b)[0], want[b]), (name, b)
        assert torch.equal(new(_misaligned(rgb), fg, None), want) and torch.equal(new(a1, _misaligned(fg), None), want), name


def _pick(t, b):
    return t if b is None else t[b:b + 1]


@pytest.mark.parametrize("nc,shape", TRI_CASES)
def test_trispace_foreground_equals_the_existing_entry(ops, dev, nc, shape):
    H, W = shape
    g = torch.Generator().manual_seed(1000 * nc + H * W)
    rgb = _rand_u8(g, 2, H, W, 3).to(dev)
    coeffs = (torch.randn(2, 3, 3, nc, generator=g) * 0.2).to(dev)
    _check_all(lambda x, m, b: ops.trispace_foreground_u8hwc(x, _pick(coeffs, b), m), lambda x, m: ops.trispace_forward_u8hwc(x, coeffs, m),
               rgb, _masks(g, H, W, nc == 126), g, dev)


def _layer_inputs(g, kind, dev):
    nl, nr, nh = KNOTS[kind]
    return [(torch.randn(2, n, generator=g) * 0.1).to(dev) for n in (nl, nr, nh)]


@pytest.mark.parametrize("kind,shape", LAYER_CASES)
def test_layer_foreground_equals_the_existing_entry(ops, dev, kind, shape):
    H, W = shape
    g = torch.Generator().manual_seed(H * W + len(kind))
    rgb = _rand_u8(g, 2, H, W, 3).to(dev)
    L, R, Hk = _layer_inputs(g, kind, dev)
    masks = _masks(g, H, W, False)
    _check_all(lambda x, m, b: ops.curl_layer_foreground_u8hwc(x, _pick(L, b), _pick(R, b), _pick(Hk, b), m)[0],
               lambda x, m: ops.curl_layer_forward_u8hwc(x, None, L, R, Hk, m)[0], rgb, masks, g, dev)
    fg = masks["a"].to(dev)
    assert torch.equal(ops.curl_layer_foreground_u8hwc(rgb, L, R, Hk, fg)[1], ops.curl_layer_forward_u8hwc(rgb, None, L, R, Hk, fg)[1])


def _packed_knots(n, curves):
    """n parameters over `curves` curves as the C ABI takes them (CURL_K_UNEVEN: the last curve's count in the high half)."""
    K = -(-n // curves)
    last = n - (curves - 1) * K
    return K if last == K else K | (last << 16)


@pytest.mark.parametrize("kind", ["even", "uneven"])
@pytest.mark.parametrize("channels", [3, 4])
def test_layer_reg_and_workspace_rows_are_the_existing_entrys(dev, kind, channels):
    """Both entries through the C ABI on workspaces of their own (zeroed: the rows have words nobody writes): reg and every
    word of the workspace, bit for bit."""
    from curl_amd import _lib
    lib = _lib.load()
    H, W = 6, 512
    g = torch.Generator().manual_seed(77 + channels)
    rgb = _rand_u8(g, 2, H, W, 3)
    img = (rgb if channels == 3 else _rgba(rgb, g)).to(dev)
    rgb = rgb.to(dev)
    fg = _masks(g, H, W, False)["c"].to(dev)
    L, R, Hk = _layer_inputs(g, kind, dev)
    K = [_packed_knots(n, c) for n, c in zip(KNOTS[kind], (3, 3, 4))]
    nbytes = lib.curl_workspace_bytes(2, sum(KNOTS[kind]))
    s = torch.cuda.current_stream().cuda_stream
    res = []
    for entry in ("old", "new"):
        ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        reg = torch.zeros(2, dtype=torch.float32, device=dev)
        out = torch.empty(2, H, W, 3, dtype=torch.uint8, device=dev)
        if entry == "old":
            rc = lib.curl_layer_fwd_u8hwc(rgb.data_ptr(), 0, 0, L.data_ptr(), R.data_ptr(), Hk.data_ptr(), fg.data_ptr(), out.data_ptr(),
                                          reg.data_ptr(), ws.data_ptr(), nbytes, 2, H, W, K[0], K[1], K[2], 0, s)
        else:
            rc = lib.curl_layer_fwd_fg_u8hwc(img.data_ptr(), channels, L.data_ptr(), R.data_ptr(), Hk.data_ptr(), fg.data_ptr(),
                                             out.data_ptr(), reg.data_ptr(), ws.data_ptr(), nbytes, 2, H, W, K[0], K[1], K[2], 0, s)
        assert rc == 0, lib.curl_last_error()
        res.append((out, reg.view(torch.int32), ws))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert bool(res[1][2].any())


def test_python_surface_checks_its_arguments(ops, dev):
    img = torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=dev)
    fg = torch.zeros(1, 8, 8, dtype=torch.uint8, device=dev)
    c = torch.zeros(1, 3, 3, 126, device=dev)
    k = [torch.zeros(1, n, device=dev) for n in (48, 48, 64)]
    assert bool((ops.trispace_foreground_u8hwc(img, c, fg) == 255).all())
    for bad_img, bad_fg in ((img.float(), fg), (img[..., :2], fg), (img[0], fg), (img, None), (img, fg[:, :7]), (img, fg.float()),
                            (img[:, :0], fg[:, :0]), (img[:0], fg[:0])):
        with pytest.raises(ValueError):
            ops.trispace_foreground_u8hwc(bad_img, c, bad_fg)
        with pytest.raises(ValueError):
            ops.curl_layer_foreground_u8hwc(bad_img, *k, bad_fg)
    with pytest.raises(RuntimeError):
        ops.trispace_foreground_u8hwc(img.cpu(), c, fg)
    with pytest.raises(RuntimeError):
        ops.curl_layer_foreground_u8hwc(img, *k, fg.cpu())
    with pytest.raises(ValueError):
        ops.trispace_foreground_u8hwc(img, c[..., :125], fg)


# ------------------------------------------------------------------ one direct pin: the oracle's chain
def _close_to_the_oracle(got, want):
    d = np.abs(got.cpu().numpy().astype(int) - want.astype(int))
    print("max grey-level difference", d.max(), "share of differing bytes", (d > 0).mean())
    assert d.max() <= 1 and (d > 0).mean() < 0.01


@pytest.mark.parametrize("nc", [126, 35])
def test_trispace_foreground_against_the_oracle(ops, dev, nc):
    """The inputs of test_gpu_parity.py::test_trispace_u8hwc_fused_file_edge at (2, 36, 52), its `white` as fg_mask, under its
    criterion: within one grey level of the oracle's chain on < 1 % of the bytes."""
    import curl_oracle as O
    B, H, W = 2, 36, 52
    g = torch.Generator().manual_seed(H * W + nc)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    white = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=g)
    white[:, : H // 3] = 0
    white[:, -H // 3:] = 255
    coeffs = torch.randn(B, 3, 3, nc, generator=g) * 0.2
    got = ops.trispace_foreground_u8hwc(img.to(dev), coeffs.to(dev), white.to(dev))
    xo = torch.stack([O.u8hwc_to_f32chw(img[b].numpy()) for b in range(B)])
    ro = O.trispace_residual(xo, coeffs[:, 0], coeffs[:, 1], coeffs[:, 2], spatial=(nc == 126))
    yo = O.white_background(O.generate_image(xo, ro), (white.float() / 255).unsqueeze(1))
    _close_to_the_oracle(got, np.stack([O.f32chw_to_u8hwc(yo[b]) for b in range(B)]))


def test_layer_foreground_against_the_oracle(ops, dev):
    """The inputs of test_gpu_parity.py::test_curl_layer_u8hwc_fused_file_edge at (2, 36, 52) (the entry has no layer mask)."""
    import curl_oracle as O
    B, H, W = 2, 36, 52
    g = torch.Generator().manual_seed(H * W)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    white = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=g)
    L, R = torch.randn(B, 48, generator=g) * 0.1, torch.randn(B, 48, generator=g) * 0.1
    Hk = torch.randn(B, 64, generator=g) * 0.1
    got, _ = ops.curl_layer_foreground_u8hwc(img.to(dev), L.to(dev), R.to(dev), Hk.to(dev), white.to(dev))
    xo = torch.stack([O.u8hwc_to_f32chw(img[b].numpy()) for b in range(B)])
    yo, _ = O.curl_layer(xo, torch.ones(B, 1, H, W), L, R, Hk)
    yo = O.white_background(yo, (white.float() / 255).unsqueeze(1))
    _close_to_the_oracle(got, np.stack([O.f32chw_to_u8hwc(yo[b]) for b in range(B)]))


# ------------------------------------------------------------------ infer.enhance(foreground=True)
class _TinyBackbone(torch.nn.Module):
    """A pooled-feature encoder with a `.classifier` slot (the heads of TriSpaceRegNet and GCURLNet go there)."""

    def __init__(self, width=16, n_out=None):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, width, 3, stride=2, padding=1)
        self.classifier = torch.nn.Identity() if n_out is None else torch.nn.Linear(width, n_out)

    def forward(self, x):
        return self.classifier(torch.tanh(self.conv(x)).mean((2, 3)))


@pytest.fixture(scope="module")
def photo():
    """1000 x 1500 random bytes (RGBA) and a disk mask with a soft rim: whole wavefronts outside, whole wavefronts inside."""
    g = torch.Generator().manual_seed(11)
    rgba = _rand_u8(g, 1000, 1500, 4).numpy()
    yy, xx = np.mgrid[0:1000, 0:1500]
    r = np.hypot(yy - 500, xx - 750)
    return rgba, np.clip((450 - r) * 16, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("arch", ["trispace", "curl"])
def test_enhance_foreground_is_enhance(dev, photo, arch):
    """enhance(foreground=True) == enhance(foreground=False), byte for byte: both architectures, RGB and RGBA arrays, both
    view= routes."""
    from curl_amd import infer, model as M
    rgba, mask = photo
    torch.manual_seed(5)
    if arch == "trispace":
        net = M.TriSpaceRegNet(polynomial_order=4, spatial=True, is_train=False, backbone=_TinyBackbone(), feature_width=16).to(dev).eval()
    else:
        net = M.GCURLNet(backbone=_TinyBackbone(n_out=160), encoder_size=320).to(dev).eval()
    rgb = np.ascontiguousarray(rgba[..., :3])
    for view in ("float", "pil"):
        want = infer.enhance(net, rgb, mask, dev, view=view)
        assert want.shape == (1000, 1500, 3) and (want[mask == 0] == 255).all() and (want != 255).any()
        for img in (rgb, rgba):
            got = infer.enhance(net, img, mask, dev, view=view, foreground=True)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (view, img.shape)
