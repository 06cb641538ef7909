"""The foreground-aware byte entries between guard bands (tests/guard_arena.py run_both): every buffer exactly as long as
include/curl_hip_fg.h says, on the 16-byte grid (the dword kernels, where the shape admits them) and one byte off it (the byte
kernels), RGB and RGBA, one dword-path and one byte-path shape per tile kind -- bands untouched, inputs untouched, no output
byte left unwritten (dead wavefronts and dead workgroups store their white themselves), nothing depending on the poison."""
import pytest
import torch

from guard_arena import IN, OUT, WORK, Buf, CLASSES, run_both

pytestmark = pytest.mark.gpu

B = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(g, H, W, channels):
    """image bytes, and a mask with every kind of wavefront: image 0 a random mix of 0 / 1 / 128 / 255 right of a zero left
    half, image 1 all zero"""
    img = torch.randint(0, 256, (B, H, W, channels), generator=g, dtype=torch.int32).to(torch.uint8)
    fg = torch.tensor([0, 1, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (B, H, W), generator=g)]
    fg[0, :, : W // 2] = 0
    fg[1] = 0
    return img, fg


def _ok(lib, rc):
    assert rc == 0, (rc, lib.curl_last_error().decode("utf-8", "replace"))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("nc,shape", [(126, (5, 520)), (126, (5, 515)), (35, (6, 512)), (35, (5, 103))])
def test_trispace_foreground_guard_bands(dev, nc, shape, channels, cls):
    from curl_amd import _lib, ops
    lib = _lib.load()
    H, W = shape
    g = torch.Generator().manual_seed(nc + H * W + channels)
    img, fg = _inputs(g, H, W, channels)
    c = torch.randn(B, 3, 3, nc, generator=g) * 0.2
    bufs = [Buf("img", IN, img), Buf("coeffs", IN, c, grid=8 if nc == 126 else None), Buf("fg_mask", IN, fg),
            Buf("out", OUT, shape=(B, H, W, 3), dtype=torch.uint8)]
    s = torch.cuda.current_stream().cuda_stream
    A = run_both(bufs, cls, dev, lambda A: _ok(lib, lib.curl_trispace_fwd_fg_u8hwc(A.ptr("img"), channels, A.ptr("coeffs"), A.ptr("fg_mask"),
                                                                                  A.ptr("out"), B, H, W, nc, 0, s)))
    assert torch.equal(A.read("out"), ops.trispace_forward_u8hwc(img[..., :3].contiguous().to(dev), c.to(dev), fg.to(dev)))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("shape", [(6, 512), (5, 103)])
def test_layer_foreground_guard_bands(dev, shape, channels, cls):
    from curl_amd import _lib, ops
    lib = _lib.load()
    H, W = shape
    g = torch.Generator().manual_seed(H * W + channels)
    img, fg = _inputs(g, H, W, channels)
    L, R, Hk = (torch.randn(B, n, generator=g) * 0.1 for n in (48, 48, 64))
    bufs = [Buf("img", IN, img), Buf("rawL", IN, L), Buf("rawR", IN, R), Buf("rawH", IN, Hk), Buf("fg_mask", IN, fg),
            Buf("out", OUT, shape=(B, H, W, 3), dtype=torch.uint8), Buf("reg", OUT, shape=(B,), dtype=torch.float32),
            Buf("workspace", WORK, nbytes=lib.curl_workspace_bytes(B, 160), grid=16)]
    s = torch.cuda.current_stream().cuda_stream
    A = run_both(bufs, cls, dev, lambda A: _ok(lib, lib.curl_layer_fwd_fg_u8hwc(
        A.ptr("img"), channels, A.ptr("rawL"), A.ptr("rawR"), A.ptr("rawH"), A.ptr("fg_mask"), A.ptr("out"), A.ptr("reg"),
        A.ptr("workspace"), A.nbytes("workspace"), B, H, W, 16, 16, 16, 0, s)))
    want, reg = ops.curl_layer_forward_u8hwc(img[..., :3].contiguous().to(dev), None, L.to(dev), R.to(dev), Hk.to(dev), fg.to(dev))
    assert torch.equal(A.read("out"), want) and torch.equal(A.read("reg"), reg)
