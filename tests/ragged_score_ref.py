"""The reference values of the ragged score tests (tests/test_ragged_score_abi.py, tests/test_gpu_ragged_score.py): the masked
squared error of two byte images in numpy int64 and the PSNR of it in numpy float64.  Nothing of the library is used."""
import numpy as np

# (H, W) of the one batch both test files use, and what each shape reaches in the score kernels (flat tiles of 256 lanes: the
# dword class, H*W % 4 == 0, takes four pixels per lane, the byte class one)
SHAPES = [
    (1, 1),      # byte class, one pixel
    (1, 3),      # byte class
    (2, 2),      # dword class, one group
    (3, 85),     # byte class, one idle lane
    (1, 257),    # byte class, a second workgroup with one pixel
    (5, 103),    # byte class, ragged third workgroup
    (32, 32),    # dword class, exactly one full workgroup
    (4, 257),    # dword class, a second workgroup with one group
    (6, 512),    # dword class, tiles crossing rows
    (150, 148),  # 22 200 pixels: 0 against 255 is 4 330 665 000 > 2^32
]


def sse_ref(a, b, mask=None):
    """a, b: uint8 [H,W,3]; mask: uint8 [H,W] or None (every pixel) -> (sum over the kept pixels and the 3 channels of
    (a - b)^2, the number of kept pixels), Python ints."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    keep = np.ones(a.shape[:2], dtype=np.int64) if mask is None else (np.asarray(mask) != 0).astype(np.int64)
    return int((keep[..., None] * (a - b) ** 2).sum()), int(keep.sum())


def psnr_ref(sse, n):
    """10 * log10(255^2 * 3 n / sse) in float64, element-wise: nan for n = 0 (0 / 0), inf for sse = 0 with n > 0."""
    sse, n = np.asarray(sse, dtype=np.float64), np.asarray(n, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(255.0 ** 2 * 3.0 * n / sse)
