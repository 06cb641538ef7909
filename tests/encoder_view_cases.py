"""The cases of the encoder-view tests (tests/test_encoder_view_*.py, tests/test_gpu_encoder_view.py) and of their fixture
(tests/golden/encoder_view.npz, written from Pillow by tests/golden/make_golden_encoder_view.py), and the Python restatement
of the two torchvision size rules and of Pillow's coefficient routine that the C code is held to.

The fixture stores the inputs of the small cases beside Pillow's outputs.  The three large inputs (641x481, 97x1003 and
1000x1500: 1.9 MB of bytes, more than a committed file may hold) come from the integer formulas below, in the script and in
the tests alike; only their expected views are stored."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_view.npz")

# name -> (H, W, size, B, channels); the smallest shapes at which each mechanism can go wrong
CASES = {
    "40x56": (40, 56, 32, 1, 3),            # landscape: the crop on x
    "56x40": (56, 40, 32, 1, 3),            # portrait: the crop on y
    "32x33": (32, 33, 32, 1, 3),            # crop margin 1 -> 0 (round half to even); y is an identity axis
    "32x35": (32, 35, 32, 1, 3),            # crop margin 3 -> 2
    "37x37_b2": (37, 37, 32, 2, 3),         # pitch 111 B: no row is dword aligned, nor the second image's base
    "20x27": (20, 27, 32, 1, 3),            # up-scaling, ksize 3
    "641x481": (641, 481, 32, 1, 3),        # 15x down-scaling
    "97x1003_s16": (97, 1003, 16, 1, 3),    # extreme aspect, long crop margin
    "1000x1500_s320": (1000, 1500, 320, 1, 3),  # the default size
    "rgba_40x56": (40, 56, 32, 1, 4),       # alpha is dropped
    "sparse_56x40": (56, 40, 32, 1, 3),     # a mask of isolated dim pixels: `> 0` sits on a rounded byte
}
FORMULA_INPUTS = ("641x481", "97x1003_s16", "1000x1500_s320")


def formula_image(B, H, W, C, seed=0):
    """Bytes with content at every frequency (an integer hash of the coordinates over a smooth ramp): uint8 [B,H,W,C]."""
    b, y, x, c = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64),
                             np.arange(C, dtype=np.int64), indexing="ij")
    h = (x * 73 + y * 151 + c * 89 + b * 57 + seed * 31 + (x * y) % 251) ^ ((x * x * 3 + y * y * 5 + c * 7) >> 3)
    ramp = (x * 100) // max(W - 1, 1) + (y * 60) // max(H - 1, 1)
    v = (h * 2654435761 >> 7) % 61 + ramp + (h & 31)  # 0 .. 251
    return np.where((x + 2 * y) % 23 == 0, 255 * ((x + y) & 1), v).astype(np.uint8)  # and pixels of pure black / white


def formula_mask(B, H, W, sparse=False, seed=0):
    """uint8 [B,H,W]: a solid foreground block with a ragged edge plus isolated pixels of 1, 2, 40 and 255 (sparse: only
    those)."""
    b, y, x = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    dots = ((x * 7 + y * 13 + b * 5 + seed) % 29 == 0) & ((x + 3 * y) % 5 != 1)
    vals = np.choose((x + y + b) % 4, [1, 2, 40, 255])
    m = np.where(dots, vals, 0)
    if not sparse:
        block = (x > W // 4 + (y * 3) % 5) & (x < (3 * W) // 4) & (y > H // 5) & (y < (4 * H) // 5 + (x * 7) % 3)
        m = np.where(block, 255, m)
    return m.astype(np.uint8)


def inputs(name, golden=None):
    """(img uint8 [B,H,W,C], mask uint8 [B,H,W]) of a case: from the fixture where it stores them, else from the formulas."""
    H, W, size, B, C = CASES[name]
    if golden is not None and f"{name}/img" in golden:
        return golden[f"{name}/img"], golden[f"{name}/mask"]
    return formula_image(B, H, W, C, seed=len(name)), formula_mask(B, H, W, sparse=name.startswith("sparse"), seed=len(name))


# ---------------------------------------------------------------------------------------------------------------------
# the two torchvision rules (reference infer.py:32-34: Resize([320]), CenterCrop((320, 320)))
# ---------------------------------------------------------------------------------------------------------------------
def view_geometry(H, W, size):
    """-> (ow, oh, top, left).  torchvision.transforms.functional.resize with a one-element size: the short side becomes
    size, the long one int(size * long / short); center_crop: int(round((h - crop_h) / 2.0)) with Python's round."""
    if W <= H:
        ow, oh = size, int(size * H / W)
    else:
        oh, ow = size, int(size * W / H)
    return ow, oh, int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))


# ---------------------------------------------------------------------------------------------------------------------
# Pillow's coefficients of one axis (8-bit bilinear resample), float64, as plain Python
# ---------------------------------------------------------------------------------------------------------------------
def axis_ksize(n_in, n_out):
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def axis_rows(n_in, n_out, first=0, count=None):
    """int64 [count, 2 + ksize]: {xmin, taps, k[ksize]} of the outputs first .. first + count - 1 (numpy float64, every sum in
    index order: the same IEEE operations as the scalar routine)."""
    count = n_out - first if count is None else count
    scale = n_in / n_out
    support = max(scale, 1.0)
    ss = 1.0 / support
    ksize = axis_ksize(n_in, n_out)
    xx = np.arange(first, first + count, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((t < 1.0) & (x < xmax[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(count)
    for j in range(ksize):  # in index order (np.sum adds pairwise)
        ww = ww + w[:, j]
    p = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = (0.5 + p * float(1 << 22)).astype(np.int64)
    return np.concatenate([xmin[:, None], xmax[:, None], k], axis=1)
