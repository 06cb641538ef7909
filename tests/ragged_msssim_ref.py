"""The shapes, contents, masks and reference values of the ragged MS-SSIM tests (tests/test_ragged_msssim_abi.py,
tests/test_gpu_ragged_msssim.py).  The yardstick is the oracle in float64 through criterion_check.MsssimReference on the
float images bytes.float() / 255 times (mask > 0), in NCHW; the bound is its own stats_bound = max(2e-6, 4 r32_stats), r32
from the oracle alone.  Nothing of the library is used."""
import numpy as np
import torch

# (H, W) of the one batch, each the smallest at which a step can go wrong (32 x 32 tiles, five levels of floor halving)
SHAPES = [
    (32, 32),    # one tile; level 4 is 2 x 2
    (33, 47),    # a second tile column and a one-row second tile row, odd at every level
    (63, 32),    # floor pooling drops a row at every level
    (64, 65),    # exact tile rows plus a one-pixel tile column
    (70, 97),
    (97, 129),   # 129 -> 64 -> 32 -> 16 -> 8
    (160, 40),   # tall
    (40, 160),   # wide
]
CONTENTS = "rensxf"  # random | equal | near (target + noise of +-12) | smooth (a ramp + noise of +-3) | extremes | flat
MASKS = "fzcl"       # all 255 | all 0 | random over {0, 1, 128, 255} | left half 0   (None: no mask arena)
TIGHT = "rns"        # the contents whose bound is 2e-6 .. 2.2e-5: the evidence; x and f are ill-conditioned in float32
LEVELS = 5
# metric.py:86, float32 there and raised to the images' dtype
WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float32).astype(np.float64)


def _rand_u8(g, *shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)


def make_data(seed=2011):
    """content kind -> the (a, b) pairs of SHAPES; mask kind -> the masks.  uint8 host tensors, made once, never changed."""
    g = torch.Generator().manual_seed(seed)
    pairs, masks = {k: [] for k in CONTENTS}, {k: [] for k in MASKS}
    for h, w in SHAPES:
        a = _rand_u8(g, h, w, 3)
        pairs["r"].append((a, _rand_u8(g, h, w, 3)))
        pairs["e"].append((a, a.clone()))
        pairs["n"].append((a, (a.int() + torch.randint(-12, 13, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)))
        ramp = (torch.linspace(0, 255, w).view(1, w, 1) * 0.7 + torch.linspace(0, 70, h).view(h, 1, 1)).expand(h, w, 3).to(torch.uint8)
        pairs["s"].append((ramp.contiguous(), (ramp.int() + torch.randint(-3, 4, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)))
        pairs["x"].append((torch.zeros(h, w, 3, dtype=torch.uint8), torch.full((h, w, 3), 255, dtype=torch.uint8)))
        pairs["f"].append((torch.full((h, w, 3), 100, dtype=torch.uint8), torch.full((h, w, 3), 101, dtype=torch.uint8)))
        left = torch.full((h, w), 255, dtype=torch.uint8)
        left[:, :w // 2] = 0
        masks["f"].append(torch.full((h, w), 255, dtype=torch.uint8))
        masks["z"].append(torch.zeros(h, w, dtype=torch.uint8))
        masks["c"].append(torch.tensor([0, 1, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (h, w), generator=g)])
        masks["l"].append(left)
    return pairs, masks


def float_images(a, b, mask=None):
    """uint8 [H,W,3] a, b and uint8 [H,W] mask (or None) -> the float32 [1,3,H,W] images the reference's Evaluator scores:
    bytes.float() / 255, times mask > 0."""
    fa, fb = (torch.as_tensor(x).permute(2, 0, 1)[None].float() / 255 for x in (a, b))
    if mask is not None:
        keep = (torch.as_tensor(mask) > 0)[None, None].float()
        fa, fb = fa * keep, fb * keep
    return fa, fb


def reference(a, b, mask=None, window_size=11):
    """-> criterion_check.MsssimReference of the float images: .stats64 [2,1,5] float64, .stats_bound."""
    import criterion_check as CC
    return CC.MsssimReference(*float_images(a, b, mask), window_size)


def msssim_formula(stats):
    """metric.py:200-207 on [B,2,5] float64 statistics in numpy: (x + 1) / 2, the powers by the five weights,
    prod(mcs[:-1]^w[:-1] * ssims[-1]^w[-1]) -- the last factor four times, as there."""
    x = (np.asarray(stats, dtype=np.float64) + 1) / 2
    pow1, pow2 = x[:, 1] ** WEIGHTS, x[:, 0] ** WEIGHTS
    return np.prod(pow1[:, :-1] * pow2[:, -1:], axis=1)


def plan_by_hand(shapes, has_mask):
    """The plan of include/curl_hip_ragged_msssim.h worked out independently: per image rgb_off, mask_off and per level
    (h, w, tiles_x, tiles, first, pair, planes); and the header's grids, pair0s, arena sizes, partial offset, workspace bytes."""
    align = lambda v: (v + 15) & ~15  # noqa: E731
    rgb = mask = planes = 0
    grid = [0] * LEVELS
    images = []
    for h, w in shapes:
        rgb, mask = align(rgb), align(mask)
        img = {"rgb_off": rgb, "mask_off": mask if has_mask else 0, "levels": []}
        rgb, mask = rgb + 3 * h * w, mask + (h * w if has_mask else 0)
        for l in range(LEVELS):
            hl, wl = h >> l, w >> l
            tx = -(-wl // 32)
            tiles = tx * -(-hl // 32)
            off = 0
            if l >= 1:
                planes = align(planes)
                off, planes = planes, planes + 24 * hl * wl
            img["levels"].append({"h": hl, "w": wl, "tiles_x": tx, "tiles": tiles, "first": grid[l], "planes": off})
            grid[l] += tiles
        images.append(img)
    pair0 = [sum(grid[:l]) for l in range(LEVELS)]
    for img in images:
        for l, lv in enumerate(img["levels"]):
            lv["pair"] = pair0[l] + lv["first"]
    planes = align(planes)
    return images, {"grid": grid, "pair0": pair0, "rgb_bytes": rgb, "mask_bytes": mask, "partial_off": planes,
                    "ws_bytes": planes + 16 * sum(grid)}
