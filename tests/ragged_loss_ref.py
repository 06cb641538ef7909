"""The reference values of the ragged CURLLoss tests (tests/test_ragged_loss_abi.py, tests/test_gpu_ragged_loss.py).  Shapes,
contents, masks and their rotation are tests/ragged_msssim_ref.py's (imported, not changed).  The yardstick is the oracle in
float64 (oracle/curl_oracle.py: curl_loss_terms, msssim, curl_loss) on bytes.float() / 255 with the bool mask `mask > 0`, one
image at a time -- the reference's own definition at batch size 1.  Nothing of the library is used."""
import numpy as np
import torch

from ragged_msssim_ref import LEVELS, msssim_formula

TERMS = 5  # float64 per level-0 workgroup: four term sums and the count


def float_pair(a, b, mask=None):
    """uint8 [H,W,3] a, b and uint8 [H,W] mask (or None) -> (pred, target, keep): float32 [1,3,H,W] bytes.float() / 255 (NOT yet
    masked: CURLLoss multiplies itself, model.py:90) and the bool [1,1,H,W] mask data.py:190 makes, all ones without a mask."""
    fa, fb = (torch.as_tensor(x).permute(2, 0, 1)[None].float() / 255 for x in (a, b))
    keep = torch.ones(1, 1, *fa.shape[2:], dtype=torch.bool) if mask is None else (torch.as_tensor(mask) > 0)[None, None]
    return fa, fb, keep


class LossReference:
    """One image's CURLLoss in float64 from the oracle: .terms (rgb, cosine, lab, hsv), .n (the unmasked pixels), .Lp / .Lt
    (the float64 clamped L planes [1,1,H,W]), .row0 (the five raw sums the terms come from) and, where the mask keeps a pixel and
    the image has five levels, .msssim and .loss."""

    def __init__(self, a, b, mask=None):
        import curl_oracle as O
        pred, target, keep = float_pair(a, b, mask)
        H, W = pred.shape[2:]
        self.n = int(keep.sum())
        with np.errstate(all="ignore"):
            rgb, cosine, lab, hsv, Lp, Lt = O.curl_loss_terms(pred.double(), target.double(), keep)
        self.terms = tuple(float(v) for v in (rgb, cosine, lab, hsv))
        self.Lp, self.Lt = Lp, Lt
        n3, hw = 3.0 * self.n, float(H * W)
        # the raw sums behind the terms: S / (3 N) three times, 1 - (S_cos + (H W - N)) / (H W) for the cosine (model.py:92-98)
        self.row0 = np.array([self.terms[0] * n3, (1.0 - self.terms[1]) * hw - (hw - self.n), self.terms[2] * n3, self.terms[3] * n3,
                              float(self.n)])
        if min(H, W) >= 32:
            self.msssim = float(O.msssim(Lp, Lt, 11, 1)[0])
            self.loss = float(O.curl_loss(pred.double(), target.double(), keep, (1 - O.msssim(Lp, Lt, 11, 1)).mean()))


def loss_formula(stats, shapes):
    """model.py:89-116 on [B,3,5] float64 statistics and the images' (H, W), in numpy -> float64 [B]."""
    stats = np.asarray(stats, dtype=np.float64)
    hw = np.array([float(h * w) for h, w in shapes])
    with np.errstate(all="ignore"):
        S, n = stats[:, 0, :4], stats[:, 0, 4]
        rgb, lab, hsv = S[:, 0] / (3 * n), S[:, 2] / (3 * n), S[:, 3] / (3 * n)
        cosine = 1 - (S[:, 1] + (hw - n)) / hw
        ssim = 1 - msssim_formula(stats[:, 1:])
        return (rgb + cosine + lab + hsv + 10 * ssim) / 5


def plan_by_hand(shapes, has_mask):
    """The plan of include/curl_hip_ragged_loss.h worked out independently: per image rgb_off, mask_off and per level
    (h, w, tiles_x, tiles, first, pair, planes -- TWO float planes per level); and the header's grids, pair0s, arena sizes,
    partial offset, term offset and workspace bytes."""
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
                off, planes = planes, planes + 8 * hl * wl
            img["levels"].append({"h": hl, "w": wl, "tiles_x": tx, "tiles": tiles, "first": grid[l], "planes": off})
            grid[l] += tiles
        images.append(img)
    pair0 = [sum(grid[:l]) for l in range(LEVELS)]
    for img in images:
        for l, lv in enumerate(img["levels"]):
            lv["pair"] = pair0[l] + lv["first"]
    planes = align(planes)
    terms_off = planes + 16 * sum(grid)
    return images, {"grid": grid, "pair0": pair0, "rgb_bytes": rgb, "mask_bytes": mask, "partial_off": planes, "terms_off": terms_off,
                    "ws_bytes": terms_off + 8 * TERMS * grid[0]}
