"""Writes tests/golden/encoder_view.npz: what the reference's `cropper(resizer(.))` (infer.py:32-41) yields for the cases of
tests/encoder_view_cases.py, taken from Pillow itself.

    python tests/golden/make_golden_encoder_view.py

torchvision's Resize on a PIL image is `img.resize((ow, oh), Image.BILINEAR)` and its CenterCrop is `img.crop`; its two size
rules are restated in encoder_view_cases.view_geometry (torchvision is not needed to run this).  The mask goes the same way
as an 'L' image (infer.py:37-41).  Stored per case: view uint8 [B,3,size,size] and mask_view uint8 [B,size,size] -- the
resampled BYTES; to_tensor's / 255 and the mask's `> 0` are exact and are applied by the tests -- and, for the small cases,
the inputs img [B,H,W,C] and mask [B,H,W]."""
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import encoder_view_cases as cases  # noqa: E402


def pillow_view(a, H, W, size):
    """a: uint8 [H,W,3] or [H,W] -> the cropped resize, same layout."""
    ow, oh, top, left = cases.view_geometry(H, W, size)
    small = Image.fromarray(a).resize((ow, oh), Image.BILINEAR)
    return np.asarray(small.crop((left, top, left + size, top + size)))


def main():
    out = {}
    for name, (H, W, size, B, C) in cases.CASES.items():
        img, mask = cases.inputs(name)
        view = np.stack([pillow_view(np.ascontiguousarray(img[b, :, :, :3]), H, W, size) for b in range(B)])  # alpha dropped
        out[f"{name}/view"] = np.ascontiguousarray(view.transpose(0, 3, 1, 2))
        out[f"{name}/mask_view"] = np.stack([pillow_view(mask[b], H, W, size) for b in range(B)])
        if name not in cases.FORMULA_INPUTS:
            out[f"{name}/img"], out[f"{name}/mask"] = img, mask
    np.savez_compressed(cases.GOLDEN, **out)
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), "bytes; Pillow", Image.__version__)


if __name__ == "__main__":
    main()
