"""Folder inference CLI: every image of a folder through the model, the model loaded once, the full-resolution pass of a
whole batch of differently sized images in one ragged call (infer.enhance_many).

    python -m curl_amd.infer_dir --img_dir in/ --mask_dir masks/ --model_file ckpt.pt --out_dir out/

A mask belongs to the image with the same file stem (in/a.png <- masks/a.png, or any other extension).  Every output is
written as <out_dir>/<stem>.png.  The flags shared with curl_amd.infer mean what they mean there; --foreground_masks takes
the foreground-aware ragged call (infer.enhance_many_foreground): the same files, the masked-out regions never computed.
"""
import argparse
import os

import numpy as np
import torch

from .infer import build_net, enhance_many, enhance_many_foreground

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")


def _by_stem(folder):
    out = {}
    for name in sorted(os.listdir(folder)):
        stem, ext = os.path.splitext(name)
        if ext.lower() in IMAGE_EXTENSIONS and stem not in out:
            out[stem] = os.path.join(folder, name)
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description="Run image enhancement model on every image of a folder")
    parser.add_argument("--img_dir", type=str, required=True, help="Folder of images to enhance")
    parser.add_argument("--mask_dir", type=str, required=True, help="Folder of masks, matched to the images by file stem")
    parser.add_argument("--model_file", type=str, required=True, help="Path to model checkpoint file ('random' = random init)")
    parser.add_argument("--out_dir", type=str, required=True, help="Folder to write the output images to (<stem>.png)")
    parser.add_argument("--arch", choices=("trispace", "curl"), default="trispace")
    parser.add_argument("--polynomial_order", type=int, default=4, choices=(1, 2, 3, 4))
    parser.add_argument("--encoder_view", choices=("float", "pil"), default="float")
    parser.add_argument("--batch_size", type=int, default=32, help="images per ragged call")
    parser.add_argument("--foreground_masks", action="store_true",
                        help="the masks are segmentation masks: regions they white out entirely are never read or computed "
                             "(the same output bytes)")
    args = parser.parse_args(argv)
    enhance = enhance_many_foreground if args.foreground_masks else enhance_many
    from PIL import Image
    images, masks = _by_stem(args.img_dir), _by_stem(args.mask_dir)
    for stem, path in images.items():
        if stem not in masks:
            raise FileNotFoundError(f"no mask for {path}: nothing named {stem}.* in {args.mask_dir}")
    device = torch.device("cuda:0")
    net = build_net(args.model_file, device, args.arch, args.polynomial_order)
    os.makedirs(args.out_dir, exist_ok=True)
    stems = list(images)
    for b0 in range(0, len(stems), args.batch_size):  # a batch of files in memory at a time
        batch = stems[b0:b0 + args.batch_size]
        imgs, ms = [], []
        for stem in batch:
            img = np.asarray(Image.open(images[stem]))
            if img.ndim == 2:
                img = np.repeat(img[..., None], 3, axis=2)
            imgs.append(img)
            ms.append(np.asarray(Image.open(masks[stem]).convert("L")))
        for stem, out in zip(batch, enhance(net, imgs, ms, device, view=args.encoder_view, batch_size=args.batch_size)):
            Image.fromarray(out).save(os.path.join(args.out_dir, stem + ".png"))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
