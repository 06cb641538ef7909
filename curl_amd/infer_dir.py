"""Folder inference CLI: every image of a folder through the model, the model loaded once, the full-resolution pass of a
whole batch of differently sized images in one ragged call (infer.enhance_many).

    python -m curl_amd.infer_dir --img_dir in/ --mask_dir masks/ --model_file ckpt.pt --out_dir out/

A mask belongs to the image with the same file stem (in/a.png <- masks/a.png, or any other extension).  Every output is
written as <out_dir>/<stem>.png.  The flags shared with curl_amd.infer mean what they mean there; --foreground_masks takes
the foreground-aware ragged call (infer.enhance_many_foreground): the same files, the masked-out regions never computed.

--gt_dir G scores every output against the target of the same stem in G (infer.enhance_and_score_many: the masked PSNR of
the reference's Evaluator, exact on the bytes, one score call per batch): one `stem<TAB>psnr` line per image, then
`mean<TAB>value<TAB>left_out` -- the mean over the images whose PSNR is finite and the number of images left out of it.
--scores_file F writes the same lines to F.  --msssim (with --gt_dir) adds the reference's second figure, the MS-SSIM of the
masked output against the masked target (infer.enhance_and_score_many_msssim, one more call per batch): the lines are
`stem<TAB>psnr<TAB>msssim`, an image under 32 pixels on a side has msssim nan, and the last line is
`mean<TAB>psnr mean<TAB>msssim mean<TAB>left_out of the psnr mean<TAB>left_out of the msssim mean`.  --loss (with --gt_dir,
combinable with --msssim) appends the Evaluator's first figure, the criterion (CURLLoss, image by image) of the output FILE's
pixels -- byte / 255, not the network's unrounded float output -- against the target under the mask
(infer.enhance_and_evaluate_many, one more call per batch): a last `loss` column on every image's line (nan under 32 pixels
on a side or where the mask keeps no pixel), and on the last line its mean over the finite ones behind the other means and
its left_out count behind the other counts.
"""
import argparse
import math
import os

import numpy as np
import torch

from .infer import (build_net, enhance_and_evaluate_many, enhance_and_score_many, enhance_and_score_many_msssim, enhance_many,
                    enhance_many_foreground)

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")


def _by_stem(folder):
    out = {}
    for name in sorted(os.listdir(folder)):
        stem, ext = os.path.splitext(name)
        if ext.lower() in IMAGE_EXTENSIONS and stem not in out:
            out[stem] = os.path.join(folder, name)
    return out


def _rgb(path):
    from PIL import Image
    img = np.asarray(Image.open(path))
    return np.repeat(img[..., None], 3, axis=2) if img.ndim == 2 else img


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
    parser.add_argument("--gt_dir", type=str, default=None,
                        help="Folder of target images, matched to the images by file stem: print every output's masked PSNR "
                             "against its target and the mean over the finite ones")
    parser.add_argument("--scores_file", type=str, default=None, help="with --gt_dir: also write the score lines to this file")
    parser.add_argument("--msssim", action="store_true",
                        help="with --gt_dir: also print every output's MS-SSIM against its target (nan under 32 pixels on a side)")
    parser.add_argument("--loss", action="store_true",
                        help="with --gt_dir: also print the criterion (CURLLoss) of every output file's pixels against its target "
                             "(nan under 32 pixels on a side)")
    args = parser.parse_args(argv)
    if args.loss and args.gt_dir is None:
        parser.error("--loss needs --gt_dir")
    if args.scores_file is not None and args.gt_dir is None:
        parser.error("--scores_file needs --gt_dir")
    if args.msssim and args.gt_dir is None:
        parser.error("--msssim needs --gt_dir")
    enhance = enhance_many_foreground if args.foreground_masks else enhance_many
    from PIL import Image
    images, masks = _by_stem(args.img_dir), _by_stem(args.mask_dir)
    targets = _by_stem(args.gt_dir) if args.gt_dir is not None else None
    for stem, path in images.items():
        if stem not in masks:
            raise FileNotFoundError(f"no mask for {path}: nothing named {stem}.* in {args.mask_dir}")
        if targets is not None and stem not in targets:
            raise FileNotFoundError(f"no target for {path}: nothing named {stem}.* in {args.gt_dir}")
    device = torch.device("cuda:0")
    net = build_net(args.model_file, device, args.arch, args.polynomial_order)
    os.makedirs(args.out_dir, exist_ok=True)
    stems = list(images)
    lines, finite, finite_ms, finite_loss = [], [], [], []
    for b0 in range(0, len(stems), args.batch_size):  # a batch of files in memory at a time
        batch = stems[b0:b0 + args.batch_size]
        imgs = [_rgb(images[stem]) for stem in batch]
        ms = [np.asarray(Image.open(masks[stem]).convert("L")) for stem in batch]
        if targets is None:
            outs = enhance(net, imgs, ms, device, view=args.encoder_view, batch_size=args.batch_size)
        elif args.loss:
            outs, psnr, msssim, loss = enhance_and_evaluate_many(net, imgs, ms, [_rgb(targets[stem]) for stem in batch], device,
                                                                 view=args.encoder_view, batch_size=args.batch_size,
                                                                 foreground=args.foreground_masks)
            for stem, value, second, third in zip(batch, psnr, msssim, loss):
                lines.append(f"{stem}\t{float(value)!r}" + (f"\t{float(second)!r}" if args.msssim else "") + f"\t{float(third)!r}")
                for figure, kept in ((value, finite), (second, finite_ms), (third, finite_loss)):
                    if math.isfinite(figure):
                        kept.append(float(figure))
        elif args.msssim:
            outs, psnr, msssim = enhance_and_score_many_msssim(net, imgs, ms, [_rgb(targets[stem]) for stem in batch], device,
                                                               view=args.encoder_view, batch_size=args.batch_size,
                                                               foreground=args.foreground_masks)
            for stem, value, second in zip(batch, psnr, msssim):
                lines.append(f"{stem}\t{float(value)!r}\t{float(second)!r}")
                if math.isfinite(value):
                    finite.append(float(value))
                if math.isfinite(second):
                    finite_ms.append(float(second))
        else:
            outs, psnr = enhance_and_score_many(net, imgs, ms, [_rgb(targets[stem]) for stem in batch], device, view=args.encoder_view,
                                                batch_size=args.batch_size, foreground=args.foreground_masks)
            for stem, value in zip(batch, psnr):
                lines.append(f"{stem}\t{float(value)!r}")
                if math.isfinite(value):
                    finite.append(float(value))
        for stem, out in zip(batch, outs):
            Image.fromarray(out).save(os.path.join(args.out_dir, stem + ".png"))
    if targets is not None:
        mean = sum(finite) / len(finite) if finite else float("nan")
        if args.loss:
            kept = [finite] + ([finite_ms] if args.msssim else []) + [finite_loss]
            means = [sum(k) / len(k) if k else float("nan") for k in kept]
            lines.append("mean\t" + "\t".join(repr(v) for v in means) + "\t" + "\t".join(str(len(lines) - len(k)) for k in kept))
        elif args.msssim:
            mean_ms = sum(finite_ms) / len(finite_ms) if finite_ms else float("nan")
            lines.append(f"mean\t{mean!r}\t{mean_ms!r}\t{len(lines) - len(finite)}\t{len(lines) - len(finite_ms)}")
        else:
            lines.append(f"mean\t{mean!r}\t{len(lines) - len(finite)}")
        print("\n".join(lines))
        if args.scores_file is not None:
            with open(args.scores_file, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
