"""Single-image inference CLI for the curve model, with the flags of the reference's infer.py:14-17.

    python -m curl_amd.infer --img_path in.png --mask_path mask.png --model_file ckpt.pt --out_path out.png

Shape of the reference's infer.py:32-47, kept: the encoder sees a 320x320 resize+centre-crop of the image, the
curves are applied to the FULL-RESOLUTION image, the result is composited on white where the mask is 0 and saved.
Everything per-pixel runs on the GPU: the decoded uint8 HWC image goes up (3-4 B/px), is converted, enhanced,
composited and quantised on the device, and uint8 HWC comes back.
`--model_file random` builds a randomly initialised model (there is no curve-model checkpoint in the reference tree).
"""
import argparse

import numpy as np
import torch

from . import model as model_mod
from . import ops
from .convert_state import convert_state_dict


def build_net(model_file, device, arch="curl", polynomial_order=4):
    if arch == "trispace":  # infer.py:22-23; a checkpoint trained at another order: ChannelPolyLayer of that order
        net = model_mod.TriSpaceRegNet(polynomial_order=polynomial_order, spatial=True, is_train=False,
                                       polylayer=model_mod.Deg4MobilePolyLayer() if polynomial_order == 4 else None)
    else:
        net = model_mod.GCURLNet(encoder_size=320)
    if model_file != "random":
        ckpt = torch.load(model_file, map_location="cpu")  # infer.py:25
        state = convert_state_dict(ckpt["model_state_dict"] if "model_state_dict" in ckpt else ckpt)  # infer.py:28
        net.load_state_dict(state)
    return net.to(device).eval()


def encoder_view(img, mask, size=320):
    """Resize([320]) (short side) + CenterCrop(320) of infer.py:32-36, on the device, in float: torch's antialiased
    interpolate on the float image (the `view="float"` route of enhance; ops.encoder_view_u8hwc is the reference's own
    arithmetic on the bytes)."""
    _, _, H, W = img.shape
    scale = size / min(H, W)
    nh, nw = max(size, round(H * scale)), max(size, round(W * scale))
    small = torch.nn.functional.interpolate(img, size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)
    msmall = torch.nn.functional.interpolate(mask, size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)
    top, left = (nh - size) // 2, (nw - size) // 2
    return small[:, :, top:top + size, left:left + size], (msmall[:, :, top:top + size, left:left + size] > 0).float()


@torch.no_grad()
def enhance(net, img_u8, mask_u8, device, view="float", foreground=False):
    """img_u8: HxWx3|4 uint8, mask_u8: HxW uint8 ('L').  Returns HxWx3 uint8 (numpy).
    The full-resolution pass runs on the file's own bytes (ops.*_u8hwc: byte/255, the model's per-pixel part, the
    white background and the truncating *255 in one launch).  The 320x320 encoder view:
      view="float"  made in float from the converted full-resolution image (encoder_view above);
      view="pil"    the reference's own view -- Pillow's 8-bit resample of the bytes, bit for bit -- in one launch
                    (ops.encoder_view_u8hwc); no full-resolution float image is made at all.
    foreground=True: the mask is a segmentation mask.  The image goes up with the channel count the file has (no host-side
    slice of an RGBA image) and the full-resolution pass is ops.*_foreground_u8hwc: wavefronts the white background overwrites
    entirely never read their pixels.  The same bytes come back."""
    if view not in ("float", "pil"):
        raise ValueError(f"view must be 'float' or 'pil', got {view!r}")
    if foreground:
        rgb = torch.from_numpy(np.ascontiguousarray(np.asarray(img_u8)[..., :4])).to(device)[None]  # RGB or RGBA, as is
    else:
        rgb = torch.from_numpy(np.ascontiguousarray(np.asarray(img_u8)[..., :3])).to(device)[None]  # alpha dropped
    white = torch.from_numpy(np.array(mask_u8, dtype=np.uint8)).to(device)[None]
    if view == "pil":
        small, msmall = ops.encoder_view_u8hwc(rgb, white)  # infer.py:32-41
    else:
        x = ops.u8hwc_to_f32chw(rgb)
        tmask = white[:, None].float() / 255.0  # to_tensor
        small, msmall = encoder_view(x, tmask)
        del x
    if isinstance(net, model_mod.TriSpaceRegNet):
        coeffs = torch.stack(net.generate_coefficients(small, msmall), 1)       # infer.py:44, model.py:522-527
        if foreground:
            return ops.trispace_foreground_u8hwc(rgb, coeffs, white)[0].cpu().numpy()
        return ops.trispace_forward_u8hwc(rgb, coeffs, white)[0].cpu().numpy()  # infer.py:44-47
    knots = net.predict_knots(small * msmall)  # the encoder sees the masked 320x320 view
    L, R, H = knots[:, :net.curve_break_1], knots[:, net.curve_break_1:net.curve_break_2], knots[:, net.curve_break_2:]
    # the reference applies the mask only when compositing (infer.py:44-46): no layer mask
    cl = net.curllayer
    if foreground:
        out, _ = ops.curl_layer_foreground_u8hwc(rgb, L[:, :cl.num_lab_points].contiguous(), R[:, :cl.num_rgb_points].contiguous(),
                                                 H[:, :cl.num_hsv_points].contiguous(), white)
        return out[0].cpu().numpy()
    out, _ = ops.curl_layer_forward_u8hwc(rgb, None, L[:, :cl.num_lab_points].contiguous(),
                                          R[:, :cl.num_rgb_points].contiguous(),
                                          H[:, :cl.num_hsv_points].contiguous(), white)
    return out[0].cpu().numpy()


@torch.no_grad()
def enhance_many(net, images_u8, masks_u8, device, view="pil", batch_size=32):
    """enhance for a list of images of any sizes: images_u8[i] HxWx3|4 uint8, masks_u8[i] HxW uint8 -> a list of HxWx3 uint8
    arrays.  Per batch of at most batch_size images: the files' bytes go up into one arena (ops.RaggedBytes.pack), the 320x320
    views of all of them are made in one launch (ops.encoder_view_u8hwc_ragged; view="float": per image, encoder_view), the
    encoder runs ONCE on the [n,3,320,320] views, and the full-resolution pass of every image is one ragged call
    (ops.*_u8hwc_ragged).  Given the same coefficients / knots every array equals enhance(net, img, mask, device, view=view) of
    that image alone, byte for byte; the encoder's convolutions on a batch of n may differ from a batch of one in the last bits
    (the convolution library's choice of algorithm per batch size, not this path's)."""
    results = []
    for rb, wm in _packed_batches(images_u8, masks_u8, device, view, batch_size):
        if view == "pil":
            small, msmall = ops.encoder_view_u8hwc_ragged(rb, wm)  # every image's view in one launch
        else:
            smalls, msmalls = [], []
            for i in range(len(rb)):
                rgb, white = rb.image(i)[None], wm.image(i)[None]
                small, msmall = encoder_view(ops.u8hwc_to_f32chw(rgb), white[:, None].float() / 255.0)
                smalls.append(small), msmalls.append(msmall)
            small, msmall = torch.cat(smalls), torch.cat(msmalls)
        results += _full_resolution_many(net, rb, wm, small, msmall, foreground=False)
    return results


@torch.no_grad()
def enhance_many_foreground(net, images_u8, masks_u8, device, view="pil", batch_size=32):
    """enhance_many for masks that are segmentation masks: the same contract and the same arrays, byte for byte, but the
    full-resolution pass of every batch is the foreground ragged call (ops.*_foreground_u8hwc_ragged): wavefronts the white
    background overwrites entirely never read their pixels, workgroups of such wavefronts stage no table.  The views are made
    from the whole images, as enhance_many makes them (the encoder sees what it saw)."""
    results = []
    for rb, wm in _packed_batches(images_u8, masks_u8, device, view, batch_size):
        if view == "pil":
            small, msmall = ops.encoder_view_u8hwc_ragged(rb, wm)
        else:
            views = [encoder_view(ops.u8hwc_to_f32chw(rb.image(i)[None]), wm.image(i)[None, None].float() / 255.0) for i in range(len(rb))]
            small, msmall = torch.cat([v[0] for v in views]), torch.cat([v[1] for v in views])
        results += _full_resolution_many(net, rb, wm, small, msmall, foreground=True)
    return results


def _packed_batches(images_u8, masks_u8, device, view, batch_size):
    """The arguments of enhance_many, checked, and per batch of at most batch_size images the two uploaded arenas."""
    if view not in ("float", "pil"):
        raise ValueError(f"view must be 'float' or 'pil', got {view!r}")
    if len(images_u8) != len(masks_u8):
        raise ValueError(f"one mask per image: {len(images_u8)} images, {len(masks_u8)} masks")
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    device = torch.device(device)

    def batches():
        for b0 in range(0, len(images_u8), batch_size):
            # view="pil": the images go up with the channel count the files have (every ragged entry takes RGBA as it is);
            # view="float": alpha dropped on the host, as enhance does (the float view needs RGB)
            imgs = [np.ascontiguousarray(np.asarray(x)[..., :4 if view == "pil" else 3]) for x in images_u8[b0:b0 + batch_size]]
            rb = ops.RaggedBytes.pack(imgs, device)
            yield rb, ops.RaggedBytes.pack([np.array(m, dtype=np.uint8) for m in masks_u8[b0:b0 + batch_size]], device)
    return batches()


@torch.no_grad()
def enhance_and_score_many(net, images_u8, masks_u8, targets_u8, device, view="pil", batch_size=32, foreground=False):
    """enhance_many (foreground=True: enhance_many_foreground) and the score of every output against its target:
    targets_u8[i] HxWx3|4 uint8 of image i's size (alpha is dropped on the host) -> (outputs, psnr).  The outputs are those
    functions' arrays, byte for byte; psnr is a float64 numpy array [N], the masked PSNR of evaluate.py:102 with the white mask
    as the metric's mask, exact on the bytes (ops.psnr_u8hwc_ragged): nan where the mask keeps no pixel, inf for an output
    equal to its target.  Per batch the out arena stays on the device, the targets go up as one RGB arena, the mask arena is
    the one already uploaded, and the score is ONE call; no float image is made."""
    results, psnr, _, _ = _enhance_and_score(net, images_u8, masks_u8, targets_u8, device, view, batch_size, foreground, msssim=False)
    return results, psnr


@torch.no_grad()
def enhance_and_score_many_msssim(net, images_u8, masks_u8, targets_u8, device, view="pil", batch_size=32, foreground=False):
    """enhance_and_score_many with the reference's second figure: -> (outputs, psnr, msssim).  msssim is a float64 numpy array
    [N], the MS-SSIM of out * mask against gt * mask (evaluate.py:105, metric.py:168-208) from the bytes
    (ops.msssim_u8hwc_ragged): per batch ONE more call, on the out arena, the target arena and the mask arena the PSNR call
    uses.  An image under 32 pixels on a side has no five-level pyramid: it gets nan and is left out of the call (the rest of
    its batch is then packed again on the device)."""
    return _enhance_and_score(net, images_u8, masks_u8, targets_u8, device, view, batch_size, foreground, msssim=True)[:3]


@torch.no_grad()
def enhance_and_evaluate_many(net, images_u8, masks_u8, targets_u8, device, view="pil", batch_size=32, foreground=False):
    """enhance_and_score_many_msssim with the reference Evaluator's first figure (evaluate.py:101): -> (outputs, psnr, msssim,
    loss).  loss is a float64 numpy array [N], the criterion of every output against its target under its mask -- CURLLoss
    (model.py:78-116) image by image, as CURLLoss()(pred[None], target[None], mask[None]) -- from the bytes
    (ops.curl_loss_u8hwc_ragged): per batch ONE more call, on the arenas the other two scores use.  It is the criterion of the
    BYTES WRITTEN (byte / 255), not of the network's unrounded float output, which the training loop's Evaluator sees.  An
    image under 32 pixels on a side gets nan and is left out of the call, as for msssim; an image whose mask keeps no pixel
    gets nan too (the reference's 0 / 0).  Outputs, psnr and msssim are enhance_and_score_many_msssim's."""
    return _enhance_and_score(net, images_u8, masks_u8, targets_u8, device, view, batch_size, foreground, msssim=True, loss=True)


def _enhance_and_score(net, images_u8, masks_u8, targets_u8, device, view, batch_size, foreground, msssim, loss=False):
    """The body of the three functions above -> (outputs, psnr, msssim or None, loss or None)."""
    if len(targets_u8) != len(images_u8):
        raise ValueError(f"one target per image: {len(images_u8)} images, {len(targets_u8)} targets")
    targets = []
    for i, (img, tgt) in enumerate(zip(images_u8, targets_u8)):
        t = np.asarray(tgt)
        if t.dtype != np.uint8 or t.ndim != 3 or t.shape[2] not in (3, 4):
            raise ValueError(f"target {i} must be uint8 HxWx3|4, got {t.dtype} {t.shape}")
        if t.shape[:2] != np.asarray(img).shape[:2]:
            raise ValueError(f"target {i} is {t.shape[0]}x{t.shape[1]}, its image {np.asarray(img).shape[0]}x{np.asarray(img).shape[1]}")
        targets.append(t)
    results, scores, ms, losses = [], [], [], []
    for k, (rb, wm) in enumerate(_packed_batches(images_u8, masks_u8, device, view, batch_size)):
        small, msmall = _encoder_views(rb, wm, view)
        out = _full_resolution_device(net, rb, wm, small, msmall, foreground)
        tg = ops.RaggedBytes.pack([np.ascontiguousarray(t[..., :3]) for t in targets[k * batch_size:(k + 1) * batch_size]], rb.device)
        psnr = ops.psnr_u8hwc_ragged(out, tg, wm)  # one score call per batch, on the arenas the batch already has
        if msssim:
            ms.append(_pyramid_score_of_batch(ops.msssim_u8hwc_ragged, out, tg, wm))
        if loss:
            losses.append(_pyramid_score_of_batch(ops.curl_loss_u8hwc_ragged, out, tg, wm))
        results += _download(out)
        scores.append(psnr.cpu().numpy())
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.float64)  # noqa: E731
    return results, cat(scores), cat(ms) if msssim else None, cat(losses) if loss else None


def _pyramid_score_of_batch(score, out, tg, wm):
    """A five-level score (ops.msssim_u8hwc_ragged, ops.curl_loss_u8hwc_ragged) of a batch's out arena against its target arena
    under its mask arena, one call -> float64 numpy [n]; nan for the images under 32 pixels on a side, which the call never sees."""
    keep = [i for i, (h, w) in enumerate(out.shapes) if min(h, w) >= ops.MSSSIM_MIN_SIDE]
    values = np.full(len(out), np.nan, dtype=np.float64)
    if len(keep) == len(out):
        values[:] = score(out, tg, wm).cpu().numpy()
    elif keep:
        sub = [ops.RaggedBytes.pack([x.image(i) for i in keep], out.device) for x in (out, tg, wm)]
        values[keep] = score(*sub).cpu().numpy()
    return values


def _encoder_views(rb, wm, view):
    """The [n,3,320,320] views of a packed batch as enhance_many and enhance_many_foreground make them (their bodies spell the
    calls out; tests read them there)."""
    if view == "pil":
        return ops.encoder_view_u8hwc_ragged(rb, wm)
    views = [encoder_view(ops.u8hwc_to_f32chw(rb.image(i)[None]), wm.image(i)[None, None].float() / 255.0) for i in range(len(rb))]
    return torch.cat([v[0] for v in views]), torch.cat([v[1] for v in views])


def _full_resolution_many(net, rb, wm, small, msmall, foreground):
    """The encoder once on the [n,3,320,320] views, the full-resolution pass of the batch in one ragged call (foreground: the
    foreground-aware one) and one download -> the batch's HxWx3 uint8 arrays."""
    return _download(_full_resolution_device(net, rb, wm, small, msmall, foreground))


def _download(out):
    """One download of an out arena -> the batch's HxWx3 uint8 arrays."""
    host = out.arena.cpu().numpy()
    return [host[o:o + h * w * 3].reshape(h, w, 3).copy() for (h, w), o in zip(out.shapes, out.offsets)]


def _full_resolution_device(net, rb, wm, small, msmall, foreground):
    """The device part of _full_resolution_many -> the RaggedBytes of the outputs, still on the device."""
    if isinstance(net, model_mod.TriSpaceRegNet):
        coeffs = torch.stack(net.generate_coefficients(small, msmall), 1)
        out = (ops.trispace_foreground_u8hwc_ragged if foreground else ops.trispace_forward_u8hwc_ragged)(rb, coeffs, wm)
    else:
        knots = net.predict_knots(small * msmall)
        L, R, H = knots[:, :net.curve_break_1], knots[:, net.curve_break_1:net.curve_break_2], knots[:, net.curve_break_2:]
        cl = net.curllayer
        layer = ops.curl_layer_foreground_u8hwc_ragged if foreground else ops.curl_layer_forward_u8hwc_ragged
        out, _ = layer(rb, L[:, :cl.num_lab_points].contiguous(), R[:, :cl.num_rgb_points].contiguous(),
                       H[:, :cl.num_hsv_points].contiguous(), wm)
    return out


def infer(argv=None):
    parser = argparse.ArgumentParser(description="Run image enhancement model on a single image")
    parser.add_argument("--img_path", type=str, required=True, help="Path to image to enhancement")
    parser.add_argument("--mask_path", type=str, required=True, help="Path to image to enhancement")
    parser.add_argument("--model_file", type=str, required=True, help="Path to model checkpoint file ('random' = random init)")
    parser.add_argument("--out_path", type=str, required=True, help="Path to write output image to")
    parser.add_argument("--arch", choices=("trispace", "curl"), default="trispace",
                        help="trispace = the reference's infer.py model (TriSpaceRegNet + Deg4MobilePolyLayer); "
                             "curl = the curve model (GCURLNet)")
    parser.add_argument("--polynomial_order", type=int, default=4, choices=(1, 2, 3, 4),
                        help="trispace: the polynomial_order the checkpoint was trained with (model.py:439)")
    parser.add_argument("--encoder_view", choices=("float", "pil"), default="float",
                        help="how the encoder's 320x320 input is made: float = torch's antialiased interpolate on the float "
                             "image; pil = the reference's Pillow resample of the bytes, bit for bit, in one HIP launch")
    parser.add_argument("--foreground_masks", action="store_true",
                        help="the mask is a segmentation mask: regions it whites out entirely are never read or computed "
                             "(the same output bytes)")
    args = parser.parse_args(argv)
    from PIL import Image
    device = torch.device("cuda:0")
    net = build_net(args.model_file, device, args.arch, args.polynomial_order)
    img = np.asarray(Image.open(args.img_path))
    if img.ndim == 2:
        img = np.repeat(img[..., None], 3, axis=2)
    mask = np.asarray(Image.open(args.mask_path).convert("L"))
    out = enhance(net, img, mask, device, view=args.encoder_view, foreground=args.foreground_masks)
    Image.fromarray(out).save(args.out_path)


if __name__ == "__main__":
    infer()
