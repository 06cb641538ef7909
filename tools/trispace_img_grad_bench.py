"""Times the fused polynomial model's image gradient, ops.trispace_backward_img (curl_trispace_bwd_img_f32: one kernel), beside
the route that gave the same gradient before it existed: the model assembled from the stand-alone differentiable pieces
(colors.*, ChannelPolyLayer(degree=4) on cat_coords, torch.sigmoid, torch.clamp) and differentiated by autograd -- forward and
backward, since that route has to run both.  Same process, the two alternating; HIP events around ITERS calls after a discarded
pass over both (warm clocks, loaded code objects).  One JSON line at the end.  A record for DESIGN.md 3a, not a pass/fail.

    python tools/trispace_img_grad_bench.py         # 8x1500x1000 and 32x256x256, 126 and 35 coefficients
    ITERS=50 python tools/trispace_img_grad_bench.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from curl_amd import _lib, colors, model, ops  # noqa: E402
from stage_bwd_bench import timed  # noqa: E402

SHAPES = [(8, 1500, 1000), (32, 256, 256)]


def assembled(dev, nc, B, H, W):
    """-> f(img, coeffs, w) = d ((clamp(img + residual)) * w).sum() / d img through the stand-alone ops' autograd nodes."""
    V = 5 if nc == 126 else 3
    poly = model.ChannelPolyLayer(degree=4, num_variables=V, num_out=3).to(dev)
    rgb2lab, lab2rgb, rgb2hsv, hsv2rgb = (m.to(dev) for m in (colors.RGB2LAB(), colors.LAB2RGB(), colors.RGB2HSV(), colors.HSV2RGB()))
    xs = (torch.arange(W, device=dev) / W).reshape(1, 1, 1, W).expand(B, 1, H, W)
    ys = (torch.arange(H, device=dev) / H).reshape(1, 1, H, 1).expand(B, 1, H, W)

    def cat(t):
        return torch.cat([t, xs, ys], 1) if V == 5 else t

    def grad(img, c, w):
        x = img.detach().requires_grad_()
        res = 2 * (torch.sigmoid(poly(cat(x), c[:, 0])) - 0.5) \
            + 2 * (lab2rgb(torch.sigmoid(poly(cat(rgb2lab(x)), c[:, 1]))) - 0.5) \
            + 2 * (hsv2rgb(torch.sigmoid(poly(cat(rgb2hsv(x)), c[:, 2]))) - 0.5)
        (g,) = torch.autograd.grad(torch.clamp(x + res, 0.0, 1.0), x, w)
        return g
    return grad


def main():
    iters = int(os.environ.get("ITERS", 30))
    _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = []
    for B, H, W in SHAPES:
        img = torch.rand(B, 3, H, W, device=dev, generator=g)
        w = torch.randn(B, 3, H, W, device=dev, generator=g)
        for nc in (126, 35):
            c = torch.randn(B, 3, 3, nc, device=dev, generator=g) * 0.3
            route = assembled(dev, nc, B, H, W)
            a, b = ops.trispace_backward_img(img, c, w), route(img, c, w)
            diff = float((a - b).abs().max() / b.abs().max())  # the two routes compute the same thing
            rows = {"trispace_backward_img (fused)": lambda: ops.trispace_backward_img(img, c, w),
                    "assembled model, autograd (forward + backward)": lambda: route(img, c, w)}
            for _ in range(2):  # the first pass over the rows is thrown away
                res = {name: timed(fn, iters) for name, fn in rows.items()}
            fused, slow = res.values()
            for name, us in res.items():
                print(f"{B}x3x{H}x{W:<5d} nc={nc:<3d} {name:48s} {us:10.1f} us/call  {B * H * W / us / 1e3:7.2f} Gpx/s")
            print(f"{B}x3x{H}x{W:<5d} nc={nc:<3d} ratio {slow / fused:.1f}x   max|fused - assembled| / max|assembled| = {diff:.2e}")
            out.append({"shape": [B, 3, H, W], "num_coeffs": nc, "us_per_call": res, "ratio": slow / fused, "rel_diff": diff})
            del route, a, b
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
