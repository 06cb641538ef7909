"""Times ops.poly_layer_backward (curl_poly_layer_bwd_f32: the stand-alone polynomial layers' backward) with both gradients and
with the coefficient gradient only, beside the layer's forward and, on 3-channel shapes, ops.trispace_backward on the same pixel
count -- HIP events around ITERS calls after a warm-up (kernels + launch gaps; the scratch allocation is torch's caching
allocator).  One JSON line at the end.  A record for DESIGN.md 3a, not a pass/fail.

    python tools/poly_layer_bwd_bench.py            # 8x5x1500x1000, 8x3x1500x1000, 32x3x256x256
    ITERS=50 python tools/poly_layer_bwd_bench.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from curl_amd import _lib, ops  # noqa: E402
from stage_bwd_bench import timed  # noqa: E402

SHAPES = [(8, 5, 1500, 1000), (8, 3, 1500, 1000), (32, 3, 256, 256)]


def main():
    iters = int(os.environ.get("ITERS", 30))
    _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = []
    for B, V, H, W in SHAPES:
        img = torch.rand(B, V, H, W, device=dev, generator=g)
        c = torch.randn(B, 3, 126 if V == 5 else 35, device=dev, generator=g) * 0.3
        w = torch.randn(B, 3, H, W, device=dev, generator=g)
        rows = {
            "poly_layer (forward)": lambda: ops.poly_layer(img, c),
            "poly_layer_backward (both)": lambda: ops.poly_layer_backward(img, c, w),
            "poly_layer_backward (coeffs only)": lambda: ops.poly_layer_backward(img, c, w, need_img_grad=False),
            "poly_layer_backward (image only)": lambda: ops.poly_layer_backward(img, c, w, need_coeffs_grad=False),
        }
        if V == 3:
            c9 = torch.randn(B, 3, 3, 35, device=dev, generator=g) * 0.3
            c9s = torch.randn(B, 3, 3, 126, device=dev, generator=g) * 0.3
            rows["trispace_backward (35 coefficients)"] = lambda: ops.trispace_backward(img, c9, w)
            rows["trispace_backward (126 coefficients)"] = lambda: ops.trispace_backward(img, c9s, w)
        for _ in range(2):  # warm clocks: the first pass over the rows is thrown away
            res = {name: timed(fn, iters) for name, fn in rows.items()}
        for name, us in res.items():
            print(f"{B}x{V}x{H}x{W:<5d} {name:38s} {us:9.1f} us/call  {B * H * W / us / 1e3:7.2f} Gpx/s")
        out.append({"shape": [B, V, H, W], "us_per_call": res})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
