"""Times the backward entry points of the stand-alone curve ops, converters and stages beside curl_layer_bwd_f32 (with the
image gradient) on the same inputs.  Meant to run under `rocprofv3 --kernel-trace --stats` (one shape per process, so that
the per-kernel averages belong to it); it also prints its own event-timed per-call times (kernels + launch gaps).

    SHAPE=frames python tools/stage_bwd_bench.py   # 32 x 3 x 1500 x 1000
    SHAPE=crop   python tools/stage_bwd_bench.py   # 32 x 3 x 256 x 256 (the training crop batch)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from curl_amd import _lib, ops  # noqa: E402

SHAPES = {"frames": (32, 1500, 1000), "crop": (32, 256, 256)}


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def main():
    shape = os.environ.get("SHAPE", "crop")
    B, H, W = SHAPES[shape]
    iters = int(os.environ.get("ITERS", 20))
    _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    img = torch.rand(B, 3, H, W, device=dev, generator=g)
    gout = torch.randn(B, 3, H, W, device=dev, generator=g)
    greg = torch.rand(B, device=dev, generator=g)
    mask = torch.rand(B, 1, H, W, device=dev, generator=g) > 0.2
    L, R, Hk = (torch.randn(B, n, device=dev, generator=g) * 0.1 for n in (48, 48, 64))
    _, _, ws_layer = ops.curl_layer_forward(img, mask, L, R, Hk, return_workspace=True)
    _, _, ws_lab = ops._lab_stage(img, mask, L, return_workspace=True)
    _, _, ws_hsv = ops._hsv_stage(img, mask, Hk, return_workspace=True)
    _, _, ws_rgb = ops._adjust_rgb(img, R, return_workspace=True)
    _, _, ws_ahsv = ops._adjust_hsv(img, Hk, return_workspace=True)
    rows = {
        "layer_bwd (grad_img)": lambda: ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg, True, workspace=ws_layer),
        "lab_stage_bwd": lambda: ops.lab_stage_backward(img, mask, L, gout, greg, workspace=ws_lab),
        "hsv_stage_bwd": lambda: ops.hsv_stage_backward(img, mask, Hk, gout, greg, workspace=ws_hsv),
        "adjust_rgb_bwd": lambda: ops.adjust_rgb_backward(img, R, gout, greg, workspace=ws_rgb),
        "adjust_lab_bwd": lambda: ops.adjust_lab_backward(img, L, gout, greg, workspace=ws_rgb),
        "adjust_hsv_bwd": lambda: ops.adjust_hsv_backward(img, Hk, gout, greg, workspace=ws_ahsv),
        "rgb2lab_bwd": lambda: ops.rgb2lab_backward(img, gout),
        "lab2rgb_bwd": lambda: ops.lab2rgb_backward(img, gout),
        "rgb2hsv_bwd": lambda: ops.rgb2hsv_backward(img, gout),
        "hsv2rgb_bwd": lambda: ops.hsv2rgb_backward(img, gout),
    }
    res = {name: timed(fn, iters) for name, fn in rows.items()}
    px = B * H * W
    for name, us in res.items():
        extra = ""
        if name.startswith(("rgb2", "lab2", "hsv2")):
            extra = f"  {36 * px / (us * 1e-6) / 1e12:.2f} TB/s at 36 B/px ({36 * px / (us * 1e-6) / 8e12 * 100:.0f} % of 8 TB/s)"
        print(f"{shape:6s} {name:32s} {us:9.1f} us/call{extra}")
    print(json.dumps({"shape": [B, H, W], "us_per_call": res}))


if __name__ == "__main__":
    main()
