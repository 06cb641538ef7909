"""Times curl_layer_pwl_bwd_f32 (the fused layer's backward with the paper's piecewise-linear curves), with and without the
image gradient, beside curl_layer_bwd_f32 (the affine form) on the same inputs, each fed the workspace its own forward filled.
Meant to run under `rocprofv3 --kernel-trace --stats` (one shape per process, so that the per-kernel averages belong to it); it
also prints its own event-timed per-call times (kernels + launch gaps) and the PWL / affine ratio.

    SHAPE=frames python tools/pwl_bwd_bench.py   # 32 x 3 x 1500 x 1000
    SHAPE=crop   python tools/pwl_bwd_bench.py   # 32 x 3 x 256 x 256 (the training crop batch)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from curl_amd import _lib, ops  # noqa: E402
from stage_bwd_bench import SHAPES, timed  # noqa: E402


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
    _, _, ws_aff = ops.curl_layer_forward(img, mask, L, R, Hk, return_workspace=True)
    _, _, ws_pwl = ops.curl_layer_forward(img, mask, L, R, Hk, flags=ops.F_PWL, return_workspace=True)
    rows = {
        "layer_bwd (grad_img)": lambda: ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg, True, workspace=ws_aff),
        "layer_bwd (knots only)": lambda: ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg, False, workspace=ws_aff),
        "layer_pwl_bwd (grad_img)": lambda: ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg, True, workspace=ws_pwl,
                                                                    flags=ops.F_PWL),
        "layer_pwl_bwd (knots only)": lambda: ops.curl_layer_backward(img, mask, L, R, Hk, gout, greg, False, workspace=ws_pwl,
                                                                      flags=ops.F_PWL),
    }
    res = {name: timed(fn, iters) for name, fn in rows.items()}
    for name, us in res.items():
        print(f"{shape:6s} {name:28s} {us:9.1f} us/call")
    ratio = {k: res[f"layer_pwl_bwd ({k})"] / res[f"layer_bwd ({k})"] for k in ("grad_img", "knots only")}
    print(json.dumps({"shape": [B, H, W], "us_per_call": res, "pwl_over_affine": ratio}))


if __name__ == "__main__":
    main()
