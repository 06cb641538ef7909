"""Times the file-to-file byte entries against their foreground-aware forms, on the GPU, in one process, alternating:

    A   curl_trispace_fwd_u8hwc / curl_layer_fwd_u8hwc          (white_mask = the mask; RGB bytes)
    B   curl_trispace_fwd_fg_u8hwc / curl_layer_fwd_fg_u8hwc    (fg_mask = the mask; RGB or RGBA bytes)

    python tools/foreground_bench.py [--rounds 9] [--iters 100] [--out profiles/foreground/bench.txt]

8 x 1500x1000 frames (H = 1000, W = 1500).  Models: the polynomial model at 126 and at 35 coefficients, the curve layer
(K = 16).  Masks: all 255 (what the extra wait for the mask costs), bench.disk_mask's disk (~70 % foreground), a smaller disk
(~40 %).  B takes the image as RGB and as RGBA; A always takes RGB (it has no other form: infer.enhance slices the alpha off
on the host first, which is not timed here).  Both go through the C ABI with every buffer allocated beforehand; the input sets
are rotated call by call and together exceed the 256 MiB last-level cache, so no call finds its bytes there.  Each round times
`iters` back-to-back calls between two device events; the two sides take turns round by round.  First A against itself, to
learn the spread a comparison has to beat; then A | B.  Before anything is timed, B's bytes are compared with A's."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from curl_amd import _lib  # noqa: E402

B, H, W = 8, 1000, 1500
N_SETS = 5  # 5 x (36 + 12 + 36 MB) = 420 MB (RGBA: 480 MB) in rotation


def disk(frac_param, dev):
    """bench.disk_mask's ellipse at another radius: d < frac_param covers pi / 4 * frac_param of the frame."""
    yy = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1)
    xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, W)
    d = ((yy - H / 2) / (H / 2)) ** 2 + ((xx - W / 2) / (W / 2)) ** 2
    return (d < frac_param).view(1, H, W).expand(B, H, W).contiguous()


def masks(dev):
    return {"all 255": torch.full((B, H, W), 255, dtype=torch.uint8, device=dev),
            "disk 70 %": bench.disk_mask(B, H, W, dev)[:, 0].to(torch.uint8).mul(255).contiguous(),
            "disk 40 %": disk(0.51, dev).to(torch.uint8).mul(255)}


def make_calls(lib, model, channels, mask, dev, g):
    """-> (call_a(i), call_b(i), out_a, out_b): call i of either side works on input set i % N_SETS"""
    rgba = [torch.randint(0, 256, (B, H, W, 4), generator=g, dtype=torch.uint8, device=dev) for _ in range(N_SETS)]
    rgb = [x[..., :3].contiguous() for x in rgba]
    img_b = rgb if channels == 3 else rgba
    fgs = [mask.clone() for _ in range(N_SETS)]
    out_a = [torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(N_SETS)]
    out_b = [torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(N_SETS)]
    s = torch.cuda.current_stream().cuda_stream
    if model == "layer":
        L, R, Hk = (torch.randn(B, n, generator=g, device=dev) * 0.1 for n in (48, 48, 64))
        nbytes = lib.curl_workspace_bytes(B, 160)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)

        def call_a(i):
            k = i % N_SETS
            return lib.curl_layer_fwd_u8hwc(rgb[k].data_ptr(), 0, 0, L.data_ptr(), R.data_ptr(), Hk.data_ptr(), fgs[k].data_ptr(),
                                            out_a[k].data_ptr(), 0, ws.data_ptr(), nbytes, B, H, W, 16, 16, 16, 0, s)

        def call_b(i):
            k = i % N_SETS
            return lib.curl_layer_fwd_fg_u8hwc(img_b[k].data_ptr(), channels, L.data_ptr(), R.data_ptr(), Hk.data_ptr(), fgs[k].data_ptr(),
                                               out_b[k].data_ptr(), 0, ws.data_ptr(), nbytes, B, H, W, 16, 16, 16, 0, s)
    else:
        nc = int(model)
        c = torch.randn(B, 3, 3, nc, generator=g, device=dev) * 0.2

        def call_a(i):
            k = i % N_SETS
            return lib.curl_trispace_fwd_u8hwc(rgb[k].data_ptr(), c.data_ptr(), fgs[k].data_ptr(), out_a[k].data_ptr(), B, H, W, nc, 0, s)

        def call_b(i):
            k = i % N_SETS
            return lib.curl_trispace_fwd_fg_u8hwc(img_b[k].data_ptr(), channels, c.data_ptr(), fgs[k].data_ptr(), out_b[k].data_ptr(), B, H, W,
                                                  nc, 0, s)
    keep = (rgba, rgb, fgs)  # the closures hold raw addresses: keep the tensors alive with them
    return call_a, call_b, out_a, out_b, keep


def timed(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        rc = call(i)
        if rc != 0:
            sys.exit(f"foreground_bench: return code {rc}: {_lib.load().curl_last_error()}")
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def alternate(f, g, rounds, iters):
    tf, tg = [], []
    for _ in range(rounds):
        tf.append(timed(f, iters))
        tg.append(timed(g, iters))
    return tf, tg


def line(label, t):
    return f"{label:<24} median {statistics.median(t):8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("foreground_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {B} x {W}x{H}; {args.rounds} rounds of {args.iters} calls; us per call of {B} frames"]
    table = ["| model | input of B | mask | A, us | B, us | B / A | A/A spread |", "|---|---|---|---|---|---|---|"]
    for model in ("126", "35", "layer"):
        for channels in (3, 4):
            for mname, mask in masks(dev).items():
                call_a, call_b, out_a, out_b, keep = make_calls(lib, model, channels, mask, dev, g)
                timed(call_a, N_SETS), timed(call_b, N_SETS)  # warm-up, and every output set written once
                same = all(torch.equal(x, y) for x, y in zip(out_a, out_b))
                a1, a2 = alternate(call_a, call_a, args.rounds, args.iters)
                ta, tb = alternate(call_a, call_b, args.rounds, args.iters)
                spread = abs(statistics.median(a1) - statistics.median(a2)) / statistics.median(a1)
                ma, mb = statistics.median(ta), statistics.median(tb)
                name = {"126": "trispace 126", "35": "trispace 35", "layer": "layer K=16"}[model]
                lines += [f"{name}, B reads {'RGB' if channels == 3 else 'RGBA'}, mask {mname} (foreground {float((mask != 0).float().mean()):.3f}); "
                          f"bytes equal: {same}",
                          line("  A (A/A, first)", a1), line("  A (A/A, second)", a2), f"  A/A spread of the medians {100 * spread:.2f} %",
                          line("  A", ta), line("  B", tb), f"  B / A {mb / ma:.3f}"]
                table.append(f"| {name} | {'RGB' if channels == 3 else 'RGBA'} | {mname} | {ma:.1f} | {mb:.1f} | {mb / ma:.3f} | {100 * spread:.2f} % |")
                if not same:
                    sys.exit("\n".join(lines) + "\nforeground_bench: the two entries disagree")
                del call_a, call_b, out_a, out_b, keep
    text = "\n".join(lines + [""] + table)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
