"""Times the two routes to the encoder's 320x320 view from image bytes, on the GPU, in one process, alternating:

    float   ops.u8hwc_to_f32chw + infer.encoder_view   (full-resolution float image, torch's antialiased interpolate twice)
    pil     ops.encoder_view_u8hwc                     (Pillow's 8-bit resample of the bytes, one launch)

    python tools/encoder_view_bench.py [--rounds 15] [--iters 50] [--out profiles/encoder_view/bench.txt]

Shapes: 1x1500x1000 and 32x1500x1000, with a mask.  Each round times `iters` back-to-back calls of a route between two device
events; the routes take turns round by round.  First the same route against itself (float | float), to learn the spread a
comparison has to beat; then float | pil.  Reported per route: the median round in microseconds per call, and min / max.
The plan of the pil route is uploaded once, before the timed rounds (ops keeps it per shape), as a caller that sees one
camera's frames would have it."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from curl_amd import infer, ops  # noqa: E402


def route_float(img, mask):
    x = ops.u8hwc_to_f32chw(img)
    return infer.encoder_view(x, mask[:, None].float() / 255.0)


def route_pil(img, mask):
    return ops.encoder_view_u8hwc(img, mask)


def timed(fn, img, mask, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn(img, mask)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def alternate(f, g, img, mask, rounds, iters):
    for fn in (f, g):  # warm-up: code objects, the allocator's blocks, the plan
        timed(fn, img, mask, 5)
    tf, tg = [], []
    for _ in range(rounds):
        tf.append(timed(f, img, mask, iters))
        tg.append(timed(g, img, mask, iters))
    return tf, tg


def line(label, t):
    return f"{label:<28} median {statistics.median(t):9.1f} us  min {min(t):9.1f}  max {max(t):9.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encoder_view_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {args.rounds} rounds; us per call"]
    for B in (1, 32):
        img = torch.randint(0, 256, (B, 1500, 1000, 3), generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
        mask = (torch.rand(B, 1500, 1000, generator=g) > 0.4).to(torch.uint8).mul(255).to(dev)
        iters = max(4, args.iters // (8 if B > 1 else 1))
        a1, a2 = alternate(route_float, route_float, img, mask, args.rounds, iters)
        f, p = alternate(route_float, route_pil, img, mask, args.rounds, iters)
        spread = abs(statistics.median(a1) - statistics.median(a2))
        lines += [f"{B}x1500x1000 + mask ({iters} calls per round)", line("  float (A/A, first)", a1), line("  float (A/A, second)", a2),
                  f"  A/A spread of the medians {spread:9.1f} us", line("  float", f), line("  pil", p),
                  f"  pil / float {statistics.median(p) / statistics.median(f):.3f}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
