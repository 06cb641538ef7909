"""Times a folder's worth of differently sized byte images through the two routes the package has, on the GPU, in one process,
alternating:

    A   a Python loop, one call per image: ops.trispace_forward_u8hwc (the compiled binding) / ops.curl_layer_forward_u8hwc
    B   ONE ragged call on the packed arenas: ops.trispace_forward_u8hwc_ragged / ops.curl_layer_forward_u8hwc_ragged

    python tools/ragged_bench.py [--rounds 7] [--window_ms 100] [--out profiles/ragged/bench.txt]

Batches: 32 x 512x341 RGBA (the reference's example size; A gets the RGB bytes, sliced beforehand and not timed, B the RGBA
arena), 32 shapes drawn with a fixed seed between 0.2 and 6 Mpx in both orientations (RGB), 8 x 1500x1000 (RGB).  Models: the
126-coefficient polynomial model and the curve layer (K = 16), both with white masks.  Every input is on the device before
anything is timed; both routes allocate their outputs inside the timed window, as a caller's would.  The input sets are
rotated call by call and together exceed the 256 MiB last-level cache.  Each round times `iters` back-to-back calls of one
route between two device events (iters: what fills --window_ms, found by a calibration run); the routes take turns round by
round.  First A against itself, to learn the spread a comparison has to beat; then A | B.  Every shape is warmed up and B's
bytes are compared with A's before anything is timed."""
import argparse
import os
import random
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from curl_amd import ops  # noqa: E402

LLC_BYTES = 256 << 20


def batches():
    rng = random.Random(20)
    mixed = []
    for k in range(32):
        mpx = rng.uniform(0.2, 6.0)
        aspect = rng.choice((1.5, 4 / 3, 16 / 9))
        short = max(8, int(round((mpx * 1e6 / aspect) ** 0.5)))
        long = int(round(short * aspect))
        mixed.append((short, long, 3) if k % 2 else (long, short, 3))  # both orientations
    return {"32 x 512x341 RGBA": [(341, 512, 4)] * 16 + [(512, 341, 4)] * 16,
            "32 mixed 0.2-6 Mpx": mixed,
            "8 x 1500x1000": [(1000, 1500, 3)] * 8}


def make_sets(shapes, dev, g):
    per_set = sum(h * w * (c + 1 + 3) for h, w, c in shapes)
    n_sets = max(2, -(-LLC_BYTES // per_set) + 1)
    sets = []
    for _ in range(n_sets):
        imgs = [torch.randint(0, 256, (h, w, c), generator=g, dtype=torch.uint8, device=dev) for h, w, c in shapes]
        masks = [torch.randint(0, 256, (h, w), generator=g, dtype=torch.uint8, device=dev) for h, w, _ in shapes]
        for m in masks:
            m[: m.shape[0] // 3] = 0
        sets.append(dict(rgb=[x[None, ..., :3].contiguous() for x in imgs], white=[m[None] for m in masks],
                         arena=ops.RaggedBytes.pack(imgs, dev), mask_arena=ops.RaggedBytes.pack(masks, dev)))
    return sets


def make_routes(model, sets, B, dev, g):
    if model == "layer":
        L, R, Hk = (torch.randn(B, n, generator=g, device=dev) * 0.1 for n in (48, 48, 64))
        rows = [(L[i:i + 1], R[i:i + 1], Hk[i:i + 1]) for i in range(B)]

        def loop(k):
            s = sets[k % len(sets)]
            return [ops.curl_layer_forward_u8hwc(x, None, *rows[i], m)[0] for i, (x, m) in enumerate(zip(s["rgb"], s["white"]))]

        def ragged(k):
            s = sets[k % len(sets)]
            return ops.curl_layer_forward_u8hwc_ragged(s["arena"], L, R, Hk, s["mask_arena"])[0]
    else:
        c = torch.randn(B, 3, 3, 126, generator=g, device=dev) * 0.2
        rows = [c[i:i + 1] for i in range(B)]

        def loop(k):
            s = sets[k % len(sets)]
            return [ops.trispace_forward_u8hwc(x, rows[i], m) for i, (x, m) in enumerate(zip(s["rgb"], s["white"]))]

        def ragged(k):
            s = sets[k % len(sets)]
            return ops.trispace_forward_u8hwc_ragged(s["arena"], c, s["mask_arena"])
    return loop, ragged


def timed(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        call(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per batch


def alternate(f, g, rounds, iters):
    tf, tg = [], []
    for _ in range(rounds):
        tf.append(timed(f, iters))
        tg.append(timed(g, iters))
    return tf, tg


def line(label, t):
    return f"{label:<24} median {statistics.median(t):9.1f} us  min {min(t):9.1f}  max {max(t):9.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {args.rounds} rounds per side; us per batch (every image of it once)"]
    table = ["| batch | model | Mpx | loop (A), us | ragged (B), us | B / A | A/A spread |", "|---|---|---|---|---|---|---|"]
    for bname, shapes in batches().items():
        B = len(shapes)
        sets = make_sets(shapes, dev, g)
        mpx = sum(h * w for h, w, _ in shapes) / 1e6
        for model in ("126", "layer"):
            loop, ragged = make_routes(model, sets, B, dev, g)
            same = True
            for k in range(len(sets)):  # warm-up of every shape and set on both routes, and the comparison
                want, got = loop(k), ragged(k)
                same = same and all(torch.equal(w[0], o) for w, o in zip(want, got.images()))
            torch.cuda.synchronize()
            iters = max(3, int(args.window_ms * 1e3 / max(timed(loop, 3), 1.0)))
            a1, a2 = alternate(loop, loop, args.rounds, iters)
            ta, tb = alternate(loop, ragged, args.rounds, iters)
            spread = abs(statistics.median(a1) - statistics.median(a2)) / statistics.median(a1)
            ma, mb = statistics.median(ta), statistics.median(tb)
            name = {"126": "trispace 126", "layer": "layer K=16"}[model]
            lines += [f"{bname} ({mpx:.1f} Mpx, {len(sets)} input sets in rotation), {name}, {iters} calls per round; bytes equal: {same}",
                      line("  A (A/A, first)", a1), line("  A (A/A, second)", a2), f"  A/A spread of the medians {100 * spread:.2f} %",
                      line("  A loop", ta), line("  B ragged", tb), f"  B / A {mb / ma:.3f}"]
            table.append(f"| {bname} | {name} | {mpx:.1f} | {ma:.1f} | {mb:.1f} | {mb / ma:.3f} | {100 * spread:.2f} % |")
            if not same:
                sys.exit("\n".join(lines) + "\nragged_bench: the two routes disagree")
        del sets
        torch.cuda.empty_cache()
    text = "\n".join(lines + [""] + table)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
