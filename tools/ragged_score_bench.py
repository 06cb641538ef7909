"""Times the masked PSNR of a folder's worth of differently sized byte images against their targets through the two routes
the package has, on the GPU, in one process, alternating:

    A   the loop that was the only way: per image ops.u8hwc_to_f32chw of the output and of the target, then
        ops.psnr_per_image with the float mask (four launches and 24 bytes of float image per pixel, per image)
    B   ONE ops.psnr_u8hwc_ragged call on the packed arenas (curl_sse_ragged_u8hwc: 7 bytes per pixel, integers)

    python tools/ragged_score_bench.py [--rounds 7] [--window_ms 100] [--out profiles/ragged_score/bench.txt]

Batches: tools/ragged_bench.py's three (32 x 512x341, 32 shapes between 0.2 and 6 Mpx, 8 x 1500x1000), as RGB, each with and
without masks (random bytes, the top third 0).  Every input is on the device before anything is timed -- A's float masks too,
made beforehand from the bytes (`mask != 0`), which is in A's favour; both routes allocate their results inside the timed
window.  The input sets are rotated call by call and together exceed the 256 MiB last-level cache.  Each round times `iters`
back-to-back calls of one route between two device events; the routes take turns round by round.  First A against itself, to
learn the spread a comparison has to beat; then A | B.  Every shape is warmed up and A's values are held to B's (2e-3 dB: A's
float32 sums) before anything is timed.  B's rate is the bytes it must move (7 per pixel, 6 without masks) over the time of the
whole call -- its three launches and the handful of torch launches that turn the integers into dB --, not a kernel's."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from curl_amd import ops  # noqa: E402
from ragged_bench import LLC_BYTES, alternate, batches, line, timed  # noqa: E402


def make_sets(shapes, dev, g):
    per_set = sum(h * w * 7 for h, w in shapes)
    n_sets = max(2, -(-LLC_BYTES // per_set) + 1)
    sets = []
    for _ in range(n_sets):
        outs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8, device=dev) for h, w in shapes]
        tgts = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8, device=dev) for h, w in shapes]
        masks = [torch.randint(0, 256, (h, w), generator=g, dtype=torch.uint8, device=dev) for h, w in shapes]
        for m in masks:
            m[: m.shape[0] // 3] = 0
        sets.append(dict(out=[x[None] for x in outs], tgt=[x[None] for x in tgts], fmask=[(m != 0).float()[None, None] for m in masks],
                         out_arena=ops.RaggedBytes.pack(outs, dev), tgt_arena=ops.RaggedBytes.pack(tgts, dev),
                         mask_arena=ops.RaggedBytes.pack(masks, dev)))
    return sets


def make_routes(sets, with_masks):
    def loop(k):
        s = sets[k % len(sets)]
        return [ops.psnr_per_image(ops.u8hwc_to_f32chw(o), ops.u8hwc_to_f32chw(t), m if with_masks else None)
                for o, t, m in zip(s["out"], s["tgt"], s["fmask"])]

    def ragged(k):
        s = sets[k % len(sets)]
        return ops.psnr_u8hwc_ragged(s["out_arena"], s["tgt_arena"], s["mask_arena"] if with_masks else None)
    return loop, ragged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_score_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {args.rounds} rounds per side; us per batch (every image of it once)"]
    table = ["| batch | masks | Mpx | loop (A), us | ragged (B), us | B / A | A/A spread | B, GB/s of its 7 (6) B/px |", "|---|---|---|---|---|---|---|---|"]
    for bname, shapes3 in batches().items():
        shapes = [(h, w) for h, w, _ in shapes3]
        sets = make_sets(shapes, dev, g)
        px = sum(h * w for h, w in shapes)
        for with_masks in (True, False):
            loop, ragged = make_routes(sets, with_masks)
            worst = 0.0
            for k in range(len(sets)):  # warm-up of every shape and set on both routes, and the comparison
                want, got = torch.cat(loop(k)).double(), ragged(k)
                worst = max(worst, float((want - got).abs().max()))
            torch.cuda.synchronize()
            iters = max(3, int(args.window_ms * 1e3 / max(timed(loop, 3), 1.0)))
            a1, a2 = alternate(loop, loop, args.rounds, iters)
            ta, tb = alternate(loop, ragged, args.rounds, iters)
            spread = abs(statistics.median(a1) - statistics.median(a2)) / statistics.median(a1)
            ma, mb = statistics.median(ta), statistics.median(tb)
            rate = px * (7 if with_masks else 6) / (mb * 1e-6) / 1e9
            mname = "masks" if with_masks else "no masks"
            lines += [f"{bname.replace(' RGBA', '')} ({px / 1e6:.1f} Mpx, {len(sets)} input sets in rotation), {mname}, {iters} calls per round; "
                      f"largest |A - B| {worst:.2e} dB",
                      line("  A (A/A, first)", a1), line("  A (A/A, second)", a2), f"  A/A spread of the medians {100 * spread:.2f} %",
                      line("  A loop", ta), line("  B ragged", tb), f"  B / A {mb / ma:.3f}; B moves {rate:.0f} GB/s of the bytes it must read"]
            table.append(f"| {bname.replace(' RGBA', '')} | {mname} | {px / 1e6:.1f} | {ma:.1f} | {mb:.1f} | {mb / ma:.3f} | {100 * spread:.2f} % | {rate:.0f} |")
            if not worst <= 2e-3:
                sys.exit("\n".join(lines) + "\nragged_score_bench: the two routes disagree")
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
