"""Times the MS-SSIM of a folder's worth of differently sized byte images against their targets through the two routes the
package has, on the GPU, in one process, alternating (the method of tools/ragged_score_bench.py):

    A   the loop that was the only way: per image ops.u8hwc_to_f32chw of the output and of the target, the two mask
        multiplies, ops.msssim_stats (ten launches) and metric.py:200-207 on its statistics
    B   ONE ops.msssim_u8hwc_ragged call on the packed arenas (curl_msssim_ragged_u8hwc: six launches, level 0 from the bytes)

    python tools/ragged_msssim_bench.py [--rounds 7] [--window_ms 100] [--out profiles/ragged_msssim/bench.txt]

Batches: tools/ragged_bench.py's three (32 x 512x341, 32 shapes between 0.2 and 6 Mpx, 8 x 1500x1000), as RGB, each with and
without masks (random bytes, the top third 0).  Every input is on the device before anything is timed -- A's float masks too,
made beforehand from the bytes (`mask != 0`), which is in A's favour; both routes allocate their results and workspaces inside
the timed window.  The input sets are rotated call by call and together exceed the 256 MiB last-level cache.  Each round times
`iters` back-to-back calls of one route between two device events; the routes take turns round by round.  Every shape is
warmed up and A's values are held to B's (1e-4: A's statistics are float32, two sides of at most 2.2e-5 on random content
times the formula's weights, which sum to under 1.4) before anything is timed; then A against itself, to learn the spread a
comparison has to beat; then A | B.  No ratio is fixed in advance: a row counts as won when B's median is below A's by more
than A's own alternating spread, and a row that is not won is printed as it is."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from curl_amd import ops  # noqa: E402
from ragged_bench import alternate, batches, line, timed  # noqa: E402
from ragged_score_bench import make_sets  # noqa: E402


def make_routes(sets, with_masks):
    def loop(k):
        s = sets[k % len(sets)]
        out = []
        for o, t, m in zip(s["out"], s["tgt"], s["fmask"]):
            fo, ft = ops.u8hwc_to_f32chw(o), ops.u8hwc_to_f32chw(t)
            if with_masks:
                fo, ft = fo * m, ft * m
            ssims, mcs = ops.msssim_stats(ft, fo)
            out.append(ops.msssim_from_stats(torch.stack((ssims, mcs), 1)))
        return out

    def ragged(k):
        s = sets[k % len(sets)]
        return ops.msssim_u8hwc_ragged(s["tgt_arena"], s["out_arena"], s["mask_arena"] if with_masks else None)
    return loop, ragged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_msssim_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {args.rounds} rounds per side; us per batch (every image of it once)"]
    table = ["| batch | masks | Mpx | loop (A), us | ragged (B), us | B / A | A/A spread | B below A by more than the spread |", "|---|---|---|---|---|---|---|---|"]
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
            won = "yes" if mb < ma * (1 - spread) else "NO"
            mname = "masks" if with_masks else "no masks"
            name = bname.replace(" RGBA", "")
            lines += [f"{name} ({px / 1e6:.1f} Mpx, {len(sets)} input sets in rotation), {mname}, {iters} calls per round; largest |A - B| {worst:.2e}",
                      line("  A (A/A, first)", a1), line("  A (A/A, second)", a2), f"  A/A spread of the medians {100 * spread:.2f} %",
                      line("  A loop", ta), line("  B ragged", tb), f"  B / A {mb / ma:.3f}; B below A by more than the spread: {won}"]
            table.append(f"| {name} | {mname} | {px / 1e6:.1f} | {ma:.1f} | {mb:.1f} | {mb / ma:.3f} | {100 * spread:.2f} % | {won} |")
            if not worst <= 1e-4:
                sys.exit("\n".join(lines) + "\nragged_msssim_bench: the two routes disagree")
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
