"""Times the criterion (CURLLoss, model.py:78-116) of a folder's worth of differently sized byte images against their targets
through the two routes the package has, on the GPU, in one process, alternating (the method of tools/ragged_msssim_bench.py,
DESIGN.md 3a.5):

    A   the loop that was the only way: per image ops.u8hwc_to_f32chw of the output and of the target and model.CURLLoss() on
        the [1,3,H,W] batch (the terms kernel and its finish, two full-resolution float L planes, ten MS-SSIM launches)
    B   ONE ops.curl_loss_u8hwc_ragged call on the packed arenas (curl_loss_ragged_u8hwc: six launches, level 0 from the bytes)

    python tools/ragged_loss_bench.py [--rounds 7] [--window_ms 100] [--out profiles/ragged_loss/bench.txt]

Batches, input sets, rotation, warm-up and the order A | A, then A | B are tools/ragged_msssim_bench.py's.  A's float masks are
made beforehand from the bytes (`mask != 0`), which is in A's favour; both routes allocate their results and workspaces inside
the timed window.  A's values are held to B's before anything is timed, to 2.5e-4: A's loss is float32 and its MS-SSIM term
enters with weight 10 / 5 -- twice the 1e-4 the MS-SSIM bench allows its two float32 sides -- plus the four pointwise terms at
3e-6 each over 5.  No ratio is fixed in advance: a row counts as won when B's median is below A's by more than A's own
alternating spread, and a row that is not won is printed as it is."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from curl_amd import model, ops  # noqa: E402
from ragged_bench import alternate, batches, line, timed  # noqa: E402
from ragged_score_bench import make_sets  # noqa: E402

AGREE = 2.5e-4


def make_routes(sets, with_masks, dev):
    criterion = model.CURLLoss().to(dev)

    @torch.no_grad()
    def loop(k):
        s = sets[k % len(sets)]
        return [criterion(ops.u8hwc_to_f32chw(o), ops.u8hwc_to_f32chw(t), m if with_masks else None).reshape(1)
                for o, t, m in zip(s["out"], s["tgt"], s["fmask"])]

    def ragged(k):
        s = sets[k % len(sets)]
        return ops.curl_loss_u8hwc_ragged(s["out_arena"], s["tgt_arena"], s["mask_arena"] if with_masks else None)
    return loop, ragged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_loss_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {args.rounds} rounds per side; us per batch (every image of it once)"]
    table = ["| batch | masks | Mpx | loop (A), us | ragged (B), us | B / A | A/A spread | B below A by more than the spread |", "|---|---|---|---|---|---|---|---|"]
    for bname, shapes3 in batches().items():
        shapes = [(h, w) for h, w, _ in shapes3]
        sets = make_sets(shapes, dev, g)
        px = sum(h * w for h, w in shapes)
        for with_masks in (True, False):
            loop, ragged = make_routes(sets, with_masks, dev)
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
            if not worst <= AGREE:
                sys.exit("\n".join(lines) + "\nragged_loss_bench: the two routes disagree")
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
