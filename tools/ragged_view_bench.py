"""Times the 320x320 encoder views of a folder's worth of differently sized byte images through the two routes the package
has, on the GPU, in one process, alternating:

    A   the loop infer.enhance_many ran before the ragged view: one ops.encoder_view_u8hwc call per image, then torch.cat
    B   ONE call on the packed arenas: ops.encoder_view_u8hwc_ragged

    python tools/ragged_view_bench.py [--rounds 7] [--window_ms 100] [--out profiles/ragged/view_bench.txt]

Batches: tools/ragged_bench.py's three -- 32 x 512x341 RGBA (A gets the RGB bytes, sliced beforehand and not timed, as
enhance_many sliced them on the host; B the RGBA arena), 32 shapes drawn with a fixed seed between 0.2 and 6 Mpx in both
orientations (RGB), 8 x 1500x1000 (RGB) --, with masks, size 320.  Every input is on the device before anything is timed and
every plan is warm: A's cache of uploaded plans is widened to hold the 32 shapes of the mixed batch (at the package's sixteen
every call of that batch would rebuild and upload its plan -- in A's disfavour).  Both routes allocate their outputs inside the
timed window, as a caller's would.  The input sets are rotated call by call and together exceed the 256 MiB last-level cache.
Each round times `iters` back-to-back calls of one route between two device events (iters: what fills --window_ms, found by a
calibration run); the routes take turns round by round.  First A against itself, to learn the spread a comparison has to
beat; then A | B.  Every shape is warmed up and B's bits are compared with A's before anything is timed.  The figures are
times per batch as a caller sees them on a busy queue: host time of the calls included wherever the device waits for it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from curl_amd import _lib, ops  # noqa: E402
from ragged_bench import LLC_BYTES, alternate, batches, line, timed  # noqa: E402

SIZE = 320


def make_sets(shapes, dev, g):
    per_set = sum(h * w * (c + 1) for h, w, c in shapes)
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


def make_routes(sets):
    def loop(k):
        s = sets[k % len(sets)]
        views = [ops.encoder_view_u8hwc(x, m, size=SIZE) for x, m in zip(s["rgb"], s["white"])]
        return torch.cat([v for v, _ in views]), torch.cat([m for _, m in views])

    def ragged(k):
        s = sets[k % len(sets)]
        return ops.encoder_view_u8hwc_ragged(s["arena"], s["mask_arena"], size=SIZE)
    return loop, ragged


def plan_facts(shapes):
    """What the ragged plan says of the batch: workgroups, the launch's LDS and the smallest image's, distinct tables."""
    plan = ops._view_ragged_plan([(h, w) for h, w, _ in shapes], [c for _, _, c in shapes], True, SIZE, torch.device("cuda:0"))
    w = plan.host.numpy()
    hw, dw = _lib.VIEW_RAGGED_HEADER_WORDS, _lib.VIEW_RAGGED_DESC_WORDS
    lds = w[hw:hw + len(shapes) * dw].reshape(len(shapes), dw)[:, 15]
    return f"grid {int(w[4])} workgroups, LDS per workgroup {int(w[5])} B (smallest image's own: {int(lds.min())} B), {int(w[6])} distinct tables, plan {plan.nbytes} B"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_view_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    ops._VIEW_PLANS_KEPT = 64  # A's plans stay warm over the 32 shapes of the mixed batch
    g = torch.Generator(device=dev).manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {args.rounds} rounds per side; us per batch (every image's {SIZE}x{SIZE} view and mask view once)"]
    table = ["| batch | Mpx | loop + cat (A), us | ragged (B), us | B / A | A/A spread |", "|---|---|---|---|---|---|"]
    for bname, shapes in batches().items():
        sets = make_sets(shapes, dev, g)
        mpx = sum(h * w for h, w, _ in shapes) / 1e6
        loop, ragged = make_routes(sets)
        same = True
        for k in range(len(sets)):  # warm-up of every shape and set on both routes, and the comparison
            (va, ma), (vb, mb) = loop(k), ragged(k)
            same = same and torch.equal(va, vb) and torch.equal(ma, mb)
        torch.cuda.synchronize()
        iters = max(3, int(args.window_ms * 1e3 / max(timed(loop, 3), 1.0)))
        a1, a2 = alternate(loop, loop, args.rounds, iters)
        ta, tb = alternate(loop, ragged, args.rounds, iters)
        spread = abs(statistics.median(a1) - statistics.median(a2)) / statistics.median(a1)
        ma_, mb_ = statistics.median(ta), statistics.median(tb)
        lines += [f"{bname} ({mpx:.1f} Mpx, {len(sets)} input sets in rotation), {iters} calls per round; bits equal: {same}",
                  f"  ragged plan: {plan_facts(shapes)}",
                  line("  A (A/A, first)", a1), line("  A (A/A, second)", a2), f"  A/A spread of the medians {100 * spread:.2f} %",
                  line("  A loop + cat", ta), line("  B ragged", tb), f"  B / A {mb_ / ma_:.3f}"]
        table.append(f"| {bname} | {mpx:.1f} | {ma_:.1f} | {mb_:.1f} | {mb_ / ma_:.3f} | {100 * spread:.2f} % |")
        if not same:
            sys.exit("\n".join(lines) + "\nragged_view_bench: the two routes disagree")
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
