"""Times the ragged byte entries against their foreground-aware forms, on the GPU, in one process, alternating:

    A   curl_trispace_fwd_ragged_u8hwc / curl_layer_fwd_ragged_u8hwc        (the mask arena as the white masks)
    B   curl_trispace_fwd_ragged_fg_u8hwc / curl_layer_fwd_ragged_fg_u8hwc  (the same mask arena)

    python tools/ragged_fg_bench.py [--rounds 7] [--window_ms 100] [--batch 0|1|2] [--out profiles/ragged_fg/bench.txt]

Batches (tools/ragged_bench.py's three): 32 x 512x341 RGBA, 32 shapes drawn with a fixed seed between 0.2 and 6 Mpx in both
orientations (RGB), 8 x 1500x1000 (RGB).  Models: the 126-coefficient polynomial model and the curve layer (K = 16).  Masks,
per image: all 255 (what the vote and the later pixel loads cost), a centred ellipse over ~70 % of the image
(tools/foreground_bench.py's disk at each image's H and W) and one over ~40 %.  Both sides go through the C ABI with the SAME
uploaded plan and the same device-resident arenas; every buffer is allocated beforehand; the input sets are rotated call by
call and together exceed the 256 MiB last-level cache.  Each round times `iters` back-to-back calls of one side between two
device events (iters: what fills --window_ms, found by a calibration run); the sides take turns round by round.  First A
against itself, to learn the spread a comparison has to beat; then A | B.  Before anything is timed, B's bytes are compared
with A's (the out arenas are zeroed first: their padding is never written).

On a shared machine run one batch per process, each under a time limit of its own:
    timeout -k 10 300 python tools/ragged_fg_bench.py --batch 0 --out b0.txt && timeout -k 10 300 python ... --batch 1 ..."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_bench  # noqa: E402  (the three batches)
from curl_amd import _lib, ops  # noqa: E402

LLC_BYTES = 256 << 20
MASKS = {"all 255": None, "ellipse 70 %": 0.9, "ellipse 40 %": 0.51}  # d < p covers pi / 4 * p of the image


def ellipse(h, w, p, dev):
    """foreground_bench.disk at this image's H and W: 255 inside the centred ellipse d < p, 0 outside; p None: all 255."""
    if p is None:
        return torch.full((h, w), 255, dtype=torch.uint8, device=dev)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(h, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, w)
    d = ((yy - h / 2) / (h / 2)) ** 2 + ((xx - w / 2) / (w / 2)) ** 2
    return (d < p).to(torch.uint8).mul(255).contiguous()


def plan_of(lib, shapes, nc, dev):
    """-> (host plan int32, its upload, (img, mask, out) arena bytes): curl_ragged_plan with has_mask = 1."""
    B = len(shapes)
    hs, ws, cs = (np.ascontiguousarray([s[k] for s in shapes], dtype=np.int32) for k in range(3))
    nbytes = lib.curl_ragged_plan_bytes(B, nc)
    host = torch.zeros(nbytes // 4, dtype=torch.int32)
    _lib.check(lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, 1, nc, host.data_ptr(), nbytes), "curl_ragged_plan")
    sizes = [int(v) for v in np.ascontiguousarray(host.numpy()[12:18]).view(np.int64)]
    return host, host.to(dev), sizes


def make_calls(lib, model, shapes, sets, mask_arenas, dev, g):
    """-> (call_a(i), call_b(i), out_a, out_b, keep): call i of either side works on input set i % len(sets)."""
    B, n = len(shapes), len(sets)
    nc = 0 if model == "layer" else int(model)
    host, plan_dev, (img_bytes, mask_bytes, out_bytes) = plan_of(lib, shapes, nc, dev)
    assert all(a.numel() == img_bytes for a in sets) and all(m.numel() == mask_bytes for m in mask_arenas)
    out_a = [torch.zeros(out_bytes, dtype=torch.uint8, device=dev) for _ in range(n)]
    out_b = [torch.zeros(out_bytes, dtype=torch.uint8, device=dev) for _ in range(n)]
    s = torch.cuda.current_stream().cuda_stream
    if model == "layer":
        L, R, Hk = (torch.randn(B, k, generator=g, device=dev) * 0.1 for k in (48, 48, 64))
        nbytes = lib.curl_workspace_bytes(B, 160)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        keep = (host, plan_dev, L, R, Hk, ws)

        def call(fn, outs, i):
            k = i % n
            return fn(sets[k].data_ptr(), img_bytes, L.data_ptr(), R.data_ptr(), Hk.data_ptr(), mask_arenas[k].data_ptr(), mask_bytes,
                      outs[k].data_ptr(), out_bytes, 0, ws.data_ptr(), nbytes, host.data_ptr(), plan_dev.data_ptr(), host.numel() * 4,
                      16, 16, 16, 0, s)
        fa, fb = lib.curl_layer_fwd_ragged_u8hwc, lib.curl_layer_fwd_ragged_fg_u8hwc
    else:
        c = torch.randn(B, 3, 3, nc, generator=g, device=dev) * 0.2
        keep = (host, plan_dev, c)

        def call(fn, outs, i):
            k = i % n
            return fn(sets[k].data_ptr(), img_bytes, c.data_ptr(), mask_arenas[k].data_ptr(), mask_bytes, outs[k].data_ptr(), out_bytes,
                      host.data_ptr(), plan_dev.data_ptr(), host.numel() * 4, nc, 0, s)
        fa, fb = lib.curl_trispace_fwd_ragged_u8hwc, lib.curl_trispace_fwd_ragged_fg_u8hwc
    return (lambda i: call(fa, out_a, i)), (lambda i: call(fb, out_b, i)), out_a, out_b, keep


def timed(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        rc = call(i)
        if rc != 0:
            sys.exit(f"ragged_fg_bench: return code {rc}: {_lib.load().curl_last_error()}")
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
    ap.add_argument("--batch", type=int, default=None, choices=(0, 1, 2), help="one of the three batches (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_fg_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(1)
    lines = [f"device {torch.cuda.get_device_name(dev)}; {args.rounds} rounds per side; us per batch (every image of it once)"]
    table = ["| batch | model | mask | foreground | ragged (A), us | foreground ragged (B), us | B / A | A/A spread |", "|---|---|---|---|---|---|---|---|"]
    for number, (bname, shapes) in enumerate(ragged_bench.batches().items()):
        if args.batch is not None and number != args.batch:
            continue
        per_set = sum(h * w * (c + 1 + 3 + 3) for h, w, c in shapes)  # image, mask, both sides' outputs
        n_sets = max(2, -(-LLC_BYTES // per_set) + 1)
        sets = [ops.RaggedBytes.pack([torch.randint(0, 256, (h, w, c), generator=g, dtype=torch.uint8, device=dev) for h, w, c in shapes], dev).arena
                for _ in range(n_sets)]
        mpx = sum(h * w for h, w, _ in shapes) / 1e6
        for mname, p in MASKS.items():
            per_image = [ellipse(h, w, p, dev) for h, w, _ in shapes]
            foreground = sum(int((m != 0).sum()) for m in per_image) / (mpx * 1e6)
            mask_arenas = [ops.RaggedBytes.pack(per_image, dev).arena for _ in range(n_sets)]  # a copy per set: rotated with it
            for model in ("126", "layer"):
                call_a, call_b, out_a, out_b, keep = make_calls(lib, model, shapes, sets, mask_arenas, dev, g)
                timed(call_a, n_sets), timed(call_b, n_sets)  # warm-up, and every output set written once
                same = all(torch.equal(x, y) for x, y in zip(out_a, out_b))
                iters = max(3, int(args.window_ms * 1e3 / max(timed(call_a, 3), 1.0)))
                a1, a2 = alternate(call_a, call_a, args.rounds, iters)
                ta, tb = alternate(call_a, call_b, args.rounds, iters)
                spread = abs(statistics.median(a1) - statistics.median(a2)) / statistics.median(a1)
                ma, mb = statistics.median(ta), statistics.median(tb)
                name = {"126": "trispace 126", "layer": "layer K=16"}[model]
                lines += [f"{bname} ({mpx:.1f} Mpx, {n_sets} input sets in rotation), {name}, mask {mname} (foreground {foreground:.3f}), "
                          f"{iters} calls per round; bytes equal: {same}",
                          line("  A (A/A, first)", a1), line("  A (A/A, second)", a2), f"  A/A spread of the medians {100 * spread:.2f} %",
                          line("  A ragged", ta), line("  B foreground ragged", tb), f"  B / A {mb / ma:.3f}"]
                table.append(f"| {bname} | {name} | {mname} | {foreground:.2f} | {ma:.1f} | {mb:.1f} | {mb / ma:.3f} | {100 * spread:.2f} % |")
                if not same:
                    sys.exit("\n".join(lines) + "\nragged_fg_bench: the two entries disagree")
                del call_a, call_b, out_a, out_b, keep
            del mask_arenas
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
