"""Per-order timing of the fused polynomial forward: each order's own kernel (B) against the way the same result was had
before it existed, the order-4 kernel on the zero-padded table (A).  One process, one GPU, alternating rounds in the manner
of tools/ab.py (the per-round difference cancels the board's drift); the inputs rotate through more bytes than the MALL holds.

    python tools/poly_orders_bench.py [f32|u8]          B, H, W, ROUNDS, LAUNCHES from the environment (8, 1000, 1500, 9, 20)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curl_amd import _lib, ops  # noqa: E402


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "f32"
    B, H, W = int(os.environ.get("B", 8)), int(os.environ.get("H", 1000)), int(os.environ.get("W", 1500))
    rounds, launches = int(os.environ.get("ROUNDS", 9)), int(os.environ.get("LAUNCHES", 20))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    # 4 input sets + 1 output: f32 144 MB per set (5 x 144 MB against a 256 MB MALL); bytes 36 MB per set -> 8 sets
    nset = 4 if what == "f32" else 8
    if what == "f32":
        imgs = [torch.rand(B, 3, H, W, device=dev) for _ in range(nset)]
        outs = [torch.empty_like(imgs[0]) for _ in range(2)]
    else:
        imgs = [torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(nset)]
        outs = [torch.empty_like(imgs[0]) for _ in range(nset)]
    cnt = [0]

    def launch(table, nc_arg):
        cnt[0] += 1
        img, out = imgs[cnt[0] % nset], outs[cnt[0] % len(outs)]
        if what == "f32":
            rc = lib.curl_trispace_fwd_f32(img.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W, nc_arg, 0, stream)
        else:
            rc = lib.curl_trispace_fwd_u8hwc(img.data_ptr(), table.data_ptr(), 0, out.data_ptr(), B, H, W, nc_arg, 0, stream)
        assert rc == 0, (rc, lib.curl_last_error())

    print(f"{what}: B={B} H={H} W={W}, {rounds} rounds x {launches} launches; A = order-4 kernel on the zero-padded table, B = the order's own kernel")
    print("order vars coeffs |   A us     B us   B / A   per-round B vs A: median (quartiles)")
    for V in (5, 3):
        for d in (4, 3, 2, 1):
            n = ops.POLY_COEFFS[V][d - 1]
            c = torch.randn(B, 3, 3, n, device=dev) * 0.2
            pad = ops._pad_order4(c, ops.POLY_COEFFS[V][3]).contiguous()
            legs = {"A": (pad, pad.shape[3]), "B": (c, ops._nc_arg(n))}
            times = {"A": [], "B": []}
            for _ in range(30):
                launch(*legs["A"])
            torch.cuda.synchronize()
            for r in range(rounds):
                for k in (("A", "B") if r % 2 == 0 else ("B", "A")):
                    for _ in range(5):
                        launch(*legs[k])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(launches):
                        launch(*legs[k])
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) / launches * 1e3)
            diffs = sorted((b - a) / a * 100 for a, b in zip(times["A"], times["B"]))
            ma, mb = sorted(times["A"])[rounds // 2], sorted(times["B"])[rounds // 2]
            print(f"  {d}    {V}    {n:4d}  | {ma:7.1f}  {mb:7.1f}  {mb / ma:6.3f}   {diffs[len(diffs) // 2]:+6.2f} % "
                  f"({diffs[len(diffs) // 4]:+.2f} .. {diffs[3 * len(diffs) // 4]:+.2f})")


if __name__ == "__main__":
    main()
