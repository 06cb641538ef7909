"""Golden vectors for polynomial orders 1-3, produced by RUNNING THE REFERENCE's classes on the inputs of poly.npz.

ChannelPolyLayer(d, V, 3) and the per-pixel methods of TriSpaceRegNet are taken from the reference's source text exactly as
make_golden_poly.py takes them (its reference_classes / make_tri are imported); the coefficient tables are the first n(d, V)
entries of poly.npz's order-4 tables.  Nothing from oracle/ or curl_amd/ is used.  Arrays only.

    python tests/golden/make_golden_poly_orders.py      (build container only)
"""
import math
import os

import numpy as np
import torch

from make_golden_poly import OUT, make_tri, reference_classes


def main():
    ns = reference_classes()
    CPL = ns["ChannelPolyLayer"]
    g = np.load(os.path.join(OUT, "poly.npz"))
    t = lambda name: torch.from_numpy(g[name])  # noqa: E731
    store = {}
    for d in (1, 2, 3):
        n5, n3 = math.comb(5 + d, d), math.comb(3 + d, d)
        store[f"powers_d{d}_v5"] = np.array(list(CPL.generate_powers(d, 5)), dtype=np.int32)
        store[f"powers_d{d}_v3"] = np.array(list(CPL.generate_powers(d, 3)), dtype=np.int32)
        store[f"channel_poly_d{d}v5"] = CPL(degree=d, num_variables=5, num_out=3)(t("x5"), t("c5")[..., :n5].contiguous()).numpy()
        store[f"channel_poly_d{d}v3"] = CPL(degree=d, num_variables=3, num_out=3)(t("x3"), t("c3")[..., :n3].contiguous()).numpy()
        tri5 = make_tri(ns, True, CPL(degree=d, num_variables=5, num_out=3))
        tri3 = make_tri(ns, False, CPL(degree=d, num_variables=3, num_out=3))
        for s in ("s02", "s1"):
            c5 = t(s + "_coeffs")[..., :n5].contiguous()
            c3 = t(s + "_coeffs35")[..., :n3].contiguous()
            for nm in (("img", "img8") if s == "s02" else ("img",)):
                res = tri5.generate_residual(t(nm), c5[:, 0], c5[:, 1], c5[:, 2])
                store[f"{s}_{nm}_residual_d{d}v5"] = res.numpy()
                store[f"{s}_{nm}_image_d{d}v5"] = tri5.generate_image(t(nm), res).numpy()
            res = tri3.generate_residual(t("img"), c3[:, 0], c3[:, 1], c3[:, 2])
            store[f"{s}_img_residual_d{d}v3"] = res.numpy()
            if s == "s02":
                store[f"{s}_img_image_d{d}v3"] = tri3.generate_image(t("img"), res).numpy()
    path = os.path.join(OUT, "poly_orders.npz")
    np.savez_compressed(path, **store)
    print("poly_orders.npz", os.path.getsize(path) // 1024, "KiB,", len(store), "arrays")


if __name__ == "__main__":
    main()
