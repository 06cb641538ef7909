"""Golden vectors for tests/test_oracle_vs_reference.py, test_host_logic.py and test_checkpoint_compat.py by RUNNING THE REFERENCE.

Run in the build container only (needs /root/reference, which never travels):

    python tests/golden/make_golden_vs_reference.py

The inputs are the test modules' own builders (apply_curve_cases, convert_state_input, ...), so the stored outputs belong to
exactly the inputs the tests rebuild.  Every array written is the output of the reference's own code on them:
  curves.apply_curve          /root/reference/curves.py:4-38   (also: whether it hands back the regulariser it was given)
  colors.RGB2LAB/LAB2RGB/...  /root/reference/colors.py         (also: whether a converter modifies its input)
  curves.adjust_*             the exception each wrapper raises
  metric.PSNRMetric           /root/reference/metric.py:28-72
  transpose.swapimdims_*      /root/reference/transpose.py
  colors.RGB2LAB/... state    the constants the converter modules hold
  convert_state.convert_state_dict   on test_host_logic.py's state dict (convert_state_input)
  TriSpaceRegNet              the attribute names its constructor registers (model.py:451-484), read from the source
Nothing from oracle/ or curl_amd/ is used for the outputs.
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CURL_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
import colors  # noqa: E402
import convert_state  # noqa: E402
import curves  # noqa: E402
import metric  # noqa: E402
import transpose  # noqa: E402

sys.path.remove(REF)
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]
import test_host_logic as TH  # noqa: E402  (the input builders only)
import test_oracle_vs_reference as T  # noqa: E402

torch.set_num_threads(1)


def golden(name):
    return np.load(os.path.join(HERE, name + ".npz"))


def npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)


def main():
    store = {}
    for K in T.K_LIST:
        for key, x, C, r0, ci, co in T.apply_curve_cases(K):
            out, reg = curves.apply_curve(x, C, r0.clone(), ci, co)
            store[key + "_out"], store[key + "_reg"] = npy(out), npy(reg)

    x, C = T.in_place_inputs()
    r1 = torch.zeros(1)
    _, out1 = curves.apply_curve(x, C, r1, 0, 0)
    store["inplace_returns_input"] = np.array(out1 is r1)
    store["inplace_reg"] = npy(r1)

    for name, _ in T.CONVERTERS:
        mod = getattr(colors, name)()
        modified = False
        for i, x in enumerate(T.converter_inputs(golden)):
            keep = x.clone()
            store[f"conv_{name}_{i}"] = npy(mod(x))
            modified |= not torch.equal(x, keep)
        store[f"conv_{name}_modifies_input"] = np.array(modified)

    raised = []
    x = T.rnd(0, 1, 3, 4, 4)
    for fn, n in T.WRAPPERS:
        try:
            getattr(curves, fn)(x, torch.zeros(1, n))
            raised.append("")
        except Exception as e:  # noqa: BLE001  (which exception is the record)
            raised.append(type(e).__name__)
    store["wrapper_raises"] = np.array(raised)

    a, b, m = T.psnr_inputs()
    store["psnr"] = npy(metric.PSNRMetric()(a, b, m))
    for i, arr in enumerate(T.transpose_inputs()):
        store[f"chw_to_hwc_{i}"] = npy(transpose.swapimdims_3HW_HW3(arr))
        hwc = np.ascontiguousarray(npy(T.O.chw_to_hwc(arr)))
        store[f"hwc_to_chw_{i}"] = npy(transpose.swapimdims_HW3_3HW(hwc))

    for name in TH.COLOUR_MODULES:
        sd = getattr(colors, name)().state_dict()
        store[f"colour_{name}_keys"] = np.array(list(sd))
        for k, v in sd.items():
            store[f"colour_{name}_{k}"] = npy(v)

    sd = convert_state.convert_state_dict(TH.convert_state_input())
    store["convert_state_keys"] = np.array(list(sd))
    for i, v in enumerate(sd.values()):
        store[f"convert_state_{i}"] = npy(v)

    src = open(os.path.join(REF, "model.py")).read()
    body = src[src.index("class TriSpaceRegNet"):]
    body = body[:body.index("def cat_coords")]
    attrs = set(re.findall(r"self\.(\w+)\s*=\s*(?:torch\.nn\.Parameter|nn\.Parameter|colors\.\w+\(|polylayer|timm\.)", body))
    store["trispace_attrs"] = np.array(sorted(attrs))

    np.savez_compressed(os.path.join(HERE, "vs_reference.npz"), **store)
    print("vs_reference ok", len(store), "arrays")


if __name__ == "__main__":
    main()
