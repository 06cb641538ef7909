"""Record tests/golden/ragged_plan_*.npy: the int32 words the ragged plan builders of the built library write for
tests/test_ragged_plan_words.py's shape list, row 0 without masks and row 1 with.  The committed files were recorded from the
build before the builders were folded together; run this again only when a plan's layout changes on purpose.

    python tests/golden/make_golden_ragged_plans.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from conftest import GOLDEN  # noqa: E402  (puts the repository root on the path too)
from test_ragged_plan_words import BUILDERS, plan_words  # noqa: E402

if __name__ == "__main__":
    from curl_amd import _lib
    lib = _lib.load()
    for builder in BUILDERS:
        words = np.stack([plan_words(lib, builder, has_mask) for has_mask in (0, 1)])
        np.save(os.path.join(GOLDEN, f"ragged_plan_{builder}.npy"), words)
        print(builder, words.shape, words.dtype)
