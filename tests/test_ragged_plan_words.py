"""Every word the five ragged plan builders write, against fixtures recorded before the builders were folded together
(tests/golden/ragged_plan_*.npy, int32, row 0 without masks and row 1 with; tests/golden/make_golden_ragged_plans.py):
curl_ragged_plan for operators 0, 35 and 126, curl_msssim_ragged_plan and curl_loss_ragged_plan on one three-image shape list.
The ABI tests beside this one read the words they name by hand; this one holds the layout, the stamps and the hashes whole."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

SHAPES = [(32, 32), (33, 47), (97, 129)]   # a one-tile image, odd sides (padding between the arenas' images), several tiles
CHANNELS = [3, 4, 3]                       # curl_ragged_plan's only: an RGBA image among RGB ones
BUILDERS = ["op0", "op35", "op126", "msssim", "loss"]


def plan_words(lib, builder, has_mask):
    """The plan of SHAPES that one builder writes: exactly *_plan_bytes / 4 int32 words."""
    B = len(SHAPES)
    hs, ws = (np.ascontiguousarray([s[k] for s in SHAPES], dtype=np.int32) for k in range(2))
    cs = np.ascontiguousarray(CHANNELS, dtype=np.int32)
    if builder.startswith("op"):
        op = int(builder[2:])
        nbytes = lib.curl_ragged_plan_bytes(B, op)
    else:
        nbytes = getattr(lib, f"curl_{builder}_ragged_plan_bytes")(B)
    assert nbytes > 0 and nbytes % 4 == 0
    buf = np.full(nbytes // 4 + 2, -1, dtype=np.int32)  # not zeros: a word the builder leaves alone would show
    assert buf.ctypes.data % 8 == 0
    if builder.startswith("op"):
        rc = lib.curl_ragged_plan(B, hs.ctypes.data, ws.ctypes.data, cs.ctypes.data, has_mask, op, buf.ctypes.data, nbytes)
    else:
        rc = getattr(lib, f"curl_{builder}_ragged_plan")(B, hs.ctypes.data, ws.ctypes.data, has_mask, buf.ctypes.data, nbytes)
    assert rc == 0, (builder, rc, lib.curl_last_error())
    assert (buf[nbytes // 4:] == -1).all()  # nothing past the size the query gives
    return buf[:nbytes // 4].copy()


@pytest.fixture(scope="module")
def lib():
    from curl_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("builder", BUILDERS)
def test_plan_words_are_the_recorded_ones(lib, builder):
    want = np.load(os.path.join(GOLDEN, f"ragged_plan_{builder}.npy"))
    assert want.dtype == np.int32 and want.shape[0] == 2
    for has_mask in (0, 1):
        got = plan_words(lib, builder, has_mask)
        assert got.shape == want[has_mask].shape, (builder, has_mask)
        differ = np.flatnonzero(got != want[has_mask])
        assert differ.size == 0, (builder, has_mask, differ[:8], got[differ[:8]], want[has_mask][differ[:8]])
    assert (want[0] != want[1]).any()  # the two rows are two plans: the mask flag and the hash at the least
