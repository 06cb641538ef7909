"""One builder for the host twins that have a source file of their own under tests/twin/: the two flavours of conftest's `twin`
fixture (rounding: g++ without contraction; contracting: hipcc's clang contracting as the kernels' compiler does)."""
import ctypes
import os
import subprocess

import pytest

from conftest import HIP_CLANG, ROOT

FLAVOURS = ["rounding", "contracting"]
CSRC = os.path.join(ROOT, "curl_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
COMMON = ["-std=c++17", "-DCURL_HOST_TWIN", "-Wno-unknown-pragmas"]


def stale(out, src):
    """`out` is missing or older than `src` or any header of curl_amd/csrc."""
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps)


def twin_library(source, flavour):
    """tests/twin/<source> -> tests/_build/lib<stem>[_contracting].so, rebuilt when stale, loaded with ctypes."""
    src = os.path.join(ROOT, "tests", "twin", source)
    stem = os.path.splitext(source)[0]
    if flavour == "rounding":
        name, cmd = f"lib{stem}.so", ["g++", "-O2", "-mfma", "-ffp-contract=off"]
    else:
        if not os.path.exists(HIP_CLANG):
            pytest.skip("hipcc's clang is not installed here")
        name, cmd = f"lib{stem}_contracting.so", [HIP_CLANG, "-O2", "-mfma", "-ffp-contract=fast-honor-pragmas"]
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, name)
    if stale(so, src):
        subprocess.check_call(cmd + ["-fPIC", "-shared"] + COMMON + ["-o", so, src])
    return ctypes.CDLL(so)
