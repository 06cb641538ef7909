"""The host side of the C ABI, pinned on a CPU: tests/twin/launch_plan_twin.cpp compiles curl_kernels.hip for the host only,
links no HIP runtime, and records every launch the entry points would make -- kernel instantiation, grid, block, dynamic LDS
and a digest of every kernel argument (`launch_plan_twin -v` prints them in full) -- for a table of calls that takes each side
of every launch rule and every single-fault error.

tests/data/launch_plan.txt is that record (launch decisions, return codes, error texts).  A wrong unroll, LDS reservation,
tile mapping or self-prep choice gives the same bits at another speed: nothing but this comparison and bench.py would notice.
The record is regenerated only for a deliberate tuning change (tools/README.md).  The source line of each launch is left out
of the comparison; the program itself checks that the lines it recorded are exactly host_api.inc's launch sites and that it
called exactly the entry points include/curl_hip.h declares."""
import difflib
import os
import re
import subprocess

import pytest

from conftest import HIP_CLANG, ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "curl_amd", "csrc")
HOST_API = os.path.join(CSRC, "kernels", "host_api.inc")
HEADER = os.path.join(ROOT, "include", "curl_hip.h")
EXPECTED = os.path.join(ROOT, "tests", "data", "launch_plan.txt")


@pytest.fixture(scope="module")
def plan_twin():
    if not (os.path.exists(HIP_CLANG) and os.path.exists(HIPCC)):
        pytest.skip("hipcc's clang is not installed here")
    src = os.path.join(ROOT, "tests", "twin", "launch_plan_twin.cpp")
    deps = [src, HEADER] + [os.path.join(d, f) for d, _, fs in os.walk(CSRC) for f in fs if f.endswith((".h", ".inc", ".hip"))]
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe, obj = os.path.join(out_dir, "launch_plan_twin"), os.path.join(out_dir, "launch_plan_twin.o")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-Wno-unused-value", "-I", CSRC,
                               "-c", src, "-o", obj])
        subprocess.check_call([HIP_CLANG, "-rdynamic", obj, "-o", exe, "-ldl"])
    return exe


def test_links_no_hip_runtime(plan_twin):
    assert "libamdhip64" not in subprocess.run(["ldd", plan_twin], capture_output=True, text=True, check=True).stdout


def test_launch_plan_is_the_recorded_one(plan_twin):
    run = subprocess.run([plan_twin, HOST_API, HEADER], capture_output=True, text=True)
    print(run.stderr)
    assert run.returncode == 0, run.stderr                       # the program's own two coverage conditions
    got = [re.sub(r"@\d+ ", "", line) for line in run.stdout.splitlines()]
    with open(EXPECTED) as f:
        want = f.read().splitlines()
    if got != want:
        diff = list(difflib.unified_diff(want, got, "tests/data/launch_plan.txt", "this tree", lineterm="", n=0))
        # the record holds a digest of each launch's arguments: show the changed calls of THIS tree with them in full
        full = subprocess.run([plan_twin, "-v", HOST_API, HEADER], capture_output=True, text=True).stdout.splitlines()
        changed = {line[1:].split(" => ")[0] for line in diff if line.startswith("+") and " => " in line}
        detail = [re.sub(r"@\d+ ", "", line) for line in full if line.split(" => ")[0] in changed]
        pytest.fail("the host side no longer plans its launches as recorded:\n" + "\n".join(line[:400] for line in diff[:60]) +
                    "\nthe changed calls of this tree, kernel arguments in full:\n" + "\n".join(detail[:30]))
