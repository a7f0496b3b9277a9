"""Builds tests/boxcull/box_cull_main.cpp (a host compile of houv_amd/csrc/houv_math.h's box_test_group and box_test_query)
with g++ and runs it as a child process.  Test infrastructure only."""
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

CASE = np.dtype([("nmet", "<i4"), ("mset", "<i4"), ("count", "<i4"), ("q", "<f4", (64, 3)), ("ub", "<f4", (64, 4)),
                 ("lo", "<f4", (3,)), ("hi", "<f4", (3,))])
VERDICT = np.dtype([("lanes", "<u8"), ("group", "<i4"), ("glo", "<f4", (3,)), ("ghi", "<f4", (3,)), ("gub", "<f4", (4,)), ("pad", "<i4")])


def build():
    out = os.path.join(_HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "box_cull_main")
    src = os.path.join(_HERE, "box_cull_main.cpp")
    hdr = os.path.join(_HERE, "..", "..", "houv_amd", "csrc", "houv_math.h")
    if (not os.path.exists(exe)) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    return exe


def cases(n, nmet=4, mset=15, count=64):
    """n cases, zero-filled but for the header fields."""
    c = np.zeros(n, dtype=CASE)
    c["nmet"], c["mset"], c["count"] = nmet, mset, count
    return c


def verdicts(c):
    """-> structured array (group, lanes, glo, ghi, gub), one entry per case, as the header computes them."""
    assert c.dtype == CASE and CASE.itemsize == 12 + 64 * 7 * 4 + 24 and VERDICT.itemsize == 56
    blob = np.int32(len(c)).tobytes() + c.tobytes()
    out = subprocess.run([build()], input=blob, stdout=subprocess.PIPE, check=True, timeout=300).stdout
    assert len(out) == len(c) * VERDICT.itemsize, (len(out), len(c))
    return np.frombuffer(out, dtype=VERDICT)
