"""Builds tests/termmasks/term_masks_main.cpp (a host compile of houv_amd/csrc/houv_math.h's term_masks) with g++ and runs it
as a child process.  Test infrastructure only."""
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
RECORD_FLOATS = 33      # anchor (8 cd | R 9 | T 3) | R 9 | T 3 | radius


def build():
    out = os.path.join(_HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "term_masks_main")
    src = os.path.join(_HERE, "term_masks_main.cpp")
    hdr = os.path.join(_HERE, "..", "..", "houv_amd", "csrc", "houv_math.h")
    if (not os.path.exists(exe)) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    return exe


def run(records, nmet=4):
    """records float32 [n, 33] -> uint8 [n]: bit m = term (metric m, dir 0) needed, bit 4 + m = (metric m, dir 1)."""
    rec = np.ascontiguousarray(records, dtype=np.float32)
    assert rec.ndim == 2 and rec.shape[1] == RECORD_FLOATS
    out = subprocess.run([build(), str(nmet)], input=rec.tobytes(), stdout=subprocess.PIPE, check=True, timeout=120).stdout
    assert len(out) == rec.shape[0]
    return np.frombuffer(out, dtype=np.uint8)
