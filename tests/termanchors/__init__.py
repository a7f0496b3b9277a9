"""Builds tests/termanchors/term_anchors_main.cpp (a host compile of houv_amd/csrc/houv_math.h's term_anchor_masks and
term_masks) with g++ and runs it as a child process.  Test infrastructure only."""
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
RECORD_FLOATS = 82      # cd 8 | fresh pose 12 | stale poses 4 x 12 | stale bits | R 9 | T 3 | radius


def build():
    out = os.path.join(_HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "term_anchors_main")
    src = os.path.join(_HERE, "term_anchors_main.cpp")
    hdr = os.path.join(_HERE, "..", "..", "houv_amd", "csrc", "houv_math.h")
    if (not os.path.exists(exe)) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    return exe


def records(cd, fresh_R, fresh_T, stale_R, stale_T, stale_bits, R, T, radius):
    """cd [n,4,2], fresh_R [n,3,3], fresh_T [n,3], stale_R [n,4,3,3], stale_T [n,4,3], stale_bits [n] (bit m / 4 + m: the term
    (metric m, dir 0 / 1) has the stale record pose of its metric), R [n,3,3], T [n,3], radius [n] -> float32 [n, 82]."""
    n = cd.shape[0]
    stale = np.concatenate([np.asarray(stale_R).reshape(n, 4, 9), np.asarray(stale_T).reshape(n, 4, 3)], axis=2).reshape(n, 48)
    return np.concatenate([np.asarray(cd).reshape(n, 8), np.asarray(fresh_R).reshape(n, 9), np.asarray(fresh_T).reshape(n, 3),
                           stale, np.asarray(stale_bits, dtype=np.float64).reshape(n, 1), np.asarray(R).reshape(n, 9),
                           np.asarray(T).reshape(n, 3), np.asarray(radius).reshape(n, 1)], axis=1).astype(np.float32)


def run(rec, nmet=4):
    """records float32 [n, 82] -> (new, old) uint8 [n] each: term_anchor_masks' and term_masks' result (the latter with cd and
    the fresh pose as its anchor); bit m = term (metric m, dir 0) needed, bit 4 + m = (metric m, dir 1)."""
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    assert rec.ndim == 2 and rec.shape[1] == RECORD_FLOATS
    out = subprocess.run([build(), str(nmet)], input=rec.tobytes(), stdout=subprocess.PIPE, check=True, timeout=120).stdout
    assert len(out) == 2 * rec.shape[0]
    both = np.frombuffer(out, dtype=np.uint8).reshape(-1, 2)
    return both[:, 0], both[:, 1]
