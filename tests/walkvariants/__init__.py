"""Builds tests/walkvariants/walk_variants_main.cpp (a host compile of houv_amd/csrc/houv_math.h's walk_variant) with g++ and
runs it as a child process.  Test infrastructure only."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def build():
    out = os.path.join(_HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "walk_variants_main")
    src = os.path.join(_HERE, "walk_variants_main.cpp")
    hdr = os.path.join(_HERE, "..", "..", "houv_amd", "csrc", "houv_math.h")
    if (not os.path.exists(exe)) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    return exe


def table():
    """-> (variant[16], instantiated[16] of bool, cost[16], packed table) as the header computes them."""
    out = subprocess.run([build()], stdout=subprocess.PIPE, check=True, timeout=120, text=True).stdout.split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out[:16]]
    assert [r[0] for r in rows] == list(range(16)), out
    packed = int(out[16].split()[1], 16)
    return [r[1] for r in rows], [bool(r[2]) for r in rows], [r[3] for r in rows], packed
