"""Builds tests/schedmath/sched_main.cpp (a host compile of houv_amd/csrc/houv_math.h's stage-scheduling arithmetic) with g++ and
runs it as a child process.  Test infrastructure only."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def build():
    out = os.path.join(_HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sched_main")
    src = os.path.join(_HERE, "sched_main.cpp")
    hdr = os.path.join(_HERE, "..", "..", "houv_amd", "csrc", "houv_math.h")
    if (not os.path.exists(exe)) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    return exe


def items(shapes):
    """shapes: [(ninst, n_iters, chunk_iters)] -> per shape (items, items64, chunks, [(ticket, chunk, hypothesis, steps, iters)])."""
    text = "".join(f"{a} {b} {c}\n" for a, b, c in shapes)
    out = subprocess.run([build()], input=text, stdout=subprocess.PIPE, check=True, timeout=120, text=True).stdout.split("\n")
    res, i = [], 0
    for _ in shapes:
        head = out[i].split()
        n = int(head[1])
        rows = [tuple(int(x) for x in line.split()) for line in out[i + 1:i + 1 + n]]
        res.append((n, int(head[2]), int(head[4]), rows))
        i += 1 + n
    return res
