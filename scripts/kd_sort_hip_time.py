"""Time the k-d leaf sort of the pruned search: solver.kd_sort (torch) against ops.kd_sort (houv_kd_sort, one HIP launch) on
256 x 2048-point clouds (leaf 32) and 256 x 4096-point clouds (leaf 64), both rules.  HIP events on the current stream after a
warm-up; the median of the repeats is reported.  Also checks that both return the same bits.

    python scripts/kd_sort_hip_time.py [--reps 20] [--out profiles/r04_kd_sort_hip.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from houv_amd import _lib, ops, solver, synthetic  # noqa: E402


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"houv_kd_sort vs solver.kd_sort (torch), {torch.cuda.get_device_name(dev)}, build {_lib.build_id()}, "
             f"torch {torch.__version__}, median of {args.reps} after warm-up, HIP events"]
    for N, leaf in ((2048, 32), (4096, 64)):
        src, tgt, _ = synthetic.make_pairs(128, N, seed=1)
        x = torch.cat([src, tgt]).to(dev)                  # 256 clouds
        for rule in ("area", "extent"):
            same = torch.equal(ops.kd_sort(x, leaf, rule).view(torch.int32), solver.kd_sort(x.clone(), leaf, rule).view(torch.int32))
            t_torch = _time(lambda: solver.kd_sort(x, leaf, rule), args.reps)
            t_hip = _time(lambda: ops.kd_sort(x, leaf, rule), args.reps)
            lines.append(f"256 x {N} pts, leaf {leaf}, rule {rule:6s}: torch {t_torch:8.3f} ms   hip {t_hip:7.3f} ms   "
                         f"x{t_torch / t_hip:6.1f}   same bits: {same}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
