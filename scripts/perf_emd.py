"""Time per call of the auction EMD (houv_emd_forward, one launch per call) at the reference's settings: training (50
iterations), completion-net evaluation (3000), the reference's own test_emd size (20 x 8192, eps 0.05, 3000) and a large batch.
HIP events after a warm-up call; the median of the repeats.  Also reports the iterations each cloud actually ran (the auction
stops early once every point is assigned) and the mean EMD.

    python scripts/perf_emd.py [--reps 3] [--out profiles/r05_perf_emd.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from houv_amd import _lib, ops  # noqa: E402

CONFIGS = [  # (label, B, N, eps, iters)
    ("training", 32, 2048, 0.005, 50),
    ("evaluation (pcn.py / vrcnet.py)", 32, 2048, 0.004, 3000),
    ("reference test_emd", 20, 8192, 0.05, 3000),
    ("large batch", 256, 2048, 0.005, 50),
]


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_emd.py needs an MI355X")
    dev = torch.device("cuda:0")
    lines = [f"# scripts/perf_emd.py  library build {_lib.build_id()}  {torch.cuda.get_device_name(0)}  reps={args.reps}",
             "# config | B x N | eps | iters | ms per call (median [min, max]) | ms per cloud-call | iterations run (min / median / max) | mean EMD"]
    for label, B, N, eps, iters in CONFIGS:
        g = torch.Generator().manual_seed(B * N + iters)
        x1 = torch.rand((B, N, 3), generator=g).to(dev)
        x2 = torch.rand((B, N, 3), generator=g).to(dev)
        ws = ops.emd_workspace(B, N, dev)
        out = {}

        def call():
            out["r"] = ops.emd_forward(x1, x2, eps, iters, workspace=ws)
        med, lo, hi = _time(call, args.reps)
        dist, _, run = out["r"]
        run = run.cpu().sort().values
        emd_mean = torch.sqrt(dist).mean().item()
        lines.append(f"{label} | {B} x {N} | {eps} | {iters} | {med:.3f} [{lo:.3f}, {hi:.3f}] | {med / B:.4f} | "
                     f"{run[0].item()} / {run[len(run) // 2].item()} / {run[-1].item()} | {emd_mean:.6f}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
