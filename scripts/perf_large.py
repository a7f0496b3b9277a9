"""Time per hypothesis-iteration of the fused loop for large clouds (houv_solve_iterate_large) against the un-fused path it
replaces (solver._run_stage_unfused: Chamfer op + torch.topk + autograd + torch.optim.Adam) and, at 4096 points, against the
in-LDS brute-force kernel (solve_kernel<1024, 4, 4, 0>), at 4096 / 6144 / 8192 / 16384 points with the view terms on.
HIP events after a warm-up; the median of the repeats.  Also derives the per-CU point-pair rate solver.LARGE_PAIRS_PER_S_PER_CU
is set from, and (--bound) runs run_stage on 256 pairs x K = 64 x 16384 points with LAUNCH_LOG on, reporting the longest launch.

    python scripts/perf_large.py [--reps 3] [--bound] [--out profiles/r04_perf_large.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from houv_amd import _lib, ops, solver, synthetic  # noqa: E402


def _time(fn, reps, warmup=1):
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


def _clouds(P, N, dev):
    src, tgt, _ = synthetic.make_pairs(min(P, 4), N, seed=31)
    reps = -(-P // src.shape[0])
    return src.repeat(reps, 1, 1)[:P].contiguous().to(dev), tgt.repeat(reps, 1, 1)[:P].contiguous().to(dev)


def _kernel(src, tgt, K, iters, large):
    P, N, _ = src.shape
    n = P * K
    state = torch.zeros((n, 24), dtype=torch.float64, device=src.device)
    state[:, :8] = torch.as_tensor(solver.houv_init_params(n)).to(src.device)

    def run():
        ops.solve_iterate(src, tgt, state, K, steps_done=0, n_iters=iters, angle_base=0, trans_mode=0, use_views=True,
                          f64_params=False, k_full=N // 2, k_view=N, lr=0.01, loss_scale=1.0 / n, large=large)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bound", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    lines = [f"houv_solve_iterate_large, {torch.cuda.get_device_name(dev)} ({n_cu} CUs), build {_lib.build_id()}, "
             f"torch {torch.__version__}, view terms on, median of {args.reps} after a warm-up, HIP events"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("points   path                         hypotheses x iterations   ms        us / hypothesis-iteration   pairs/s per CU")
    K = 64
    for N in (4096, 6144, 8192, 16384):
        P = 8 if N <= 8192 else 4                 # 512 / 256 workgroups: whole rounds of one workgroup per CU
        iters = 4 if N <= 8192 else 1
        src, tgt = _clouds(P, N, dev)
        n = P * K
        rows = [("large (fused, streamed)", True)] + ([("in-LDS brute <1024,4,4,0,1>", False)] if N <= 4096 else [])
        for name, large in rows:
            ms = _time(_kernel(src, tgt, K, iters, large), args.reps)
            us = ms * 1e3 / (n * iters)
            rate = 2.0 * N * N * n * iters / (ms * 1e-3) / n_cu
            emit(f"{N:6d}   {name:28s} {n:6d} x {iters:2d}               {ms:9.2f}   {us:10.2f}                  {rate / 1e9:6.1f} G")
        # the un-fused path, fewer hypotheses (it replicates both clouds K-fold and keeps autograd intermediates)
        Pu, itu = (2, 2) if N <= 8192 else (1, 2)
        su, tu = src[:Pu].contiguous(), tgt[:Pu].contiguous()
        p0 = solver.houv_init_params(Pu * K)

        def unf():
            solver._run_stage_unfused(su, tu, torch.as_tensor(p0), K, itu, angle_base=0, trans_mode=0, use_views=True,
                                      f64_params=False, lr=0.01, want_grad=False, want_cd=False, alpha=0.5)
        ms = _time(unf, max(1, args.reps - 1))
        emit(f"{N:6d}   {'un-fused (Chamfer op + torch)':28s} {Pu * K:6d} x {itu:2d}               {ms:9.2f}   "
             f"{ms * 1e3 / (Pu * K * itu):10.2f}")
        del src, tgt, su, tu
        torch.cuda.empty_cache()
    if args.bound:
        P, N = 256, 16384
        src, tgt = _clouds(P, N, dev)
        pairs, iters = solver.large_launch_plan(P, K, N, N, n_cu)
        solver.LAUNCH_LOG = []
        torch.cuda.synchronize()
        solver.run_stage(src, tgt, solver.houv_init_params(P * K), K, 2, angle_base=0, trans_mode=0, use_views=True,
                         f64_params=False, lr=0.01)
        torch.cuda.synchronize()
        log, solver.LAUNCH_LOG = solver.LAUNCH_LOG, None
        ms = [a.elapsed_time(b) for a, b, *_ in log]
        emit(f"run_stage 256 pairs x K=64 x 16384 points x 2 iterations: plan {pairs} pairs x {iters} iterations per launch, "
             f"{len(log)} launches, longest {max(ms):.1f} ms, median {statistics.median(ms):.1f} ms "
             f"(bound solver.LARGE_LAUNCH_BUDGET_S = {solver.LARGE_LAUNCH_BUDGET_S * 1e3:.0f} ms, "
             f"rate constant {solver.LARGE_PAIRS_PER_S_PER_CU / 1e9:.0f} G pairs/s per CU)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
