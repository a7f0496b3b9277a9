"""What seeding a stage's first iteration (houv_solve_seed; solver.SEED_FIRST) does to a base stage at bench.py's launch shape
(P pairs x 64 hypotheses x 2048 points x 200 iterations), unseeded and seeded alternated on one device:

  1. the stage launched chunk by chunk (ITERS per launch): HIP-event time of every launch -- the first one carries the first
     iteration (unseeded: the brute-force sweep over every sub-tile; seeded: houv_solve_seed + a pruned iteration);
  2. houv_solve_seed alone;
  3. the stage as solver.run_stage runs it by default (one houv_solve_stage_pruned launch), by its LAUNCH_LOG events;
  4. houv_debug_set("solve_stats") of a seeded stage and of its first iteration alone.

The score sums of all runs must be equal to the digit.  -> profiles/r15_remnants.txt"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from houv_amd import _lib, ops, solver, synthetic

dev = torch.device("cuda:0")
P, K, N = int(os.environ.get("P", 256)), 64, int(os.environ.get("N", 2048))
total, iters, reps = int(os.environ.get("TOTAL", 200)), int(os.environ.get("ITERS", 50)), int(os.environ.get("REPS", 3))
n = P * K
src, tgt, _ = synthetic.make_pairs(P, N, seed=2021)
src, tgt = solver.spatial_sort(src.to(dev)), solver.spatial_sort(tgt.to(dev))
p0 = solver.houv_init_params(n)
kw = dict(angle_base=0, trans_mode=0, use_views=True, f64_params=False, lr=0.01)
print(f"{P} pairs x {K} x {N} points x {total} iterations; build {_lib.build_id()}", flush=True)


def stage(seeded, n_iters=total, **extra):
    solver.SEED_FIRST = seeded
    solver.LAUNCH_LOG = []
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    out, _ = solver.run_stage(src, tgt, p0, K, n_iters, **kw, **extra)
    e1.record(); torch.cuda.synchronize()
    solver.check_stage_status(wait=True)
    log, solver.LAUNCH_LOG = solver.LAUNCH_LOG, None
    return e0.elapsed_time(e1), [a.elapsed_time(b) for a, b, *_ in log], float(out["score"].double().sum())


stage(True, n_iters=2); stage(False, n_iters=2)                       # first-use set-up of both kernels
print(f"## 1. launches of {iters} iterations", flush=True)
for rep in range(2):
    for seeded in (False, True):
        ms, per, score = stage(seeded, iters_per_launch=iters)
        print(f"{'seeded  ' if seeded else 'unseeded'}: " + " / ".join(f"{x:.1f}" for x in per) + f" ms, sum {sum(per):.1f} ms; score sum {score:.9f}",
              flush=True)
print("## 2. houv_solve_seed alone", flush=True)
state = torch.zeros((n, 24), dtype=torch.float64, device=dev)
state[:, :8] = torch.as_tensor(p0).to(dev)
ws = ops.solve_workspace(n, N, N, dev)
for rep in range(reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    ops.solve_seed(src, tgt, state, K, 0, 0, True, ws)
    e1.record(); torch.cuda.synchronize()
    print(f"seed kernel: {e0.elapsed_time(e1):.3f} ms = {e0.elapsed_time(e1) * 1e3 / n:.4f} us per hypothesis", flush=True)
print("## 3. one launch per stage (LAUNCH_LOG events; the seeded stage's span its seed launch)", flush=True)
for rep in range(reps):
    for seeded in (False, True):
        ms, per, score = stage(seeded)
        print(f"{'seeded  ' if seeded else 'unseeded'}: stage {ms:.1f} ms, kernels {sum(per):.1f} ms in {len(per)} launch; "
              f"{sum(per) * 1e3 / (n * total):.4f} us per hypothesis-iteration; score sum {score:.9f}", flush=True)
print("## 4. solve_stats of a seeded stage", flush=True)
buf = torch.zeros(8, dtype=torch.int64, device=dev)
for seeded, n_iters in ((False, total), (True, total), (True, 1)):
    buf.zero_()
    _lib.debug_set("solve_stats", buf.data_ptr())
    try:
        stage(seeded, n_iters=n_iters)
    finally:
        _lib.debug_set("solve_stats", 0)
    v = [int(x) for x in buf.cpu()]
    print(f"{'seeded  ' if seeded else 'unseeded'}, {n_iters} iterations: asked {v[0]}, steps {v[1]}, pruned wave-sweeps {v[2]}, brute wave-sweeps "
          f"{v[3]}; sub-tiles asked per query and sweep {v[0] / max(v[2], 1) / 256.0:.2f}; terms {v[6]} of {v[7]}", flush=True)
