"""What the group cull of the pruned solve's box tests (prune_masks, houv_amd/csrc/houv_sweep.h) does at bench.py's launch shape --
P pairs x 64 hypotheses, LAUNCHES launches of 50 iterations of one base stage -- per launch and over the stage:
houv_debug_set("solve_cull_stats"), four counters: groups tested (one per k of a walking wave and sweep), reference boxes that
survive the group test, per-query tests executed and per-query tests of a loop over all boxes (both per lane: 64 a box).  Beside
them solve_stats[0] and [1] (sub-tile visits asked, steps walked): the visit masks are the same bits with and without the cull, so
these two are equal to the digit between builds.  What profiles/r13_box_cull.txt quotes.  Environment: P, N, LAUNCHES."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from houv_amd import _lib, ops, solver, synthetic
dev = torch.device("cuda:0")
P, K, N, iters, launches = int(os.environ.get("P", 256)), 64, int(os.environ.get("N", 2048)), 50, int(os.environ.get("LAUNCHES", 4))
src, tgt, _ = synthetic.make_pairs(P, N, seed=2021)
leaf = solver.sort_leaf(N, N)
src, tgt = solver.spatial_sort(src.to(dev), leaf), solver.spatial_sort(tgt.to(dev), leaf)
n = P * K
state = torch.zeros((n, 24), dtype=torch.float64, device=dev)
state[:, :8] = torch.as_tensor(solver.houv_init_params(n), dtype=torch.float64).to(dev)
nn_ws = ops.solve_workspace(n, N, N, dev)
_, q, mode = _lib.solve_variant(N, N, True, with_mode=True)
ntile = (N + (64 if mode == 3 else 32) - 1) // (64 if mode == 3 else 32)
print("build", _lib.build_id(), "points", N, "boxes", ntile, "points per lane", q, flush=True)
try:
    _lib.debug_set("solve_cull_stats", 0)
    have_cull = True
except _lib.HouvHipError:            # a library from before the cull: solve_stats alone
    have_cull = False
total = [0] * 4
done = 0
for l in range(launches):
    cull = torch.zeros(4, dtype=torch.int64, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    _lib.debug_set("solve_stats", stats.data_ptr())
    if have_cull:
        _lib.debug_set("solve_cull_stats", cull.data_ptr())
    ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=iters, angle_base=0, trans_mode=0, use_views=True, f64_params=False,
                      k_full=N // 2, k_view=N, lr=0.01, loss_scale=1.0 / n, want_grad=False, want_cd=False, nn_ws=nn_ws, ws_valid=done > 0)
    torch.cuda.synchronize()
    _lib.debug_set("solve_stats", 0)
    if have_cull:
        _lib.debug_set("solve_cull_stats", 0)
    c, s = [int(x) for x in cull.cpu()], [int(x) for x in stats.cpu()]
    done += iters
    print(f"launch {l}: solve_stats[0] visits asked {s[0]}, [1] steps {s[1]}, [2] wave-sweeps walked {s[2]}, [3] brute {s[3]}; "
          f"visits per query {s[0] / max(s[2] * 64 * q, 1):.3f}", flush=True)
    if have_cull:
        g, sv, ex, full = c
        print(f"  groups {g}, boxes surviving {sv} = {sv / max(g, 1):.2f} of {ntile} per group ({100.0 * sv / max(g * ntile, 1):.1f} %); "
              f"per-query tests executed {ex} of {full} ({100.0 * ex / max(full, 1):.1f} %)", flush=True)
        total = [a + b for a, b in zip(total, c)]
if have_cull:
    g, sv, ex, full = total
    print(f"all launches: groups {g}, boxes surviving {sv / max(g, 1):.2f} of {ntile} per group ({100.0 * sv / max(g * ntile, 1):.1f} %), "
          f"per-query tests executed {100.0 * ex / max(full, 1):.1f} % of a full loop")
    print("raw", total)
