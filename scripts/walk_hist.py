"""Histogram of the term masks (`need`, four bits per direction) the pruned walks see at bench.py's launch shape -- P pairs x 64
hypotheses, LAUNCHES launches of 50 iterations of one base stage -- per launch and over the stage, with the table of compiled
walk variants (houv_solve_walk_variant) of the loaded library: houv_debug_set("solve_walk_hist"), +1 in slot `need` per walking
wave and sweep, the unit of solve_stats[2].  What profiles/r12_walk_variants.txt chose the variants from.  Environment: P, N, LAUNCHES."""
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
print("build", _lib.build_id(), "table", [_lib.solve_walk_variant(i) for i in range(16)], flush=True)
total = [0] * 16
done = 0
for l in range(launches):
    hist = torch.zeros(16, dtype=torch.int64, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    _lib.debug_set("solve_walk_hist", hist.data_ptr()); _lib.debug_set("solve_stats", stats.data_ptr())
    ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=iters, angle_base=0, trans_mode=0, use_views=True, f64_params=False,
                      k_full=N // 2, k_view=N, lr=0.01, loss_scale=1.0 / n, want_grad=False, want_cd=False, nn_ws=nn_ws, ws_valid=done > 0)
    torch.cuda.synchronize()
    _lib.debug_set("solve_walk_hist", 0); _lib.debug_set("solve_stats", 0)
    h, s = [int(x) for x in hist.cpu()], [int(x) for x in stats.cpu()]
    done += iters
    tot = sum(h)
    print(f"launch {l}: wave-sweeps walked {tot} (stats[2] {s[2]}), brute {s[3]}, terms {s[6]}/{s[7]}", flush=True)
    print("  " + " ".join(f"{m}:{100.0 * c / tot:.2f}%" for m, c in enumerate(h)), flush=True)
    print("  raw", h, flush=True)
    total = [a + b for a, b in zip(total, h)]
tot = sum(total)
print("all launches: " + " ".join(f"{m}:{100.0 * c / tot:.2f}%" for m, c in enumerate(total)))
print("raw", total)
