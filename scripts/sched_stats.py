"""Where the chip stands idle while the fused loop runs: houv_debug_set("solve_sched") at scripts/pmc_probe.py's launch shape
(P pairs x 64 hypotheses x ITERS iterations per launch, LAUNCHES of them = one stage).

MODE=launches  separate houv_solve_iterate[_pruned] launches, one workgroup per hypothesis (the counters are read per launch)
MODE=stage     one houv_solve_stage[_pruned] launch of LAUNCHES x ITERS iterations in items of ITERS (persistent grid, tickets)
SOLVER=pruned|brute|both.  Per launch it prints each XCD's items, busy span and mean workgroup time, the spread of the XCDs' end
stamps over the launch span, the launch span from the stamps beside the HIP-event time of the same launch (the 100-MHz counter
agrees across XCDs when the two match), and the idle slot-time 1 - sum of durations / (resident workgroups x launch span)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from houv_amd import _lib, ops, solver, synthetic

dev = torch.device("cuda:0")
P, K, N, iters = int(os.environ.get("P", 256)), 64, int(os.environ.get("N", 2048)), int(os.environ.get("ITERS", 50))
launches = int(os.environ.get("LAUNCHES", 3))
mode = os.environ.get("MODE", "launches")
which = os.environ.get("SOLVER", "both")
TICK_US = 0.01                                                       # s_memrealtime: 100 MHz

src, tgt, _ = synthetic.make_pairs(P, N, seed=2021)
src, tgt = solver.spatial_sort(src.to(dev)), solver.spatial_sort(tgt.to(dev))
n = P * K
cus = torch.cuda.get_device_properties(dev).multi_processor_count
ONES = (1 << 64) - 1


def fresh_counters():
    c = torch.zeros((8, 4), dtype=torch.int64, device=dev)
    c[:, 2] = -1                                                     # all ones: the minima start there
    return c


def report(tag, c, ms, resident):
    c = c.cpu().numpy().astype("uint64")
    live = [x for x in range(8) if c[x, 0] > 0]
    t0, t1 = min(int(c[x, 2]) for x in live), max(int(c[x, 3]) for x in live)
    span = (t1 - t0) * TICK_US
    busy = sum(int(c[x, 1]) for x in live) * TICK_US
    ends = [int(c[x, 3]) for x in live]
    print(f"{tag}: HIP events {ms * 1e3:.0f} us, stamps {span:.0f} us (ratio {span / (ms * 1e3):.4f}); items {int(c[:, 0].sum())}; "
          f"XCD end-stamp spread {(max(ends) - min(ends)) * TICK_US:.0f} us = {(max(ends) - min(ends)) / (t1 - t0) * 100:.2f} % of the span; "
          f"idle slot-time {(1 - busy / (resident * span)) * 100:.2f} % of {resident} slots", flush=True)
    for x in live:
        print(f"    XCD {x}: {int(c[x, 0]):6d} items, busy span {(int(c[x, 3]) - int(c[x, 2])) * TICK_US:9.0f} us, "
              f"starts +{(int(c[x, 2]) - t0) * TICK_US:7.1f} us, ends -{(t1 - int(c[x, 3])) * TICK_US:7.1f} us, "
              f"workgroup time summed {int(c[x, 1]) * TICK_US / 1e3:10.1f} ms", flush=True)


for name in (("pruned", "brute") if which == "both" else (which,)):
    pruned = name == "pruned"
    state = torch.zeros((n, 24), dtype=torch.float64, device=dev)
    state[:, :8] = torch.as_tensor(solver.houv_init_params(n)).to(dev)
    nn_ws = ops.solve_workspace(n, N, N, dev) if pruned else None
    lds = _lib.load().houv_solve_lds_bytes(N, N, int(pruned))
    # what a CU holds of the 128-VGPR kernels (two points per lane or more): 160 KiB of LDS, 16 waves
    resident = min(n, cus * max(1, min(163840 // lds, 1024 // _lib.solve_variant(N, N, pruned)[0])))
    kw = dict(angle_base=0, trans_mode=0, use_views=True, f64_params=False, k_full=N // 2, k_view=N, lr=0.01, loss_scale=1.0 / n,
              nn_ws=nn_ws)
    print(f"{name}, MODE={mode}: {P} pairs x {K} x {iters} iterations x {launches}; {cus} CUs, LDS {lds} B, {resident} resident "
          f"workgroups; build {_lib.build_id()}", flush=True)
    try:
        if mode == "stage":
            c = fresh_counters()
            sched_ws = ops.solve_sched_workspace(n, dev)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            _lib.debug_set("solve_sched", c.data_ptr())
            torch.cuda.synchronize(); e0.record()
            ops.solve_iterate(src, tgt, state, K, steps_done=0, n_iters=iters * launches, ws_valid=False, chunk_iters=iters,
                              sched_ws=sched_ws, **kw)
            e1.record(); torch.cuda.synchronize()
            report(f"  stage of {launches} x {iters}", c, e0.elapsed_time(e1), resident)
            print(f"    status word {int(sched_ws[1].item())}", flush=True)
        else:
            for l in range(launches):
                c = fresh_counters()
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                _lib.debug_set("solve_sched", c.data_ptr())
                torch.cuda.synchronize(); e0.record()
                ops.solve_iterate(src, tgt, state, K, steps_done=l * iters, n_iters=iters, ws_valid=l > 0, **kw)
                e1.record(); torch.cuda.synchronize()
                report(f"  launch {l}", c, e0.elapsed_time(e1), resident)
    finally:
        _lib.debug_set("solve_sched", 0)
