"""GPU: houv_solve_stage[_pruned] -- a whole stage in one launch, a persistent grid drawing (hypothesis, chunk) tickets -- against
the existing entry points run as separate launches of chunk_iters: optimiser state, score, loss, R, T, grad and cd must be equal
bit for bit (torch.equal), the status word must stay 0, and the work counters must agree to the digit.  The grids of 1 to 3
workgroups (houv_debug_set("solve_max_workgroups")) make one workgroup hand a hypothesis to itself, and make a workgroup draw the
next chunk of a hypothesis while another still runs the chunk before it."""
import ctypes

import pytest
import torch

KEYS = ("score", "loss", "R", "T", "grad", "cd")

# name: (pairs, restarts, N, M, views, f64 params, pruned, iterations, chunk_iters, grid cap (0 = the occupancy-sized grid),
#        expected (block, points per lane, prune mode))
CASES = {
    "grid1_64pt_brute": (2, 3, 64, 64, True, False, False, 7, 3, 1, (64, 1, 0)),
    "grid3_320pt_pruned": (1, 2, 320, 320, True, False, True, 7, 3, 3, (256, 2, 2)),
    "grid3_7hyp_257pt_pruned_f64": (7, 1, 257, 257, True, True, True, 5, 2, 3, (256, 2, 2)),
    "uncapped_2048pt_bench_kernel": (2, 4, 2048, 2048, True, False, True, 6, 3, 0, (512, 4, 2)),
    "uncapped_2048pt_one_item_per_hypothesis": (2, 4, 2048, 2048, True, False, True, 6, 8, 0, (512, 4, 2)),
    "uncapped_12288hyp_64pt_brute": (48, 256, 64, 64, True, False, False, 4, 2, 0, (64, 1, 0)),
    "uncapped_600x450_one_metric_pruned": (2, 4, 600, 450, False, False, True, 5, 2, 0, (256, 3, 2)),
}


def _problem(name, dev):
    from houv_amd import solver, synthetic
    P, K, N, M = CASES[name][:4]
    src, tgt, _ = synthetic.make_pairs(P, max(N, M), seed=77)
    src, tgt = src[:, :N].contiguous(), tgt[:, :M].contiguous()
    leaf = solver.sort_leaf(N, M)
    src, tgt = solver.spatial_sort(src.to(dev), leaf), solver.spatial_sort(tgt.to(dev), leaf)
    n = P * K
    p0 = torch.as_tensor(solver.houv_init_params(max(n, 26))[:n], dtype=torch.float64)     # rows 0..25: the lattice axes
    return src, tgt, p0


def _kwargs(name, n):
    _, _, N, M, views, f64, _, _, _, _, _ = CASES[name]
    return dict(angle_base=1, trans_mode=0, use_views=views, f64_params=f64, k_full=int(min(N, M) * 0.5),
                k_view=N if views else 1, lr=0.01, loss_scale=1.0 / n, want_grad=True, want_cd=True)


def _fresh_state(name, p0, src):
    from houv_amd import ops
    P, K, N, M = CASES[name][:4]
    n = P * K
    state = torch.zeros((n, 24), dtype=torch.float64, device=src.device)
    state[:, :8] = p0.to(src.device)
    return state, (ops.solve_workspace(n, N, M, src.device) if CASES[name][6] else None)


def _separate_launches(name, src, tgt, p0):
    """The oracle: houv_solve_iterate[_pruned], one launch per chunk.  -> (last launch's outputs, state)."""
    from houv_amd import ops
    P, K = CASES[name][:2]
    iters, chunk = CASES[name][7:9]
    state, nn_ws = _fresh_state(name, p0, src)
    done, out = 0, None
    while done < iters:
        it = min(chunk, iters - done)
        out = ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=it, nn_ws=nn_ws, ws_valid=done > 0,
                                **_kwargs(name, P * K))
        done += it
    return out, state


def _one_stage(name, src, tgt, p0):
    """houv_solve_stage[_pruned] under the case's grid cap.  -> (outputs, state, sched_ws after the launch)."""
    from houv_amd import _lib, ops
    P, K = CASES[name][:2]
    iters, chunk, cap = CASES[name][7:10]
    state, nn_ws = _fresh_state(name, p0, src)
    sched_ws = ops.solve_sched_workspace(P * K, src.device)
    sched_ws.fill_(-7)                                       # the call itself zeroes it
    try:
        _lib.debug_set("solve_max_workgroups", cap)
        out = ops.solve_iterate(src, tgt, state, K, steps_done=0, n_iters=iters, nn_ws=nn_ws, ws_valid=False, chunk_iters=chunk,
                                sched_ws=sched_ws, **_kwargs(name, P * K))
        torch.cuda.synchronize()
    finally:
        _lib.debug_set("solve_max_workgroups", 0)
    return out, state, sched_ws.cpu()


def _check_sched_ws(name, ws):
    P, K = CASES[name][:2]
    iters, chunk = CASES[name][7:9]
    chunks = -(-iters // chunk)
    assert int(ws[1]) == 0, f"status word {int(ws[1])}: a hand-off ran out of time"
    assert int(ws[0]) >= P * K * chunks                      # every item drawn (plus one ticket per workgroup past the end)
    assert bool((ws[4:4 + P * K] == chunks).all()), "every hypothesis must have published every chunk"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_equals_separate_launches(name):
    from houv_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    P, K, N, M = CASES[name][:4]
    assert _lib.solve_variant(N, M, CASES[name][6], with_mode=True) == CASES[name][10]
    src, tgt, p0 = _problem(name, dev)
    ref, st_ref = _separate_launches(name, src, tgt, p0)
    got, st, ws = _one_stage(name, src, tgt, p0)
    _check_sched_ws(name, ws)
    assert torch.equal(st, st_ref), "state"
    for key in KEYS:
        assert torch.equal(got[key], ref[key]), key
    assert torch.isfinite(ref["loss"]).all()


@pytest.mark.gpu
def test_stage_does_the_same_work_and_the_scheduling_counters_count_items():
    """solve_stats[0..3] (sub-tile visits asked for, sub-tile steps executed, pruned wave-sweeps, brute wave-sweeps) of one stage
    call equal the sums over the separate launches to the digit: the same work, not only the same results -- a hypothesis handed
    to another workgroup finds the NN records its previous chunk left.  solve_sched counts exactly hypotheses x chunks items, with
    sane stamps, and nothing is written to it when it is off."""
    from houv_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    for name in ("grid3_320pt_pruned", "uncapped_2048pt_bench_kernel"):
        P, K = CASES[name][:2]
        iters, chunk = CASES[name][7:9]
        src, tgt, p0 = _problem(name, dev)
        stats = {}
        try:
            for which, run in (("launches", _separate_launches), ("stage", _one_stage)):
                buf = torch.zeros(8, dtype=torch.int64, device=dev)
                sched = torch.zeros((8, 4), dtype=torch.int64, device=dev)
                sched[:, 2] = -1
                _lib.debug_set("solve_stats", buf.data_ptr())
                _lib.debug_set("solve_sched", sched.data_ptr())
                res = run(name, src, tgt, p0)
                torch.cuda.synchronize()
                _lib.debug_set("solve_stats", 0)
                _lib.debug_set("solve_sched", 0)
                if which == "stage":
                    _check_sched_ws(name, res[2])
                stats[which] = [int(x) for x in buf.cpu()]
                s = sched.cpu()
                live = s[:, 0] > 0
                print(name, which, "solve_stats", stats[which], "solve_sched items per XCD", s[:, 0].tolist())
                assert int(s[:, 0].sum()) == P * K * -(-iters // chunk), s
                assert bool((s[live, 2] <= s[live, 3]).all()) and bool((s[live, 1] > 0).all()), s
                assert bool((s[~live, 1:] == torch.tensor([0, -1, 0])).all()), s
            # off: the next runs must leave the buffer alone
            before = sched.clone()
            _one_stage(name, src, tgt, p0)
            _separate_launches(name, src, tgt, p0)
            torch.cuda.synchronize()
            assert torch.equal(sched, before)
        finally:
            _lib.debug_set("solve_stats", 0)
            _lib.debug_set("solve_sched", 0)
        assert stats["stage"][:4] == stats["launches"][:4], stats
        assert stats["stage"][2] > 0                          # the pruned walk did run
        assert stats["stage"][6:8] == stats["launches"][6:8], stats


@pytest.mark.gpu
def test_stage_edge_arguments():
    from houv_amd import _lib, ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    name = "grid1_64pt_brute"
    P, K, N = CASES[name][:3]
    src, tgt, p0 = _problem(name, dev)
    n = P * K
    # P = 0 returns at once: nothing is launched, the scheduling workspace is not touched
    ws = ops.solve_sched_workspace(0, dev).fill_(-7)
    ops.solve_iterate(src[:0], tgt[:0], torch.zeros((0, 24), dtype=torch.float64, device=dev), K, steps_done=0, n_iters=3,
                      chunk_iters=2, sched_ws=ws, **_kwargs(name, 1))
    torch.cuda.synchronize()
    assert bool((ws == -7).all())
    # chunk_iters < 1
    state, _ = _fresh_state(name, p0, src)
    before = state.clone()
    ws = ops.solve_sched_workspace(n, dev).fill_(-7)
    for bad in (0, -3):
        with pytest.raises(_lib.HouvHipError, match="chunk_iters"):
            ops.solve_iterate(src, tgt, state, K, steps_done=0, n_iters=3, chunk_iters=bad, sched_ws=ws, **_kwargs(name, n))
    # sched_ws null or not aligned for int32: refused by the library itself
    lib = _lib.load()
    kw = _kwargs(name, n)
    common = (_lib.ptr(src), _lib.ptr(tgt), P, N, N, K, _lib.ptr(state), 0, 3, kw["angle_base"], kw["trans_mode"], 1, 0,
              kw["k_full"], kw["k_view"], 0.01, 0.9, 0.999, 1e-8, 1.0 / n, None, None, None, None, None, None)
    nn_ws = ops.solve_workspace(n, N, N, dev)
    for sched in (None, ctypes.c_void_p(ws.data_ptr() + 2), ctypes.c_void_p(ws.data_ptr() + 1)):
        assert lib.houv_solve_stage(*common, 2, sched, _lib.stream_of(src)) == 0
        assert "sched_ws" in _lib.last_error()
        assert lib.houv_solve_stage_pruned(*common, _lib.ptr(nn_ws), 0, nn_ws.shape[2], 2, sched, _lib.stream_of(src)) == 0
        assert "sched_ws" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(state, before) and bool((ws == -7).all())


@pytest.mark.gpu
def test_run_stage_makes_one_stage_call_and_keeps_its_results():
    """solver.run_stage without iters_per_launch is one houv_solve_stage call with items of ITERS_PER_LAUNCH iterations (one
    LAUNCH_LOG entry: the stage's iterations, first = True); with iters_per_launch it is the loop of separate launches.  Same bits."""
    from houv_amd import solver
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    name = "grid3_320pt_pruned"
    P, K, N = CASES[name][:3]
    src, tgt, p0 = _problem(name, dev)
    kw = dict(angle_base=0, trans_mode=0, use_views=True, f64_params=False, lr=0.01, want_grad=True, want_cd=True)
    old_iters, old_log = solver.ITERS_PER_LAUNCH, solver.LAUNCH_LOG
    try:
        solver.ITERS_PER_LAUNCH = 3
        solver.LAUNCH_LOG = []
        got, st = solver.run_stage(src, tgt, p0, K, 8, **kw)
        torch.cuda.synchronize()
        log = list(solver.LAUNCH_LOG)
        assert [e[2:] for e in log] == [(P * K, 8, N, N, True, True, True)], log
        solver.check_stage_status(wait=True)
        solver.LAUNCH_LOG = []
        ref, st_ref = solver.run_stage(src, tgt, p0, K, 8, iters_per_launch=3, **kw)
        assert [e[3] for e in solver.LAUNCH_LOG] == [3, 3, 2]
    finally:
        solver.ITERS_PER_LAUNCH, solver.LAUNCH_LOG = old_iters, old_log
    assert torch.equal(st, st_ref)
    for key in KEYS:
        assert torch.equal(got[key], ref[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("P,K,N", [(2, 26, 300), (1, 26, 4097)], ids=["300pt_pruned", "4097pt_large"])
def test_run_stage_cuts_with_last_params(P, K, N):
    """solver.run_stage(n_iters=5, iters_per_launch=2, want_last_params=True) -- launches of 2, 2, then 1 and 1 iterations: the cut
    rule of every form -- returns the outputs and state of the plain 5-iteration stage, and as last_params the parameters a
    4-iteration stage ends on.  Pruned kernel (seeded) and large kernel; every comparison is on bits."""
    from houv_amd import solver, synthetic
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    assert solver.uses_pruned(N, N) == (N == 300) and solver.uses_large(N, N) == (N == 4097)
    src, tgt, _ = synthetic.make_pairs(P, N, seed=77)
    src, tgt = src.to(dev), tgt.to(dev)
    p0 = torch.as_tensor(solver.houv_init_params(P * K), dtype=torch.float64)
    kw = dict(angle_base=0, trans_mode=0, use_views=True, f64_params=False, lr=0.01, want_grad=True, want_cd=True)
    got, st = solver.run_stage(src, tgt, p0, K, 5, iters_per_launch=2, want_last_params=True, **kw)
    ref, st_ref = solver.run_stage(src, tgt, p0, K, 5, **kw)
    _, st_4 = solver.run_stage(src, tgt, p0, K, 4, **kw)
    solver.check_stage_status(wait=True)
    assert set(got) == set(KEYS) | {"last_params"} and set(ref) == set(KEYS)
    assert got["last_params"].dtype == torch.float64 and torch.equal(got["last_params"], st_4[:, :8])
    assert not torch.equal(got["last_params"], st[:, :8])        # the last Adam step did move the parameters
    assert torch.equal(st, st_ref), "state"
    for key in KEYS:
        assert torch.equal(got[key], ref[key]), key
    assert torch.isfinite(ref["loss"]).all()
