"""GPU: the walk variants of the pruned solve (box tests and walk compiled per metric set; houv::walk_variant,
houv_amd/csrc/houv_math.h) against the brute-force kernel on the same spatially sorted clouds, bit for bit (integer views, so a NaN
compares as its bit pattern): optimiser state, score, loss, R, T, grad and cd after EVERY launch.  Launches of 1 + 7 + 50 + 3
iterations put dropped terms -- and so the variants -- across launch boundaries.  Clouds: tests/walk_variant_cases.py (plain
pairs at 320 / 512 / 768 / 2,048 / 2,500 points, a cropped target, points displaced along one axis, one NaN point, standing
still).  With houv_debug_set("solve_walk_hist") the walks count the masks they see: the cases together run every compiled set."""
import pytest
import torch

from tests import walk_variant_cases as wc

K = wc.K
_RUNS = {}


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _stage(name, f64, pruned, dev, hist=True, predict=0):
    """[(outputs, state)] after every launch; for a pruned stage also (walk histogram [16], solve_stats [8]) over its launches."""
    from houv_amd import _lib, ops, solver
    N, lr, _, pairs, launches, _, _ = wc.CASES[name]
    src, tgt = wc.gpu_clouds(name, dev)
    n = pairs * K
    state = torch.zeros((n, 24), dtype=torch.float64, device=dev)
    state[:, :8] = torch.as_tensor(solver.houv_init_params(n), dtype=torch.float64).to(dev)
    nn_ws = ops.solve_workspace(n, N, N, dev) if pruned else None
    walk = torch.zeros(16, dtype=torch.int64, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    done, res = 0, []
    try:
        if pruned:
            _lib.debug_set("solve_predict", predict)
            _lib.debug_set("solve_stats", stats.data_ptr())
            _lib.debug_set("solve_walk_hist", walk.data_ptr() if hist else 0)
        for it in launches:
            out = ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=it, angle_base=0, trans_mode=0, use_views=True,
                                    f64_params=f64, k_full=int(N * 0.5), k_view=N, lr=lr, loss_scale=1.0 / n, want_grad=True,
                                    want_cd=True, nn_ws=nn_ws, ws_valid=done > 0)
            res.append((out, state.clone()))
            done += it
        torch.cuda.synchronize()
    finally:
        _lib.debug_set("solve_walk_hist", 0)
        _lib.debug_set("solve_stats", 0)
        _lib.debug_set("solve_predict", 0)
    return res, [int(x) for x in walk.cpu()], [int(x) for x in stats.cpu()]


def _run(name, f64, pruned, dev):
    """A stage of a case: computed once, shared, never modified."""
    if (name, f64, pruned) not in _RUNS:
        _RUNS[(name, f64, pruned)] = _stage(name, f64, pruned, dev)
    return _RUNS[(name, f64, pruned)]


PARITY = [(n, f64) for n in sorted(wc.CASES) for f64 in wc.CASES[n][6]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,f64", PARITY, ids=[f"{n}-{'f64' if f else 'f32'}_params" for n, f in PARITY])
def test_pruned_solve_with_walk_variants_equals_brute_force(name, f64):
    from houv_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    N, _, kind, pairs, launches, variant, _ = wc.CASES[name]
    assert _lib.solve_variant(N, N, True, with_mode=True) == variant
    ref, _, _ = _run(name, f64, False, dev)
    got, walk, stats = _run(name, f64, True, dev)
    print(f"{name}: masks the walks saw {walk}")
    for launch, ((o, st), (o_ref, st_ref)) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(st), _bits(st_ref)), f"state after launch {launch} of {launches}"
        for key in ("score", "loss", "R", "T", "grad", "cd"):
            assert torch.equal(_bits(o[key]), _bits(o_ref[key])), f"{key} after launch {launch} of {launches}"
    last = ref[-1][0]["loss"]
    if kind == "nan":          # the NaN reaches pair 0's view terms and leaves pair 1 alone
        assert torch.isnan(last[:K]).all() and torch.isfinite(last[K:]).all()
    else:
        assert torch.isfinite(last).any()
    # one count per walking wave and sweep: the unit of solve_stats[2]
    assert sum(walk) == stats[2] and walk[0] == 0, (walk, stats)


@pytest.mark.gpu
def test_the_cases_together_run_every_compiled_variant():
    """Every compiled metric set is the walk_variant of a mask that some case's walks saw; the standing-still case saw each
    mask that the rule, restated on the CPU, produces for sure.  The counts are printed, not gated."""
    from houv_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    table = [_lib.solve_walk_variant(m) for m in range(16)]
    sets = sorted(set(table[1:]))
    assert 15 in sets and all(table[m] & m == m for m in range(16)), table
    total = [0] * 16
    for name, f64 in PARITY:
        _, walk, _ = _run(name, f64, True, dev)
        total = [a + b for a, b in zip(total, walk)]
    per_set = {s: sum(total[m] for m in range(1, 16) if table[m] == s) for s in sets}
    print(f"table {table}\nmasks the walks saw, all cases: {total}\nwave-sweeps per compiled set: {per_set}")
    assert all(c > 0 for c in per_set.values()), per_set
    for name in wc.STILL_CASES:
        _, walk, _ = _run(name, False, True, dev)
        missing = [m for m in sorted(wc.standing_still_masks(name) - {0}) if walk[m] == 0]
        assert not missing, f"{name}: the rule produces the masks {missing}, the walks did not see them: {walk}"


@pytest.mark.gpu
def test_walk_histogram_under_rescan_everything_and_switched_off():
    """Under solve_predict = 2 every term is computed on every iteration: only slot 15 counts.  With the switch off nothing is
    written."""
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    _, walk, stats = _stage("320_plain", False, True, dev, predict=2)
    assert walk[15] == stats[2] > 0 and sum(walk) == walk[15], (walk, stats)
    _, walk, stats = _stage("320_plain", False, True, dev, hist=False)
    assert walk == [0] * 16 and stats[2] > 0, (walk, stats)
