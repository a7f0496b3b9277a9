"""GPU: the pruned solve with the group cull of its box tests (prune_masks, houv_amd/csrc/houv_sweep.h; houv::box_test_group,
houv_math.h) against the brute-force kernel on the same spatially sorted clouds, bit for bit (integer views, so a NaN compares as
its bit pattern): optimiser state, score, loss, R, T, grad and cd after EVERY launch of 1 + 7 + 50 + 3 iterations.  Shapes: 257
points (nine tiles: a partial last tile and a partial last group), 320, 768, 2,048 (survivors in both words of a mask) and 2,500
(super-tiles); a single-metric case with N != M; a cloud with a NaN point and one with all points of a tile equal.
houv_debug_set("solve_cull_stats") counts what the cull did: it must have skipped tests, and its totals must add up."""
import pytest
import torch

K = 26
LAUNCHES = (1, 7, 50, 3)

# name: (N, M, pairs, with views, kind, expected (block, points per lane, prune mode), parameter precisions)
CASES = {
    "257_partial_tile_and_group": (257, 257, 2, True, "plain", (256, 2, 2), (False,)),
    "320": (320, 320, 2, True, "plain", (256, 2, 2), (False,)),
    "768": (768, 768, 2, True, "plain", (256, 3, 2), (False,)),
    "2048_both_mask_words": (2048, 2048, 1, True, "plain", (512, 4, 2), (False, True)),
    "2500_super_tiles": (2500, 2500, 1, True, "plain", (1024, 3, 3), (False,)),
    "600x450_single_metric": (600, 450, 2, False, "plain", (256, 3, 2), (False,)),
    "512_one_nan_point": (512, 512, 2, True, "nan", (256, 2, 2), (False,)),
    "512_a_tile_of_equal_points": (512, 512, 2, True, "equal", (256, 2, 2), (False,)),
}
_RUNS = {}


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _clouds(name, dev):
    from houv_amd import solver, synthetic
    N, M, pairs, _, kind, _, _ = CASES[name]
    src, tgt, _ = synthetic.make_pairs(pairs, max(N, M), seed=77)
    src, tgt = src[:, :N].contiguous(), tgt[:, :M].contiguous()
    leaf = solver.sort_leaf(N, M)
    src, tgt = solver.spatial_sort(src.to(dev), leaf), solver.spatial_sort(tgt.to(dev), leaf)
    if kind == "nan":
        src[0, 5, 0] = float("nan")
    elif kind == "equal":          # tile 3 of both clouds of pair 0 collapses to one point: degenerate boxes, exact ties
        src[0, 96:128] = src[0, 100].clone()
        tgt[0, 96:128] = tgt[0, 97].clone()
    return src, tgt


def _stage(name, f64, pruned, dev, cull_from=None, predict=0, cull_on=True):
    """[(outputs, state)] after every launch; for a pruned stage also solve_cull_stats [4] and solve_stats [8], counted over the
    launches from index `cull_from` on (None: never)."""
    from houv_amd import _lib, ops, solver
    N, M, pairs, views, _, _, _ = CASES[name]
    src, tgt = _clouds(name, dev)
    n = pairs * K
    state = torch.zeros((n, 24), dtype=torch.float64, device=dev)
    state[:, :8] = torch.as_tensor(solver.houv_init_params(n), dtype=torch.float64).to(dev)
    nn_ws = ops.solve_workspace(n, N, M, dev) if pruned else None
    cull = torch.full((4,), 7, dtype=torch.int64, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    done, res = 0, []
    try:
        _lib.debug_set("solve_predict", predict)
        for i, it in enumerate(LAUNCHES):
            if pruned and cull_from is not None and i == cull_from:
                cull.zero_()
                _lib.debug_set("solve_stats", stats.data_ptr())
                _lib.debug_set("solve_cull_stats", cull.data_ptr() if cull_on else 0)
            out = ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=it, angle_base=0, trans_mode=0, use_views=views,
                                    f64_params=f64, k_full=int(min(N, M) * 0.5), k_view=min(N, M), lr=0.01, loss_scale=1.0 / n,
                                    want_grad=True, want_cd=True, nn_ws=nn_ws, ws_valid=done > 0)
            res.append((out, state.clone()))
            done += it
        torch.cuda.synchronize()
    finally:
        _lib.debug_set("solve_cull_stats", 0)
        _lib.debug_set("solve_stats", 0)
        _lib.debug_set("solve_predict", 0)
    return res, [int(x) for x in cull.cpu()], [int(x) for x in stats.cpu()]


def _run(name, f64, pruned, dev):
    """A stage of a case: computed once, shared, never modified.  The pruned stage counts from its second launch on: every sweep
    counted starts from a valid workspace."""
    if (name, f64, pruned) not in _RUNS:
        _RUNS[(name, f64, pruned)] = _stage(name, f64, pruned, dev, cull_from=1 if pruned else None)
    return _RUNS[(name, f64, pruned)]


def _check_totals(name, cull, stats):
    """groups, boxes surviving, per-query tests executed, per-query tests of a loop over all boxes (the last two per lane)."""
    N, M, _, _, _, (block, q, mode), _ = CASES[name]
    groups, surviving, executed, full = cull
    print(f"{name}: groups {groups}, boxes surviving {surviving}, tests executed {executed}, of a full loop {full}: "
          f"{100.0 * executed / max(full, 1):.1f} %")
    assert groups == q * stats[2] > 0, "one group per k of every walking wave and sweep (the unit of solve_stats[2])"
    assert executed == 64 * surviving, "one test per lane and surviving box"
    assert executed < full, "the cull skipped nothing"
    if N == M:
        ntile = (N + (64 if mode == 3 else 32) - 1) // (64 if mode == 3 else 32)
        assert full == 64 * ntile * groups
        skipped = 64 * (groups * ntile - surviving)
        assert executed + skipped == full


PARITY = [(n, f64) for n in CASES for f64 in CASES[n][6]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,f64", PARITY, ids=[f"{n}-{'f64' if f else 'f32'}_params" for n, f in PARITY])
def test_pruned_solve_with_group_cull_equals_brute_force_after_every_launch(name, f64):
    from houv_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    N, M, _, _, kind, variant, _ = CASES[name]
    assert _lib.solve_variant(N, M, True, with_mode=True) == variant
    ref, _, _ = _run(name, f64, False, dev)
    got, cull, stats = _run(name, f64, True, dev)
    for launch, ((o, st), (o_ref, st_ref)) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(st), _bits(st_ref)), f"state after launch {launch} of {LAUNCHES}"
        for key in ("score", "loss", "R", "T", "grad", "cd"):
            assert torch.equal(_bits(o[key]), _bits(o_ref[key])), f"{key} after launch {launch} of {LAUNCHES}"
    last = ref[-1][0]["loss"]
    if kind == "nan":          # the NaN reaches pair 0's view terms and leaves pair 1 alone
        assert torch.isnan(last[:K]).all() and torch.isfinite(last[K:]).all()
    else:
        assert torch.isfinite(last).all()
    _check_totals(name, cull, stats)


@pytest.mark.gpu
def test_cull_counters_from_a_valid_workspace_add_up_also_under_rescan_everything():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    for predict in (0, 2):
        _, cull, stats = _stage("320", False, True, dev, cull_from=1, predict=predict)
        assert stats[3] == 0, "no brute-force sweep after the first launch"
        _check_totals("320", cull, stats)


@pytest.mark.gpu
def test_cull_counters_switched_off_leave_their_buffer_untouched():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    _, cull, stats = _stage("320", False, True, dev, cull_from=1, cull_on=False)
    assert cull == [0, 0, 0, 0] and stats[2] > 0, (cull, stats)
    _, cull, _ = _stage("320", False, True, dev, cull_from=None)
    assert cull == [7, 7, 7, 7], cull
