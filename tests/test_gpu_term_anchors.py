"""GPU: the pruned solve with per-term records (houv::term_anchor_masks, houv_amd/csrc/houv_math.h: a Chamfer term stays dropped
for as long as its own record and the winner's fresh one prove that it loses; solve.hip's kTermMaxAge, the limit on the iterations
in a row, is 0 = none) against
the brute-force kernel on the same spatially sorted clouds, bit for bit (integer views, so a NaN compares as its bit pattern):
optimiser state, score, loss, R, T, grad and cd after EVERY launch, fp32 and fp64 parameters.

Launch patterns: 1 + 30 + 9 + 20 iterations at lr 0.01 (drops that live across several NN refreshes -- every 4th iteration -- and
across 12 and more iterations, launch boundaries on and off the refreshes) and one launch of 60 iterations at lr 0.002 (slow
motion: drops that last most of the launch)."""
import pytest
import torch

LAUNCHES = (1, 30, 9, 20)
SLOW = (60,)
P, K = 2, 26
MAX_AGE = 0                                      # kTermMaxAge, solve.hip: 0 = a dropped term is never forced back
REL, ABS, MOVE = 1e-3, 1e-6, 1e-6                # kTermRel, kTermAbs, kTermMoveErr, houv_math.h

# name: (N, M, views, trans_mode, lr, kind, P, launches, expected (block, points per lane, prune mode))
CASES = {
    "320_views": (320, 320, True, 0, 0.01, "plain", P, LAUNCHES, (256, 2, 2)),
    "512_views": (512, 512, True, 0, 0.01, "plain", P, LAUNCHES, (256, 2, 2)),
    "512_views_slow": (512, 512, True, 0, 0.002, "plain", P, SLOW, (256, 2, 2)),
    "768_views": (768, 768, True, 0, 0.01, "plain", P, LAUNCHES, (256, 3, 2)),
    "768_views_slow": (768, 768, True, 0, 0.002, "plain", P, SLOW, (256, 3, 2)),
    "700x520_noviews": (700, 520, False, 0, 0.01, "plain", P, LAUNCHES, (256, 3, 2)),
    "700x520_noviews_slow": (700, 520, False, 0, 0.002, "plain", P, SLOW, (256, 3, 2)),
    "2500_views_super_tiles": (2500, 2500, True, 0, 0.01, "plain", 1, (1, 14), (1024, 3, 3)),
    "512_target_is_source": (512, 512, True, 0, 0.01, "same", P, LAUNCHES, (256, 2, 2)),
    "512_one_nan_point": (512, 512, True, 0, 0.01, "nan", P, LAUNCHES, (256, 2, 2)),
    "512_standing_still": (512, 512, True, 0, 1e-9, "plain", P, (1, 40), (256, 2, 2)),
}


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _clouds(name, dev):
    from houv_amd import solver, synthetic
    N, M, _, _, _, kind, pairs, _, _ = CASES[name]
    src, tgt, _ = synthetic.make_pairs(pairs, max(N, M), seed=91)
    src, tgt = src[:, :N].contiguous(), tgt[:, :M].contiguous()
    if kind == "same":         # all eight terms nearly tie once the pose is found; far apart before
        tgt = src.clone()
    leaf = solver.sort_leaf(N, M)
    src, tgt = solver.spatial_sort(src.to(dev), leaf), solver.spatial_sort(tgt.to(dev), leaf)
    if kind == "nan":
        src[0, 5, 0] = float("nan")
    return src, tgt


def _stage(src, tgt, p0, name, f64, pruned):
    """[(outputs, state)] after every launch."""
    from houv_amd import ops
    N, M, views, trans_mode, lr, _, pairs, launches, _ = CASES[name]
    n = pairs * K
    state = torch.zeros((n, 24), dtype=torch.float64, device=src.device)
    state[:, :8] = torch.as_tensor(p0, dtype=torch.float64).to(src.device)
    nn_ws = ops.solve_workspace(n, N, M, src.device) if pruned else None
    done, res = 0, []
    for it in launches:
        out = ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=it, angle_base=0, trans_mode=trans_mode,
                                use_views=views, f64_params=f64, k_full=int(N * 0.5), k_view=N, lr=lr, loss_scale=1.0 / n,
                                want_grad=True, want_cd=True, nn_ws=nn_ws, ws_valid=done > 0)
        res.append((out, state.clone()))
        done += it
    return res


_BRUTE = {}


def _brute(name, f64, dev):
    """The brute-force stage of a case: computed once, shared, never modified."""
    from houv_amd import solver
    if (name, f64) not in _BRUTE:
        src, tgt = _clouds(name, dev)
        p0 = solver.houv_init_params(CASES[name][6] * K)
        _BRUTE[(name, f64)] = (src, tgt, p0, _stage(src, tgt, p0, name, f64, pruned=False))
    return _BRUTE[(name, f64)]


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [False, True], ids=["f32_params", "f64_params"])
@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "512_standing_still"))
def test_pruned_solve_with_term_records_equals_brute_force(name, f64):
    from houv_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    N, M, _, _, _, kind, pairs, launches, variant = CASES[name]
    assert _lib.solve_variant(N, M, True, with_mode=True) == variant
    src, tgt, p0, ref = _brute(name, f64, dev)
    got = _stage(src, tgt, p0, name, f64, pruned=True)
    for launch, ((o, st), (o_ref, st_ref)) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(st), _bits(st_ref)), f"state after launch {launch} of {launches}"
        for key in ("score", "loss", "R", "T", "grad", "cd"):
            assert torch.equal(_bits(o[key]), _bits(o_ref[key])), f"{key} after launch {launch} of {launches}"
    last = ref[-1][0]["loss"]
    if kind == "nan":          # the NaN reaches pair 0's view terms and leaves pair 1 alone
        assert torch.isnan(last[:K]).all() and torch.isfinite(last[K:]).all()
    elif kind == "same":       # a point that lands exactly on its twin has d = 0: 0 * inf = NaN in the gradient, as torch's sqrt
        assert torch.isfinite(last).any()   # backward gives; the brute-force kernel yields the same bits, finite or not
    else:
        assert torch.isfinite(last).all()


def _counted_stage(src, tgt, p0, name, mode, dev):
    """Counters [6] terms computed, [7] terms possible per launch of the pruned stage, and its results."""
    from houv_amd import _lib, ops
    N, M, views, trans_mode, lr, _, pairs, launches, _ = CASES[name]
    n = pairs * K
    state = torch.zeros((n, 24), dtype=torch.float64, device=dev)
    state[:, :8] = torch.as_tensor(p0, dtype=torch.float64).to(dev)
    nn_ws = ops.solve_workspace(n, N, M, dev)
    done, counts, res = 0, [], []
    try:
        _lib.debug_set("solve_predict", mode)
        for it in launches:
            buf = torch.zeros(8, dtype=torch.int64, device=dev)
            _lib.debug_set("solve_stats", buf.data_ptr())
            out = ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=it, angle_base=0, trans_mode=trans_mode,
                                    use_views=views, f64_params=False, k_full=int(N * 0.5), k_view=N, lr=lr, loss_scale=1.0 / n,
                                    want_grad=True, want_cd=True, nn_ws=nn_ws, ws_valid=done > 0)
            torch.cuda.synchronize()
            _lib.debug_set("solve_stats", 0)
            v = [int(x) for x in buf.cpu()]
            counts.append((v[6], v[7]))
            res.append((out, state.clone()))
            done += it
    finally:
        _lib.debug_set("solve_stats", 0)
        _lib.debug_set("solve_predict", 0)
    return counts, res


@pytest.mark.gpu
def test_standing_still_every_clear_loser_is_dropped_on_every_iteration_but_the_first_and_the_last():
    """lr = 1e-9: the pose effectively stands still (40 steps of 1e-9 move a point by < 1e-7, and cd with it), so the rule's
    slack is its margin  kTermRel (cd_0 + cd_1) + kTermAbs + kTermMoveErr (2 radius + 2 |T|)  alone.  From the brute-force cd of the
    1-iteration launch: a (hypothesis, metric) whose gap exceeds 1.01 margins has a loser that MUST be dropped, one whose gap is
    below 0.99 margins cannot be.  In the 40-iteration launch the first and the last iteration compute every term; a loser is
    dropped in iterations 1..38 except where a kTermMaxAge > 0 forces it back (every (kTermMaxAge + 1)-th: with 12, iterations 13
    and 26), so 38 times with kTermMaxAge = 0.  The computed-term counter of that launch must lie between the two counts; under
    solve_predict = 2 every term is computed."""
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    name = "512_standing_still"
    n, n_it = P * K, CASES[name][7][1]
    src, tgt, p0, ref = _brute(name, False, dev)
    cd = ref[0][0]["cd"].double().cpu().view(n, 4, 2)
    T = ref[0][0]["T"].double().cpu().view(n, 3).norm(dim=1)
    radius = src.double().cpu().norm(dim=2).max(dim=1)[0].repeat_interleave(K) * 1.000001
    margin = REL * (cd[:, :, 0].abs() + cd[:, :, 1].abs()) + (ABS + MOVE * (2.0 * radius + 2.0 * T))[:, None]
    gap = (cd[:, :, 0] - cd[:, :, 1]).abs()
    sure, maybe = int((gap > 1.01 * margin).sum()), int((gap > 0.99 * margin).sum())
    in_band = maybe - sure
    print(f"{n * 4} (hypothesis, metric) pairs: {sure} clear losers, {in_band} within 1 % of the threshold")
    assert in_band * 10 <= n * 4, "too many pairs in the band: pick another seed"
    assert sure * 10 >= n * 4, "the case does not engage the rule"
    dropped_each = (n_it - 2) - ((n_it - 2) // (MAX_AGE + 1) if MAX_AGE else 0)      # iterations 1..38 without forced returns
    assert dropped_each == 38
    counts, got = _counted_stage(src, tgt, p0, name, 0, dev)
    for launch, ((o, st), (o_ref, st_ref)) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(st), _bits(st_ref)), f"state after launch {launch}"
        for key in ("score", "loss", "R", "T", "grad", "cd"):
            assert torch.equal(_bits(o[key]), _bits(o_ref[key])), f"{key} after launch {launch}"
    print(f"terms computed / possible per launch: {counts}")
    assert counts[0] == (n * 8, n * 8), counts                      # a 1-iteration launch computes every term
    computed, possible = counts[1]
    assert possible == n * n_it * 8, counts
    assert possible - dropped_each * maybe <= computed <= possible - dropped_each * sure, (counts, sure, maybe)
    counts2, _ = _counted_stage(src, tgt, p0, name, 2, dev)
    assert counts2[1] == (possible, possible), counts2
