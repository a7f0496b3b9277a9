"""GPU: the pruned solve with term masks (a Chamfer term that provably loses its metric's min is not computed: houv::term_masks,
houv_amd/csrc/houv_math.h) against the brute-force kernel on the same spatially sorted clouds, bit for bit (integer views, so a
NaN compares as its bit pattern -- stricter than torch.equal): optimiser state, score, loss, R, T, grad and cd after EVERY launch.
A stage is run as launches of 1 + 7 + 50 + 3 iterations, so that launch boundaries fall on and off the every-4th-iteration
anchors (steps 0 | 1..7 | 8..57 | 58..60), with fp32 and fp64 parameters."""
import pytest
import torch

LAUNCHES = (1, 7, 50, 3)
P, K = 2, 26

# name: (N, M, views, trans_mode, lr, kind, P, launches, expected (block, points per lane, prune mode))
CASES = {
    "320_views": (320, 320, True, 0, 0.01, "plain", P, LAUNCHES, (256, 2, 2)),
    "512_views": (512, 512, True, 0, 0.01, "plain", P, LAUNCHES, (256, 2, 2)),
    "768_views": (768, 768, True, 0, 0.01, "plain", P, LAUNCHES, (256, 3, 2)),
    "512_single_metric_solve_twin": (512, 512, False, 1, 0.1, "plain", P, LAUNCHES, (256, 2, 2)),
    "2500_views_super_tiles": (2500, 2500, True, 0, 0.01, "plain", 1, (1, 7), (1024, 3, 3)),
    "512_target_is_source": (512, 512, True, 0, 0.01, "same", P, LAUNCHES, (256, 2, 2)),
    "512_one_nan_point": (512, 512, True, 0, 0.01, "nan", P, LAUNCHES, (256, 2, 2)),
    "700x520_noviews": (700, 520, False, 0, 0.01, "plain", P, LAUNCHES, (256, 3, 2)),
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


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [False, True], ids=["f32_params", "f64_params"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_pruned_solve_with_term_masks_equals_brute_force(name, f64):
    from houv_amd import _lib, solver
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    N, M, _, _, _, kind, pairs, launches, variant = CASES[name]
    assert _lib.solve_variant(N, M, True, with_mode=True) == variant
    src, tgt = _clouds(name, dev)
    p0 = solver.houv_init_params(pairs * K)
    ref = _stage(src, tgt, p0, name, f64, pruned=False)
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


@pytest.mark.gpu
def test_term_masks_engage_and_switch_off_under_rescan_everything():
    """The counters of houv_debug_set("solve_stats"): [6] terms computed, [7] terms possible, per workgroup-iteration.  On the
    512-point case with views some terms are dropped (share < 1); under solve_predict = 2 ("every term, every rescan") none.
    The share itself is a measurement, not a gate."""
    from houv_amd import _lib, solver
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    name = "512_views"
    src, tgt = _clouds(name, dev)
    p0 = solver.houv_init_params(P * K)
    share = {}
    try:
        for mode in (0, 2):
            buf = torch.zeros(8, dtype=torch.int64, device=dev)
            _lib.debug_set("solve_predict", mode)
            _lib.debug_set("solve_stats", buf.data_ptr())
            _stage(src, tgt, p0, name, False, pruned=True)
            torch.cuda.synchronize()
            _lib.debug_set("solve_stats", 0)
            v = [int(x) for x in buf.cpu()]
            assert v[7] == P * K * sum(LAUNCHES) * 8, v
            share[mode] = (v[6], v[7])
            print(f"solve_predict={mode}: {v[6]} of {v[7]} terms computed ({v[6] / v[7]:.4f})")
    finally:
        _lib.debug_set("solve_stats", 0)
        _lib.debug_set("solve_predict", 0)
    assert share[0][0] < share[0][1], share
    assert share[2][0] == share[2][1], share
