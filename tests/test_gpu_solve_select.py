"""GPU tests of the fused solve loop's top-k selection (select_smallest and repair_direction_a in solve.hip, select_threshold and
its tie rank in solve_large.hip, the radix passes of houv_solve.h) at every k, tie pattern and launch path.  The inputs, the
expected values and the bounds come from tests/solve_select_cases.py; tests/test_solve_select_host.py proves them on the CPU."""
import numpy as np
import pytest
import torch

import solve_select_cases as sc

pytestmark = pytest.mark.gpu
T = torch.tensor


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(src, tgt, state0, *, k_full, k_view=None, tm=0, f64=False, views=False, base=0, n_iters=1, **kw):
    """One launch on a fresh copy of the state; returns (out, state after the launch)."""
    from houv_amd import ops
    state = state0.clone()
    out = ops.solve_iterate(src, tgt, state, 1, steps_done=0, n_iters=n_iters, angle_base=base, trans_mode=tm, use_views=views,
                            f64_params=f64, k_full=k_full, k_view=src.shape[1] if k_view is None else k_view,
                            lr=0.1 if f64 else 0.01, loss_scale=1.0 / src.shape[0], want_grad=True, want_cd=True, **kw)
    return out, state


def _state(params, dev):
    st = torch.zeros((len(params), 24), dtype=torch.float64, device=dev)
    st[:, :8] = T(params).to(dev)
    return st


def _values(out):
    """[P,4] = cd0, cd1, score, loss of a no-view launch."""
    return torch.cat([out["cd"][:, :2], out["score"][:, None], out["loss"][:, None]], 1)


class _Exact:
    """Collects the launches of one path and compares them with the constructed values bit for bit, in one device comparison."""

    def __init__(self, names, ks, expected, dev):
        self.names, self.ks, self.exp, self.got = names, ks, T(expected).to(dev), {}
        self.eye = _bits(torch.eye(3, device=dev))

    def add(self, path, out):
        # the pose of the construction: R bitwise I, T bitwise +0 (move_point then returns the source's bits)
        assert bool((_bits(out["R"]) == self.eye).all()) and not bool(_bits(out["T"]).any()), path
        assert bool(torch.isfinite(out["grad"]).all()), path
        self.got.setdefault(path, []).append(_values(out))

    def check(self):
        for path, rows in self.got.items():
            got = torch.stack(rows)
            bad = (_bits(got) != _bits(self.exp)).nonzero().cpu().numpy()
            msg = [(path, "k=%d" % self.ks[i], self.names[p], ("cd0", "cd1", "score", "loss")[c],
                    float(got[i, p, c]), float(self.exp[i, p, c])) for i, p, c in bad[:8]]
            assert len(bad) == 0, (len(bad), msg)


def _tier_a_paths(dev, N, M, idx, lds=True, large=True, both_f64=True):
    """Every path of the issue for one Tier A shape.  The trans_mode / f64_params of the main runs alternate with the shape."""
    from houv_amd import _lib, ops, solver
    names, src_h, tgt_h, ks = sc.tier_a_batch(N, M)
    P = len(names)
    tm, f64 = idx % 2, bool((idx // 2) % 2)
    st = _state(sc.tier_a_params(P, tm, seed=idx), dev)
    src, tgt = T(src_h).to(dev), T(tgt_h).to(dev)
    chk = _Exact(names, ks, sc.tier_a_expected_batch(N, M, ks), dev)
    if lds:
        leaf = solver.sort_leaf(N, M)
        ssrc, stgt = solver.spatial_sort(src, leaf), solver.spatial_sort(tgt, leaf)
    for k in ks:
        kw = dict(k_full=k, tm=tm, f64=f64)
        if lds:
            grads = []
            try:
                for mode in (0, 1, 2):           # normal | every A-win through repair_direction_a | rescan everything
                    _lib.debug_set("solve_predict", mode)
                    out, _ = _launch(src, tgt, st, **kw)
                    chk.add("predict%d" % mode, out)
                    grads.append(out["grad"])
            finally:
                _lib.debug_set("solve_predict", 0)
            assert torch.equal(_bits(grads[0]), _bits(grads[1])) and torch.equal(_bits(grads[0]), _bits(grads[2])), k
            if both_f64:
                out, _ = _launch(src, tgt, st, k_full=k, tm=tm, f64=not f64)
                chk.add("f64_params=%d" % (not f64), out)
            # the pruned entry point on spatially sorted clouds (a permutation: the expected values do not change)
            ref, _ = _launch(ssrc, stgt, st, **kw)
            chk.add("sorted brute force", ref)
            for ws_valid in (False, "verify"):
                out, _ = _launch(ssrc, stgt, st, nn_ws=ops.solve_workspace(P, N, M, dev), ws_valid=ws_valid, **kw)
                chk.add("pruned ws_valid=%s" % ws_valid, out)
                assert torch.equal(_bits(out["grad"]), _bits(ref["grad"])), (k, ws_valid)
        if large:
            out, _ = _launch(src, tgt, st, large=True, **kw)
            chk.add("large", out)
            if both_f64:
                out, _ = _launch(src, tgt, st, large=True, k_full=k, tm=tm, f64=not f64)
                chk.add("large f64_params=%d" % (not f64), out)
    chk.check()


INLDS = sc.inlds_shapes()


@pytest.mark.parametrize("N,M", INLDS)
def test_tier_a_exact_selection_in_lds(dev, N, M):
    """Tier A at a full and a partial size of every row of the variant table, N == M and N != M: cd of both directions, score
    and loss are bit-identical to the constructed values for every named multiset and every k, through houv_solve_iterate
    under the three solve_predict modes, both f64_params, houv_solve_iterate_pruned (fresh workspace, and its verify mode) on
    sorted clouds and houv_solve_iterate_large; the gradient is finite and the same bits across the prediction modes and
    between brute force and pruned."""
    _tier_a_paths(dev, N, M, INLDS.index((N, M)))


@pytest.mark.parametrize("N,M", [s for s in sc.LARGE_SHAPES if s not in INLDS])
def test_tier_a_exact_selection_large_kernel(dev, N, M):
    """Tier A through houv_solve_iterate_large at its own sizes: one past the reference tile (1025), one past the query chunk
    (4097), N != M either way across chunks, and 16384 points once."""
    _tier_a_paths(dev, N, M, sc.LARGE_SHAPES.index((N, M)), lds=False, both_f64=max(N, M) < 16384)


@pytest.mark.parametrize("N", sc.VIEW_SIZES)
def test_tier_a_view_terms_under_ties(dev, N):
    """NMET = 4 under the tie patterns: offsets (m, m, m) u with m a power of 8, so that d = 3 m^2 u^2 (2 m^2 u^2 in a view) is
    exact and only the roots round.  The eight terms agree with their float64 values within (k+1) 2^-24 relative -- a quarter
    of what any swap across the cut changes (tests/test_solve_select_host.py) -- on every path, and the gradient is the same
    bits across the prediction modes and between brute force and pruned."""
    from houv_amd import _lib, ops, solver
    cases = [sc.tier_a_view_case(N, p) for p in sc.VIEW_PATTERNS]
    P = len(cases)
    src, tgt = T(np.stack([c["src"] for c in cases])).to(dev), T(np.stack([c["tgt"] for c in cases])).to(dev)
    st = _state(sc.tier_a_params(P, 0, seed=N), dev)
    leaf = solver.sort_leaf(N, N)
    ssrc, stgt = solver.spatial_sort(src, leaf), solver.spatial_sort(tgt, leaf)
    eye = _bits(torch.eye(3, device=dev))
    ks = sc.k_values(N, N, [k for c in cases for k in c["ks"]])
    got = {}
    for k in ks:
        kw = dict(k_full=k, k_view=N, views=True)
        runs = {}
        try:
            for mode in (0, 1, 2):
                _lib.debug_set("solve_predict", mode)
                runs["predict%d" % mode] = _launch(src, tgt, st, **kw)[0]
        finally:
            _lib.debug_set("solve_predict", 0)
        for mode in (1, 2):
            assert torch.equal(_bits(runs["predict%d" % mode]["grad"]), _bits(runs["predict0"]["grad"])), (k, mode)
        runs["sorted brute force"] = _launch(ssrc, stgt, st, **kw)[0]
        runs["pruned"] = _launch(ssrc, stgt, st, nn_ws=ops.solve_workspace(P, N, N, dev), **kw)[0]
        assert torch.equal(_bits(runs["pruned"]["grad"]), _bits(runs["sorted brute force"]["grad"])), k
        runs["large"] = _launch(src, tgt, st, large=True, **kw)[0]
        for path, out in runs.items():
            assert bool((_bits(out["R"]) == eye).all()) and not bool(_bits(out["T"]).any()), path
            assert bool(torch.isfinite(out["grad"]).all()), path
            got.setdefault(path, []).append(out["cd"].double())
    want = np.array([[sc.view_expected64(c, k, N).reshape(8) for c in cases] for k in ks])             # [nk, P, 8]
    bound = np.array([[[sc.view_bound(k)] * 2 + [sc.view_bound(N)] * 6] * P for k in ks]) * want
    worst = 0.0
    for path, rows in got.items():
        err = np.abs(torch.stack(rows).cpu().numpy() - want)
        worst = max(worst, float((err / bound).max()))
        bad = np.argwhere(err > bound)
        assert len(bad) == 0, (path, [(ks[i], sc.VIEW_PATTERNS[p], int(c), err[i, p, c], bound[i, p, c]) for i, p, c in bad[:8]])
    print(f"views under ties N={N}: worst error / bound = {worst:.3f}")


def _tier_b(dev, N, M, views, k_view, path, ks, base=1):
    """The Tier B comparison of one case over the k values `ks`; returns the worst (bound, half gap, error) for the record."""
    from houv_amd import _lib
    src_h, tgt_h, params = sc.tier_b_inputs(N, M)
    P = len(params)
    src, tgt, st = T(src_h).to(dev), T(tgt_h).to(dev), _state(params, dev)
    nn = sc.oracle_nn(src_h, tgt_h, params, base, 0, views)
    lists, figures = None, []
    for k in ks:
        kw = dict(k_full=k, k_view=k_view if views else k, views=views, base=base, large=(path == "large"))
        out, _ = _launch(src, tgt, st, **kw)
        if path == "lds":               # the three prediction modes agree bit for bit at every k
            try:
                for mode in (1, 2):
                    _lib.debug_set("solve_predict", mode)
                    o2, _ = _launch(src, tgt, st, **kw)
                    for key in ("cd", "score", "loss", "grad"):
                        assert torch.equal(_bits(o2[key]), _bits(out[key])), (k, mode, key)
            finally:
                _lib.debug_set("solve_predict", 0)
        if lists is None:               # the kernel's own fp32 R and T: they do not depend on k
            R, Tt = out["R"].cpu().numpy(), out["T"].cpu().numpy()
            lists = [sc.cd_reference(src_h[h], tgt_h[h], R[h], Tt[h], views) for h in range(P)]
        nmet = 4 if views else 1
        cd = out["cd"].cpu().numpy().astype(np.float64).reshape(P, 4, 2)[:, :nmet]
        bound, gap, err = 0.0, np.inf, 0.0
        for h, (d64, d32) in enumerate(lists):
            ref, b, g = sc.tier_b_bound_and_gap(d64, d32, k, k_view if views else k, min(N, M))
            bound, gap, err = max(bound, b), min(gap, g), max(err, float(np.abs(cd[h] - ref).max()))
        print(f"tier B ({N},{M},views={views},k_view={k_view},{path}) k={k}: bound {bound:.3e} half gap {gap:.3e} error {err:.3e}")
        figures.append((k, bound, gap, err))
        assert bound <= gap, (k, bound, gap)
        assert err <= bound, (k, err, bound)
        # the gradient: the rule of test_single_forward_backward_vs_oracle, unchanged
        want = sc.oracle_terms(src_h, tgt_h, params, base, 0, views, k, k_view if views else k, nn)
        g = out["grad"].cpu().numpy()
        scale = np.abs(want["grads"]).max(axis=1, keepdims=True)
        gerr = (np.abs(g - want["grads"]) / scale).max(axis=1)
        assert (gerr > 2e-4).sum() <= (1 if max(N, M) <= 1100 else 2), (k, gerr)
        assert gerr.max() < 3.0 / min(N, M), (k, gerr)
    return figures


@pytest.mark.parametrize("N,M,views,k_view,path", sc.TIER_B_CASES)
def test_tier_b_k_sweep_vs_float64(dev, N, M, views, k_view, path):
    """Generic poses and clouds at every k of the sweep: the two Chamfer terms against the float64 restatement under the
    kernel's own R and T, within four times the float32 restatement's loss (itself at most half the gap to the selections
    k-1 and k+1), and the parameter gradient against the autograd oracle at the same k."""
    _tier_b(dev, N, M, views, k_view, path, sc.k_values(N, M))


@pytest.mark.parametrize("N,M,k_view", sc.VIEW_CORNER_CASES)
def test_view_terms_with_unequal_clouds_and_partial_k_view(dev, N, M, k_view):
    """houv_solve_iterate accepts use_views with N != M and k_view < max(N, M): the view terms then select, too.  Tier B's
    comparison of all eight terms and of the gradient, over a sweep of k_full; houv_solve_iterate_large rejects the call."""
    from houv_amd import _lib
    _tier_b(dev, N, M, True, k_view, "lds", sorted({1, 2, N // 2, min(N, M) - 1, min(N, M), k_view}))
    src_h, tgt_h, params = sc.tier_b_inputs(N, M)
    with pytest.raises(_lib.HouvHipError, match="the view terms need N == M and k_view == N"):
        _launch(T(src_h).to(dev), T(tgt_h).to(dev), _state(params, dev), k_full=N // 2, k_view=k_view, views=True, large=True)


@pytest.mark.parametrize("N,views", [(700, True), (700, False), (2500, True), (2500, False)])
def test_pruned_equals_brute_force_at_other_k(dev, N, views):
    """The pruned search's term masks and picked_direction divide by k: five iterations at k_full = 1 and count-1 (balanced
    walk over sub-tiles at 700 points, over super-tiles at 2500) must equal the brute-force kernel bit for bit."""
    from houv_amd import _lib, ops, solver, synthetic
    P, K = 2, 26
    assert _lib.solve_variant(N, N, True, with_mode=True)[2] == (2 if N <= 2048 else 3)
    src, tgt, _ = synthetic.make_pairs(P, N, seed=31)
    leaf = solver.sort_leaf(N, N)
    src, tgt = solver.spatial_sort(src.to(dev), leaf), solver.spatial_sort(tgt.to(dev), leaf)
    st0 = _state(np.asarray(solver.houv_init_params(P * K)), dev)
    for k in (1, N - 1):
        res = []
        for ws in (None, ops.solve_workspace(P * K, N, N, dev)):
            state = st0.clone()
            out = ops.solve_iterate(src, tgt, state, K, steps_done=0, n_iters=5, angle_base=1, trans_mode=0, use_views=views,
                                    f64_params=False, k_full=k, k_view=N, lr=0.01, loss_scale=1.0 / (P * K), want_grad=True,
                                    want_cd=True, nn_ws=ws, ws_valid=False)
            res.append((out, state))
        for key in ("score", "loss", "R", "T", "grad", "cd"):
            assert torch.equal(_bits(res[0][0][key]), _bits(res[1][0][key])), (k, key)
        assert torch.equal(res[0][1], res[1][1]), k
