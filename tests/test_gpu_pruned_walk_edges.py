"""Edges of the pruned solve's balanced walk: the list pop on 32-bit halves, the branch-free unit bookkeeping (strict <, ascending
units), the per-wave bin scan of the counting sort and the empty-list bin.  Every GPU case compares the pruned search with the
brute-force kernel on the same spatially sorted clouds, bit for bit (integer views, so NaN compares as its bit pattern): score,
loss, R, T, cd, grad and the optimiser state, over 6 iterations in launches of 3 (a chunk boundary, refresh iterations 0 and 4,
non-refresh iterations between).

1024 x 1000 cannot run with the view terms (run_stage raises on N != M with views, as the reference does), so the 32-sub-tile
edge is covered three ways: 1024 x 1000 without views, and 1024 x 1024 and 1000 x 1000 (last block partly filled) with them."""
import numpy as np
import pytest
import torch

P, K, ITERS, CHUNK = 2, 26, 6, 3

# name: (N, M, views, f64, kind, expected (block, points per lane, prune mode))
CASES = {
    "257_views": (257, 257, True, False, "plain", (256, 2, 2)),
    "1024x1000_noviews": (1024, 1000, False, False, "plain", (256, 4, 2)),
    "1024_views": (1024, 1024, True, False, "plain", (256, 4, 2)),
    "1000_views": (1000, 1000, True, False, "plain", (256, 4, 2)),
    "1025_views": (1025, 1025, True, False, "plain", (512, 3, 2)),
    "1300x1000_noviews_f64": (1300, 1000, False, True, "plain", (512, 3, 2)),
    "2049_views": (2049, 2049, True, False, "plain", (1024, 3, 3)),
    "duplicates": (1000, 1000, True, False, "dup", (256, 4, 2)),
    "three_points": (1200, 1200, True, False, "three", (512, 3, 2)),
    "nan": (640, 640, True, False, "nan", (256, 3, 2)),
}


def _clouds(name):
    """CPU clouds of a case, before the spatial sort."""
    from houv_amd import synthetic
    N, M, _, _, kind, _ = CASES[name]
    src, tgt, _ = synthetic.make_pairs(P, max(N, M), seed=77)
    src, tgt = src[:, :N].contiguous(), tgt[:, :M].contiguous()
    if kind == "dup":          # exact ties: 64 target points twice
        tgt[:, 64:128] = tgt[:, 0:64]
    if kind == "three":        # 400 copies of 3 distinct points: every query has the same list length
        src = src[:, :3].repeat(1, 400, 1).contiguous()
        tgt = tgt[:, :3].repeat(1, 400, 1).contiguous()
    return src, tgt


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_sort_is_the_torch_sort(name):
    """CPU: spatial_sort of a CPU cloud is kd_sort's order, bit for bit, same shape and dtype -- and a permutation of the input."""
    from houv_amd import solver
    N, M, _, _, _, _ = CASES[name]
    leaf = solver.sort_leaf(N, M)
    for c in _clouds(name):
        a, b = solver.spatial_sort(c.clone(), leaf), solver.kd_sort(c.clone(), leaf)
        assert a.dtype == torch.float32 and a.shape == c.shape and torch.equal(_bits(a), _bits(b))
        key = lambda x: sorted(map(tuple, x[0].tolist()))
        assert key(a) == key(c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_pruned_walk_equals_brute_force(name):
    from houv_amd import _lib, solver
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    N, M, views, f64, kind, variant = CASES[name]
    assert _lib.solve_variant(N, M, True, with_mode=True) == variant
    leaf = solver.sort_leaf(N, M)
    src_c, tgt_c = _clouds(name)
    src, tgt = solver.spatial_sort(src_c.to(dev), leaf), solver.spatial_sort(tgt_c.to(dev), leaf)
    # the device sort returns the host sort's bits
    assert torch.equal(_bits(src.cpu()), _bits(solver.kd_sort(src_c.clone(), leaf)))
    assert torch.equal(_bits(tgt.cpu()), _bits(solver.kd_sort(tgt_c.clone(), leaf)))
    if kind == "dup":          # the ties must straddle tracking units (16 references) and sub-tiles (32) for the rule to matter
        where = {}
        for i, pt in enumerate(map(tuple, tgt[0].cpu().tolist())):
            where.setdefault(pt, []).append(i)
        ties = [v for v in where.values() if len(v) > 1]
        assert len(ties) == 64 and any(v[0] // 16 != v[-1] // 16 for v in ties) and any(v[0] // 32 != v[-1] // 32 for v in ties)
    if kind == "nan":          # one NaN coordinate in pair 0's source; the tensor keeps its order and stays marked as sorted
        src[0, 5, 0] = float("nan")
        solver._mark_sorted(src, leaf)
    p0 = solver.houv_init_params(P * K) if not f64 else np.random.default_rng(1).standard_normal((P * K, 8))
    kw = dict(angle_base=1, trans_mode=0, use_views=views, f64_params=f64, lr=0.1 if f64 else 0.01, want_grad=True, want_cd=True,
              iters_per_launch=CHUNK)
    ref, st_ref = solver.run_stage(src, tgt, p0, K, ITERS, pruned=False, **kw)
    out, st = solver.run_stage(src, tgt, p0, K, ITERS, pruned=True, **kw)
    for key in ("score", "loss", "R", "T", "cd", "grad"):
        assert torch.equal(_bits(out[key]), _bits(ref[key])), key
    assert torch.equal(_bits(st), _bits(st_ref))
    if kind == "nan":          # the NaN reaches pair 0's view terms and leaves pair 1 alone
        assert torch.isnan(ref["loss"][:K]).all() and torch.isfinite(ref["loss"][K:]).all()
    elif kind != "three":
        assert torch.isfinite(ref["loss"]).all()
