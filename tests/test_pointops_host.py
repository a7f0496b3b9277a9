"""CPU: the host restatements of the point-op contracts (tests/pointops_host.py) against independent formulations, and the
public names the reference imports from `mm3d_pn2` and `model_utils_completion`."""
import numpy as np
import pytest
import torch

import pointops_host as host


@pytest.mark.parametrize("N", [1500, 5000])
def test_fps_float32_equals_float64_on_the_lattice(N):
    """On the 1/8 lattice every distance is exact in both types, so the two runs must pick the same points; there are 512
    sites at most, so the 600 picks run out of distinct points: from then on every running minimum is 0 and the pick is 0."""
    B, m = 2, 600
    x = host.fps_cloud(B, N, "lattice")
    assert np.array_equal(x * 8, np.round(x * 8)) and x.min() >= 0 and x.max() < 1
    for b in range(B):
        sites = len(np.unique(x[b], axis=0))
        assert sites <= 512 < m
        a = host.fps(x[b], m)
        assert a.dtype == np.int32 and np.array_equal(a, host.fps(x[b], m, np.float64))
        assert np.array_equal(a, host.fps_expected(B, N, m, "lattice")[b])
        assert len(set(a[:sites].tolist())) == sites and (a[sites:] == 0).all()
        # a tie is broken towards the lowest index: every pick is the first occurrence of its site
        first = {}
        for i, p in enumerate(map(tuple, x[b])):
            first.setdefault(p, i)
        assert all(first[tuple(x[b, i])] == i for i in a[:sites])


def test_fps_starts_at_point_zero_and_from_1e10():
    x = np.array([[0, 0, 0], [3e5, 0, 0], [1, 0, 0]], np.float32)       # 9e10 > 1e10: the start value caps the first minimum
    assert host.fps(x, 3).tolist() == [0, 1, 2]
    assert host.fps(x[:1], 1).tolist() == [0]


def test_ball_query_restatement_against_float64_mask():
    """Inputs with margins: coordinates on a 1/64 grid make every squared distance exact in fp32 and in float64, so the hit
    sets of the two agree exactly; the slots then follow from the sets."""
    rng = np.random.default_rng(7)
    xyz = (rng.integers(0, 64, (2, 400, 3)) / 64.0).astype(np.float32)
    ctr = (rng.integers(0, 64, (2, 37, 3)) / 64.0).astype(np.float32)
    ctr[0, 0] = xyz[0, 5]                                    # a centre on a point: d2 == 0 is a hit below min_radius
    ctr[1, 3] = 9.0                                          # nothing in reach
    lo, hi, ns = 0.125, 0.25, 16
    idx, cnt = host.ball_query(xyz, ctr, lo, hi, ns)
    d2 = ((ctr.astype(np.float64)[:, :, None] - xyz.astype(np.float64)[:, None]) ** 2).sum(-1)
    hit = (d2 == 0) | ((d2 >= lo * lo) & (d2 < hi * hi))
    assert hit[0, 0, 5] and cnt[1, 3] == 0 and (idx[1, 3] == 0).all()
    seen_short = seen_full = False
    for b in range(2):
        for c in range(37):
            want = np.flatnonzero(hit[b, c])
            n = min(len(want), ns)
            assert cnt[b, c] == n
            assert (idx[b, c, :n] == want[:n]).all()
            assert (idx[b, c, n:] == (want[0] if n else 0)).all()
            seen_short |= 0 < len(want) < ns
            seen_full |= len(want) > ns
    assert seen_short and seen_full


def test_ball_query_bounds_are_inclusive_below_and_strict_above():
    xyz = np.array([[[0.25, 0, 0], [0.5, 0, 0], [0.125, 0, 0], [0, 0, 0], [0.375, 0, 0]]], np.float32)
    idx, cnt = host.ball_query(xyz, np.zeros((1, 1, 3), np.float32), 0.25, 0.5, 4)
    assert cnt[0, 0] == 3 and idx[0, 0].tolist() == [0, 3, 4, 0]      # 0.25 in, 0.5 out, 0.125 out, the centre itself in


def test_three_interpolate_restatement():
    rng = np.random.default_rng(1)
    f = rng.standard_normal((2, 5, 30)).astype(np.float32)
    idx = rng.integers(0, 30, (2, 11, 3))
    w = rng.random((2, 11, 3)).astype(np.float32)
    out = host.three_interpolate(f, idx, w)
    ref = np.einsum("bcnj,bnj->bcn", np.stack([f[b][:, idx[b]] for b in range(2)]).astype(np.float64), w.astype(np.float64))
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("S,weighted", [(1, False), (3, True), (1, True)])
def test_scatter_restatement_is_the_ordered_loop_and_close_to_float64(S, weighted):
    rng = np.random.default_rng(S + 10 * weighted)
    B, C, N, M = 2, 3, 17, 60 * S
    g = rng.standard_normal((B, C, M // S)).astype(np.float32)
    g[0, 0, :4] = -0.0
    idx = rng.integers(0, N - 2, (B, M))                      # destination N-2 receives nothing
    if S == 1 and not weighted:
        idx[0, :4] = N - 1                                    # four -0 terms: a sum started from the first term stays -0
    w = rng.random((B, M)).astype(np.float32) if weighted else None
    a = host.scatter_points_grad(g, idx, w, N, S)
    b = host.scatter_points_grad_loop(g, idx, w, N, S)
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    terms = torch.from_numpy(g).double()[:, :, torch.arange(M) // S]
    if weighted:
        terms = terms * torch.from_numpy(w).double()[:, None]
    ref = torch.zeros(B, C, N, dtype=torch.float64)
    for i in range(B):
        ref[i].index_add_(1, torch.from_numpy(idx[i]), terms[i])
    # a list of n fp32 terms summed sequentially errs by at most (n-1) eps * sum|t| (+ eps per product): n <= M here
    np.testing.assert_allclose(a, ref.numpy(), rtol=1e-5, atol=1e-5 * M)
    assert (a[:, :, N - 2] == 0).all()
    if S == 1 and not weighted:
        assert a[0, 0, N - 1] == 0 and np.signbit(a[0, 0, N - 1])


def test_public_names_exist():
    from houv_amd import mm3d_pn2, model_utils_completion
    for name in ("furthest_point_sample", "gather_points", "grouping_operation", "ball_query", "three_nn", "three_interpolate",
                 "QueryAndGroup", "GroupAll"):
        assert callable(getattr(mm3d_pn2, name)), name
    for name in ("knn_point", "knn", "edge_preserve_sampling", "get_repulsion_loss", "get_uniform_loss", "symmetric_sample",
                 "three_nn_upsampling"):
        assert callable(getattr(model_utils_completion, name)), name


def test_new_ops_and_helpers_refuse_cpu_tensors():
    from houv_amd import _lib, mm3d_pn2 as pn2, model_utils_completion as muc
    x = torch.rand(2, 64, 3)
    f = torch.rand(2, 4, 64)
    i3 = torch.zeros(2, 8, 3, dtype=torch.int32)
    calls = [lambda: pn2.ball_query(0, 0.2, 8, x, x[:, :5].contiguous()),
             lambda: pn2.grouping_operation(f, i3),
             lambda: pn2.three_interpolate(f, i3, torch.rand(2, 8, 3)),
             lambda: pn2.QueryAndGroup(0.2, 8)(x, x[:, :5].contiguous(), f),
             lambda: muc.knn_point(2, x, x),
             lambda: muc.knn(x.transpose(1, 2).contiguous(), 8),
             lambda: muc.edge_preserve_sampling(f, x, 16),
             lambda: muc.get_repulsion_loss(x),
             lambda: muc.get_uniform_loss(torch.rand(1, 2048, 3)),
             lambda: muc.symmetric_sample(x, 16),
             lambda: muc.three_nn_upsampling(x, x[:, :9].contiguous())]
    for call in calls:
        with pytest.raises(_lib.HouvHipError):
            call()
    assert pn2.GroupAll()(x, None, f).shape == (2, 7, 1, 64)          # pure torch: runs anywhere
    with pytest.raises(NotImplementedError):
        pn2.QueryAndGroup(0.2, 8, uniform_sample=True)
