"""CPU: the host restatements of tests/dcp_ops_host.py against independent formulations, the properties of the seeded inputs that
tests/test_gpu_dcp_ops.py relies on (no distance ties in the k-NN clouds; planted duplicates in different quarters and stages),
and the errors of the fp32 torch compositions that bound the kernels there (printed with -s; DESIGN.md records them)."""
import numpy as np
import pytest
import torch

import dcp_ops_host as host


# ---------------------------------------------------------------------------------------------------------------------
# k-NN
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k", [(20, 20), (64, 8), (300, 20), (513, 16), (1025, 3)])
def test_knn_host_function_equals_float64_brute_force(N, k):
    """hm_knn_fmaf against dcp.py:35-42 in float64 on clouds without near-ties: every list the same set in the same order."""
    x = host.knn_cloud(N)
    idx, dist = host.knn_host(x, k)
    ref = host.knn_float64(x, k)
    assert torch.equal(idx, ref)
    assert bool((idx[..., 0] == torch.arange(N)).all()) and float(dist[..., 0].abs().max()) == 0.0
    # the distances are the fused form of metric_sqdist<0>: within one rounding of float64 on the same differences
    d = x.unsqueeze(1).expand(-1, N, -1, -1).gather(2, idx.unsqueeze(-1).expand(-1, -1, -1, 3)) - x.unsqueeze(2)
    assert d.dtype == torch.float32
    exact = (d.double() ** 2).sum(-1)
    assert bool(((dist.double() - exact).abs() <= 3 * host.EPS32 * exact).all())     # three roundings of non-negative terms


def test_knn_host_function_is_lexicographic_on_ties():
    x = torch.zeros(1, 6, 3)
    x[0, :, 0] = torch.tensor([0.0, 1.0, -1.0, 1.0, 2.0, -1.0])      # from point 0: d = 0, 1, 1, 1, 4, 1
    idx, dist = host.knn_host(x, 5)
    assert idx[0, 0].tolist() == [0, 1, 2, 3, 5] and dist[0, 0].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]
    assert idx[0, 4].tolist() == [4, 1, 3, 0, 2]


@pytest.mark.parametrize("N", sorted(set(host.KNN_N) | set(host.KNN_K)))
def test_knn_clouds_have_no_distance_ties(N):
    """Every cloud the GPU test searches: in each query's list the distances increase strictly down to the 21st place (or the N-th),
    so the k nearest and their order are unique for every k in use, and a kernel may be held to exact index equality."""
    x = host.knn_cloud(N)
    assert not torch.equal(x[0], x[1])                               # a batch-offset error would show
    idx, dist = host.knn_lists(N)
    assert idx.shape == (host.KNN_B, N, min(N, 21))
    assert bool((dist[..., 1:] > dist[..., :-1]).all())
    for k in host.KNN_K:
        if N in (k, 257):                                            # the list for k is a prefix of the deeper one (spot check)
            assert torch.equal(host.knn_host(x, k)[0], idx[..., :k])


@pytest.mark.parametrize("N", host.KNN_DUP_N)
def test_knn_duplicate_clouds_tie_only_across_quarters_and_stages(N):
    """With planted duplicates: every tie inside a list is between two copies of one point that lie in different quarters of the
    split kernel -- where its merge, not its unstable insertion, orders them -- and, from 2050 points on, in different 1024-stages
    of the single scan.  Ties occur, also across the k-th place for the k in use."""
    x = host.knn_dup_cloud(N)
    idx, dist = host.knn_lists(N, dup=True)
    quarter = (N + 3) // 4
    tied = dist[..., 1:] == dist[..., :-1]
    assert int(tied.sum()) >= 2 * 2 * host.KNN_DUP_COPIES * host.KNN_B
    assert not bool((tied[..., 1:] & tied[..., :-1]).any())          # pairs only
    i0, i1 = idx[..., :-1][tied], idx[..., 1:][tied]
    b = torch.arange(host.KNN_B).view(-1, 1, 1).expand_as(tied)[tied]
    assert bool((x[b, i0] == x[b, i1]).all()) and bool((i0 < i1).all())
    assert bool((i0 // quarter != i1 // quarter).all())
    if N >= 2050:
        assert bool((i0 // 1024 != i1 // 1024).all())
    for k in (16, 20):
        assert bool(tied[..., k - 1].any())                          # a tie between the k-th and the (k+1)-th place


# ---------------------------------------------------------------------------------------------------------------------
# edgeconv1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k", host.EDGECONV_CASES[:4])
def test_edgeconv_fp32_composition_holds_the_bound(B, N, k):
    xyz, idx, W, scale, shift = host.edgeconv_inputs(B, N, k)
    assert len({tuple(r) for r in W.tolist()}) == 64 and bool((W[:, :3] != W[:, 3:]).all())
    assert bool((scale > 0).any()) and bool((scale < 0).any()) and bool((shift > 0).any()) and bool((shift < 0).any())
    pre, ref, bound = host.edgeconv1_ref(xyz, idx, W, scale, shift)
    assert ref.shape == (B * N * k, 64)
    if N > 1:
        assert bool((pre > 0).any()) and bool((pre < 0).any())
        assert 0.1 < float((pre < 0).double().mean()) < 0.9          # ReLU clips a share of the outputs
    got = host.edgeconv1_f32(xyz, idx, W, scale, shift)
    assert got.dtype == torch.float32
    excess = ((got.double() - ref).abs() / bound).max()
    print(f"edgeconv1 fp32 composition B={B} N={N} k={k}: max error / bound = {float(excess):.3f}")
    assert float(excess) <= 1.0
    if N > 1:
        # the bound tells the two halves of the edge feature apart: centre first misses it at most outputs
        Wsw = torch.cat((W[:, 3:], W[:, :3]), dim=1)
        wrong = host.edgeconv1_f32(xyz, idx, Wsw, scale, shift)
        live = (ref > 0) | (wrong > 0)                               # not clipped to zero both ways
        assert float(((wrong.double() - ref).abs() > bound)[live].double().mean()) > 0.95


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 compositions whose error bounds layernorm, softmax_rows_ and softmax_corr
# ---------------------------------------------------------------------------------------------------------------------
def _report(title, table):
    print(f"\n{title}: largest error of the fp32 torch composition against float64, in ulp of the output magnitude")
    for key, (ulps, err, where) in table.items():
        print(f"  {key:<10} {ulps:8.2f} ulp   abs {err:.3e}   at {where}")


def test_layernorm_reference_and_composition_errors():
    x, a, b, r = host.layernorm_inputs(64, 5, "1")
    ref = host.layernorm_ref(x, a, b, r)
    want = a.double() * (x.double() - x.double().mean(-1, keepdim=True)) / (x.double().std(-1, keepdim=True) + host.LN_EPS) \
        + b.double() + r.double()
    np.testing.assert_allclose(ref.numpy(), want.numpy(), rtol=1e-13, atol=1e-13)
    biased = a.double() * (x.double() - x.double().mean(-1, keepdim=True)) / (x.double().std(-1, unbiased=False, keepdim=True)
                                                                                 + host.LN_EPS) + b.double() + r.double()
    assert float((ref - biased).abs().max()) > 1e-3                  # D against D - 1 is far outside any margin below
    table = {}
    for variant in host.LN_VARIANTS:
        worst = (-1.0, 0.0, "")
        for D in host.LN_D:
            for rows in host.LN_ROWS:
                x, a, b, r = host.layernorm_inputs(D, rows, variant)
                if variant == "offset":
                    assert abs(float(x[0].mean()) - 1000) < 2 and 0.2 < float(x[0].std()) < 3
                for res in (None, r):
                    ref = host.layernorm_ref(x, a, b, res)
                    err = host.max_err(host.layernorm_f32(x, a, b, res), ref)
                    mag = float(ref.abs().max())
                    assert np.isfinite(err) and err <= (1e-3 if variant == "offset" else 2e-5) * max(mag, 1.0)
                    worst = max(worst, (err / host.ulp32(mag), err, f"D={D} rows={rows} residual={res is not None}"))
        table[variant] = worst
    _report("layernorm", table)


def test_softmax_reference_and_composition_errors():
    x = host.softmax_inputs(77, 5, "special")
    assert bool(torch.isinf(x[0]).any()) and not bool(torch.isinf(x[0]).all()) and float(x[-1].max()) == 80.0
    ref = host.softmax_ref(x)
    np.testing.assert_allclose(ref.numpy(), torch.softmax(x.double(), -1).numpy(), rtol=1e-13, atol=1e-300)
    assert bool((ref[0][torch.isinf(x[0])] == 0).all()) and float(ref[-1, 77 // 2]) > 0.999999
    table = {}
    for variant in host.SM_VARIANTS:
        worst = (-1.0, 0.0, "")
        for L in host.SM_L:
            for rows in host.SM_ROWS:
                x = host.softmax_inputs(L, rows, variant)
                ref = host.softmax_ref(x)
                got = host.softmax_f32(x)
                err = host.max_err(got, ref)
                assert np.isfinite(err) and err <= 1e-6
                assert float((got.double().sum(-1) - 1).abs().max()) <= max(L, 8) * host.EPS32
                worst = max(worst, (err / host.ulp32(float(ref.max())), err, f"L={L} rows={rows}"))
        table[variant] = worst
    _report("softmax_rows", table)


def test_softmax_corr_reference_and_composition_errors():
    s, pts = host.softmax_corr_inputs(3, 50, 77, "plain")
    sp, pts2 = host.softmax_corr_inputs(3, 50, 77, "peaked")
    assert torch.equal(sp, s * 10) and torch.equal(pts, pts2)
    ref = host.softmax_corr_ref(s, pts)
    want = torch.einsum("pnm,pmc->pcn", torch.softmax(s.double(), -1), pts.double())
    np.testing.assert_allclose(ref.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
    mags = ref.abs().amax(dim=(0, 2))
    assert float(mags[1]) > 3 * float(mags[0]) and float(mags[2]) > 3 * float(mags[1])      # a swapped channel shows
    table = {}
    for variant in host.SC_VARIANTS:
        worst = (-1.0, 0.0, "")
        for P, N, M in host.SC_CASES:
            s, pts = host.softmax_corr_inputs(P, N, M, variant)
            ref = host.softmax_corr_ref(s, pts)
            err = host.per_coordinate_err(host.softmax_corr_f32(s, pts), ref)
            mag = ref.abs().amax(dim=(0, 2))
            for c in range(3):
                assert np.isfinite(float(err[c])) and float(err[c]) <= 2e-5 * max(float(mag[c]), host.SC_COORD_SCALE[c])
                worst = max(worst, (float(err[c]) / host.ulp32(float(mag[c])), float(err[c]), f"P={P} N={N} M={M} coordinate {c}"))
        table[variant] = worst
    _report("softmax_corr", table)


def test_margin_is_four_times_the_composition_plus_two_ulp():
    assert host.ulp32(1.0) == 2.0 ** -23 and host.ulp32(1000.0) == 2.0 ** -14 and host.ulp32(0.75) == 2.0 ** -24
    assert host.margin(1e-6, 1.0) == 4e-6 + 2.0 ** -22
    assert host.margin(0.0, 0.0) > 0
