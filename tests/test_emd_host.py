"""CPU: the host restatement of the auction EMD (tests/emd_host.py) is an auction algorithm -- run to completion it returns a
bijection within N * eps of the optimal assignment -- and the Python surface mirrors the reference's metrics package."""
import inspect

import numpy as np
import pytest
import torch

import emd_host


@pytest.mark.parametrize("N,eps,seed", [(16, 0.005, 0), (33, 0.01, 1), (64, 0.005, 2), (100, 0.02, 3), (128, 0.005, 4)])
def test_auction_to_completion_is_near_optimal_bijection(N, eps, seed):
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(seed)
    x1 = rng.random((N, 3), dtype=np.float32)
    x2 = rng.random((N, 3), dtype=np.float32)
    dist, assign, run = emd_host.emd_cloud(x1, x2, eps, 10 ** 7)
    assert run < 10 ** 7                                         # finished by itself, not by the forced last step
    assert sorted(assign.tolist()) == list(range(N))             # a bijection
    cost = np.linalg.norm(x1.astype(np.float64)[:, None, :] - x2.astype(np.float64)[None, :, :], axis=2)
    r, c = opt.linear_sum_assignment(cost)
    best = cost[r, c].sum()
    total = cost[np.arange(N), assign].sum()
    # epsilon-complementary slackness: total benefit within N * eps of the optimum.  fp32 slack: the benefits 3 - |d| and the
    # prices (sums of increments, a few units at most) carry relative rounding ~6e-8 each; 1e-5 per point bounds it widely.
    assert best - 1e-9 <= total <= best + N * eps + N * 1e-5
    np.testing.assert_allclose(np.sqrt(dist.astype(np.float64)), cost[np.arange(N), assign], rtol=1e-5, atol=1e-6)


def test_forced_last_step_and_early_exit():
    rng = np.random.default_rng(7)
    x1 = rng.random((50, 3), dtype=np.float32)
    x2 = x1[::-1].copy()
    _, assign, run = emd_host.emd_cloud(x1, x2, 0.01, 1)         # one iteration: every bidder takes its best object
    assert run == 1 and (assign == np.arange(50)[::-1]).all()
    _, a1, r1 = emd_host.emd_cloud(x1, x2, 0.01, 10 ** 6)
    _, a2, r2 = emd_host.emd_cloud(x1, x2, 0.01, r1 + 5)
    assert r1 == r2 and (a1 == a2).all()


def test_single_point():
    dist, assign, run = emd_host.emd_cloud(np.array([[0.1, 0.2, 0.3]]), np.array([[0.5, 0.2, 0.3]]), 0.005, 10)
    assert run == 1 and assign.tolist() == [0]
    assert dist[0] == np.float32(np.float32(0.1) - np.float32(0.5)) ** 2


def test_metrics_import_names_after_install():
    from houv_amd import compat
    compat.uninstall()
    compat.install()
    try:
        from metrics import cd, emd, fscore                      # registration/model_utils_completion.py:18
        from houv_amd import metrics
        assert cd is metrics.cd and emd is metrics.emd and fscore is metrics.fscore
        from model_utils_completion import calc_emd              # noqa: F401
    finally:
        compat.uninstall()


def test_fscore_formula():
    from houv_amd.metrics import fscore
    d1 = torch.tensor([[0.0, 1e-5, 1.0, 2.0], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    d2 = torch.tensor([[1e-5, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [1.0, 0.0, 0.0, 0.0]])
    f, p1, p2 = fscore(d1, d2)
    assert p1.tolist() == [0.5, 0.0, 1.0] and p2.tolist() == [0.25, 0.0, 0.75]
    expect = 2 * p1 * p2 / (p1 + p2)
    assert f[0] == expect[0] and f[2] == expect[2]
    assert f[1] == 0.0                                           # both precisions 0: NaN set to 0
    f, p1, p2 = fscore(d1, d2, threshold=1.5)
    assert p1.tolist() == [0.75, 1.0, 1.0]


def test_calc_emd_signature_matches_reference():
    from houv_amd.model_utils_completion import calc_emd
    sig = inspect.signature(calc_emd)
    assert list(sig.parameters) == ["output", "gt", "eps", "iterations"]
    assert sig.parameters["eps"].default == 0.005 and sig.parameters["iterations"].default == 50


def test_emd_module_interface():
    from houv_amd.metrics import emd, emdFunction, emdModule
    assert emd is emdModule
    assert list(inspect.signature(emdModule.forward).parameters) == ["self", "input1", "input2", "eps", "iters"]
    assert list(inspect.signature(emdFunction.forward).parameters) == ["ctx", "xyz1", "xyz2", "eps", "iters"]


# ---------------------------------------------------------------------------------------------------
# Coverage guard of the GPU parity tables (tests/emd_cases.py, run on the GPU by tests/test_gpu_emd.py): shown with the
# restatement alone, so a table that stops reaching a bid branch fails here, without a GPU.
# ---------------------------------------------------------------------------------------------------
import emd_cases  # noqa: E402


def _shapes(clouds_of, cases):
    got = set()
    for case in cases:
        x1, x2 = clouds_of(case)
        trace = []
        emd_host.emd(x1.numpy(), x2.numpy(), case[2], case[1], trace=trace)
        got |= {emd_cases.bid_shape(u) for cloud in trace for u in cloud}
    return got


def test_bid_shape_mirrors_the_branch_table():
    table = [(16384, (4, 1, 4)), (12289, (4, 1, 4)), (12288, (4, 1, 3)), (8193, (4, 1, 3)), (8192, (4, 1, 2)), (4097, (4, 1, 2)),
             (4096, (4, 1, 1)), (2049, (4, 1, 1)), (2048, (4, 2, 1)), (1025, (4, 2, 1)), (1024, (1, 1, 1)), (513, (1, 1, 1)),
             (512, (1, 2, 1)), (257, (1, 2, 1)), (256, (1, 4, 1)), (129, (1, 4, 1)), (128, (1, 8, 1)), (65, (1, 8, 1)),
             (64, (1, 16, 1)), (33, (1, 16, 1)), (32, (1, 32, 1)), (17, (1, 32, 1)), (16, (1, 64, 1)), (1, (1, 64, 1))]
    for cnt, want in table:
        assert emd_cases.bid_shape(cnt) == want, cnt
    assert {emd_cases.bid_shape(c) for c in range(1, 4097)} == emd_cases.REACHABLE_LDS
    assert {emd_cases.bid_shape(c) for c in range(1, 16385)} == emd_cases.REACHABLE_STREAM
    assert len(emd_cases.REACHABLE_LDS) == 9 and len(emd_cases.REACHABLE_STREAM) == 12


def test_in_lds_cases_reach_every_bid_branch():
    assert all(c[0] <= 4096 for c in emd_cases.LDS_CASES)
    assert _shapes(emd_cases.lds_clouds, emd_cases.LDS_CASES) == emd_cases.REACHABLE_LDS


def test_streamed_cases_reach_every_bid_branch():
    assert all(4096 < c[0] <= 16384 for c in emd_cases.STREAM_CASES)
    old = _shapes(emd_cases.stream_clouds, emd_cases.STREAM_CASES_OLD)
    assert old == {(4, 1, 2), (4, 1, 1), (4, 2, 1)}              # the gap: no P = 1 branch, never more than two passes
    assert old | _shapes(emd_cases.stream_clouds, emd_cases.STREAM_CASES_NEW) == emd_cases.REACHABLE_STREAM


@pytest.mark.parametrize("case,passes", [(emd_cases.STREAM_LASTOBJ3, 3), (emd_cases.STREAM_LASTOBJ4, 4)])
def test_lastobj_cases_crowd_the_last_object(case, passes):
    N, iters, eps, B, kind = case
    assert kind == "lastobj" and N % 4096 == 1                   # the last object tile and the last bid pass hold one entry
    x1, x2 = emd_cases.stream_clouds(case)
    x1, x2 = x1[0].numpy(), x2[0].numpy()
    js, _ = emd_host._bid(x1, x2, np.zeros(N, dtype=np.float32), np.arange(N), eps)
    assert (js == N - 1).sum() >= N / 4                          # bids at t = 0
    assert emd_cases.bid_shape(N) == (4, 1, passes)


def test_run_to_completion_case():
    N, iters, eps, B, kind = emd_cases.STREAM_COMPLETE
    x1, x2 = emd_cases.stream_clouds(emd_cases.STREAM_COMPLETE)
    trace = []
    _, assign, run = emd_host.emd_cloud(x1[0].numpy(), x2[0].numpy(), eps, iters, trace=trace)
    assert run < iters and len(trace) == run
    assert sorted(assign.tolist()) == list(range(N))
    assert {emd_cases.bid_shape(u)[1] for u in trace if u <= 1024} == {1, 2, 4, 8, 16, 32, 64}


def test_dupbid_case_has_equal_increment_ties():
    N, iters, eps, B, kind = emd_cases.STREAM_DUPBID
    x1, x2 = emd_cases.stream_clouds(emd_cases.STREAM_DUPBID)
    js, incs = emd_host._bid(x1[0].numpy(), x2[0].numpy(), np.zeros(N, dtype=np.float32), np.arange(N), eps)
    assert (js[1::2] == js[0:N - 1:2]).all()
    assert np.array_equal(incs[1::2].view(np.uint32), incs[0:N - 1:2].view(np.uint32))   # the award must take the lowest i


def test_ties_case_has_equal_values_down_the_tail():
    N, iters, eps, B, kind = emd_cases.STREAM_TIES
    x1, x2 = emd_cases.stream_clouds(emd_cases.STREAM_TIES)
    x1, x2 = x1[0].numpy(), x2[0].numpy()
    assert N % 2 == 0 and np.array_equal(x2[1::2], x2[0::2])     # every object has a twin
    js, incs = emd_host._bid(x1, x2, np.zeros(N, dtype=np.float32), np.arange(N), eps)
    assert (js % 2 == 0).all() and (incs == np.float32(eps)).all()   # best == second: the lower twin, increment eps alone
    trace = []
    _, assign, run = emd_host.emd_cloud(x1, x2, eps, iters, trace=trace)
    assert run < iters and sorted(assign.tolist()) == list(range(N))
    assert {emd_cases.bid_shape(u)[1] for u in trace if u <= 1024} == {1, 2, 4, 8, 16, 32, 64}


def test_mixed_batch_has_three_different_iteration_counts():
    x1, x2 = emd_cases.batch_clouds()
    _, assign, run = emd_host.emd(x1.numpy(), x2.numpy(), emd_cases.BATCH_EPS, emd_cases.BATCH_ITERS)
    assert run[0] == 1 and 1 < run[1] < emd_cases.BATCH_ITERS and run[2] == emd_cases.BATCH_ITERS
    assert (assign[0] == np.arange(emd_cases.BATCH_N)).all()
    assert emd_cases.BATCH_N % 4 != 0


def test_backward_restatement_against_float64():
    rng = np.random.default_rng(5)
    B, N = 3, 257
    x1 = rng.random((B, N, 3), dtype=np.float32)
    x2 = rng.random((B, N, 3), dtype=np.float32)
    g = rng.standard_normal((B, N)).astype(np.float32)
    a = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32)
    a[1, :] = a[1, 0]                                            # many-to-one
    out = emd_host.emd_backward(x1, x2, g, a)
    assert out.dtype == np.float32
    y = np.take_along_axis(x2.astype(np.float64), a[:, :, None].astype(np.int64), axis=1)
    term = (2.0 * g.astype(np.float64))[:, :, None] * (x1.astype(np.float64) - y)
    ulp = np.spacing(np.float32(np.abs(term).max()))
    assert np.abs(out - term).max() <= 4 * ulp
    # accumulation: into a caller's buffer, in place, one fp32 addition per element
    into = rng.standard_normal((B, N, 3)).astype(np.float32)
    before = into.copy()
    again = emd_host.emd_backward(x1, x2, g, a, into=into)
    assert again is into and np.array_equal(into, before + out)
