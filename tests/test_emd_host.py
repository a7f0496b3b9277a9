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
