"""GPU: houv_solve_iterate_large, the fused loop for clouds of 4097..16384 points (neither cloud resident in LDS): against the
CPU oracle, against the in-LDS kernel at sizes both serve, against the un-fused path it replaces, bitwise determinism and
chunking, memory on the product path, and solve_model / train_utils.solve end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_solve import _oracle_terms  # noqa: E402

T = torch.tensor


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _kw(mode):
    return dict(trans_mode=0 if mode == "houv" else 1, use_views=(mode == "houv"), f64_params=(mode != "houv"))


@pytest.mark.parametrize("N,M,base,mode", [(4500, 4500, 0, "houv"), (6000, 5000, 1, "solve"), (8192, 8192, 2, "solve"),
                                           (8192, 8192, 3, "houv")])
def test_large_single_forward_backward_vs_oracle(dev, N, M, base, mode):
    """The tolerances of test_gpu_solve.py::test_single_forward_backward_vs_oracle: the 8 Chamfer terms 1e-5, loss 5e-5,
    min_1 1e-5, R/T 1e-6, the gradient 2e-4 of its largest component with the same near-tie allowance.  P = 1-2: the
    oracle's float64 [P,N,M] temporaries are 0.5 GB each at 8192^2."""
    from houv_amd import ops, synthetic
    P = 2 if max(N, M) < 8192 else 1
    src, tgt, _ = synthetic.make_pairs(P, max(N, M), seed=78)
    src, tgt = src[:, :N].contiguous(), tgt[:, :M].contiguous()
    rng = np.random.default_rng(N + base)
    params = rng.standard_normal((P, 8)).astype(np.float32).astype(np.float64)
    want = _oracle_terms(src, tgt, params, base, mode)
    state = torch.zeros((P, 24), dtype=torch.float64, device=dev)
    state[:, :8] = T(params).to(dev)
    out = ops.solve_iterate(src.to(dev), tgt.to(dev), state, 1, steps_done=0, n_iters=1, angle_base=base, k_full=int(N * 0.5),
                            k_view=N, lr=0.01, loss_scale=1.0 / P, want_grad=True, want_cd=True, large=True, **_kw(mode))
    ncd = 8 if mode == "houv" else 2
    np.testing.assert_allclose(out["cd"].cpu().numpy()[:, :ncd], want["cd"][:, :ncd], rtol=0, atol=1e-5)
    np.testing.assert_allclose(out["loss"].cpu().numpy(), want["loss"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(out["score"].cpu().numpy(), want["min1"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(out["R"].cpu().numpy(), want["R"], atol=1e-6)
    np.testing.assert_allclose(out["T"].cpu().numpy(), want["T"], atol=1e-6)
    g = out["grad"].cpu().numpy()
    scale = np.abs(want["grads"]).max(axis=1, keepdims=True)
    err = (np.abs(g - want["grads"]) / scale).max(axis=1)
    assert (err > 2e-4).sum() <= 1, err
    assert err.max() < 3.0 / min(N, M), err


def _run(src, tgt, p0, K, n_iters, mode, large, iters_per_launch=None, lr=None, base=1):
    """n_iters iterations of every hypothesis through ops.solve_iterate (in-LDS brute-force kernel, or the large one), chunked
    like run_stage; returns (last forward's outputs, state)."""
    from houv_amd import ops
    P, N, _ = src.shape
    n = P * K
    state = torch.zeros((n, 24), dtype=torch.float64, device=src.device)
    state[:, :8] = T(p0).to(src.device)
    step = iters_per_launch or n_iters
    done, out = 0, None
    while done < n_iters:
        it = min(step, n_iters - done)
        out = ops.solve_iterate(src, tgt, state, K, steps_done=done, n_iters=it, angle_base=base, k_full=int(N * 0.5),
                                k_view=N, lr=lr or (0.01 if mode == "houv" else 0.1), loss_scale=1.0 / n,
                                want_grad=True, want_cd=True, large=large, **_kw(mode))
        done += it
    return out, state


def _assert_tracks(got, st_g, want, st_w, mode, N):
    """test_gpu_solve.py::test_large_cloud_path_matches_fused_kernel's tolerances (a few iterations, different sum orders).  The
    Adam first moments get, on top of its rtol 1e-2 / atol 1e-7, the gradient's near-tie allowance: 12/N of the row's largest
    moment.  A flip moves a small component's moment by that much (at 8192 points, measured: one of 208 moments off by 2.8e-7,
    1.4e-4 of its row's largest; the in-LDS kernel against the un-fused path at 4096 points: 5.4e-7, 1.1e-4)."""
    tol = 2e-5 if mode == "houv" else 2e-4
    for key in ("score", "loss", "R", "T", "cd"):
        assert torch.allclose(got[key], want[key], rtol=0, atol=tol * (5 if key == "loss" else 1)), key
    g_scale = want["grad"].abs().max(dim=1, keepdim=True)[0]
    err = ((got["grad"] - want["grad"]).abs() / g_scale).max(dim=1)[0]
    assert int((err > 2e-4).sum()) <= 4 and float(err.max()) < 12.0 / N, err
    assert torch.allclose(st_g[:, :8], st_w[:, :8], rtol=0, atol=20 * tol)
    m_tol = 1e-7 + 12.0 / N * st_w[:, 8:16].abs().max(dim=1, keepdim=True)[0]
    assert bool(((st_g[:, 8:16] - st_w[:, 8:16]).abs() <= 1e-2 * st_w[:, 8:16].abs() + m_tol).all())


@pytest.mark.parametrize("N,M,mode", [(64, 64, "houv"), (64, 64, "solve"), (1000, 1000, "houv"), (1000, 1000, "solve"),
                                      (2500, 2500, "houv"), (3000, 2200, "solve"), (4096, 4096, "houv"),
                                      (3500, 4096, "solve")])
def test_large_kernel_tracks_the_in_lds_kernel(dev, N, M, mode):
    """Where both serve (<= 4096 points), the new entry tracks the in-LDS brute-force kernel over 4 iterations, across the
    variant table (one wave ... 1024 threads x 4 points)."""
    from houv_amd import solver, synthetic
    P, K = 2, 26
    src, tgt, _ = synthetic.make_pairs(P, max(N, M), seed=5)
    src, tgt = src[:, :N].contiguous().to(dev), tgt[:, :M].contiguous().to(dev)
    p0 = solver.houv_init_params(P * K)
    want, st_w = _run(src, tgt, p0, K, 4, mode, large=False)
    got, st_g = _run(src, tgt, p0, K, 4, mode, large=True)
    _assert_tracks(got, st_g, want, st_w, mode, min(N, M))


@pytest.mark.parametrize("N,mode,iters", [(8192, "houv", 3), (8192, "solve", 3), (16384, "houv", 2), (16384, "solve", 2)])
def test_large_kernel_tracks_the_unfused_path(dev, monkeypatch, N, mode, iters):
    """run_stage on the new kernel against run_stage on the un-fused path it replaces (HOUV_LARGE=unfused)."""
    from houv_amd import solver, synthetic
    P, K = 1, 26
    src, tgt, _ = synthetic.make_pairs(P, N, seed=11)
    src, tgt = src.to(dev), tgt.to(dev)
    p0 = solver.houv_init_params(P * K)
    kw = dict(angle_base=2, lr=0.01 if mode == "houv" else 0.1, want_grad=True, want_cd=True, **_kw(mode))
    got, st_g = solver.run_stage(src, tgt, p0, K, iters, **kw)
    monkeypatch.setattr(solver, "LARGE_IMPL", "unfused")
    want, st_w = solver.run_stage(src, tgt, p0, K, iters, **kw)
    _assert_tracks(got, st_g, want, st_w, mode, N)


@pytest.mark.parametrize("mode", ["houv", "solve"])
def test_large_kernel_is_deterministic_and_chunking_neutral(dev, mode):
    """Same inputs, same bits; launches of 2 + 2 iterations (steps_done = 2 for the second) give the bits of one launch of 4."""
    from houv_amd import solver, synthetic
    P, K, N = 2, 26, 6000
    src, tgt, _ = synthetic.make_pairs(P, N, seed=12)
    src, tgt = src.to(dev), tgt.to(dev)
    p0 = solver.houv_init_params(P * K)
    runs = [_run(src, tgt, p0, K, 4, mode, True, chunk) for chunk in (4, 4, 2, 1)]
    for out, st in runs[1:]:
        for key in ("score", "loss", "R", "T", "grad", "cd"):
            assert torch.equal(out[key], runs[0][0][key]), key
        assert torch.equal(st, runs[0][1])


def test_run_stage_large_adds_no_per_hypothesis_clouds(dev):
    """P = 4 pairs x K = 64 on 8192-point clouds: run_stage allocates state and outputs only (< 16 MB over the clouds).  The
    un-fused path replicates both clouds K-fold (50 MB) before any autograd intermediate."""
    from houv_amd import solver, synthetic
    P, K, N = 4, 64, 8192
    src, tgt, _ = synthetic.make_pairs(P, N, seed=13)
    src, tgt = src.to(dev), tgt.to(dev)
    p0 = solver.houv_init_params(P * K)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    solver.LAUNCH_LOG = []
    try:
        out, state = solver.run_stage(src, tgt, p0, K, 2, angle_base=0, trans_mode=0, use_views=True, f64_params=False,
                                      lr=0.01, want_grad=True, want_cd=True)
        torch.cuda.synchronize()
        log = solver.LAUNCH_LOG
    finally:
        solver.LAUNCH_LOG = None
    extra = torch.cuda.max_memory_allocated(dev) - base
    assert extra < 16 * 2 ** 20, f"{extra / 2 ** 20:.1f} MB"
    assert log and all(e[4] == N and e[5] == N and not e[7] for e in log)          # logged launches of the large kernel
    assert bool(torch.isfinite(out["score"]).all()) and bool(torch.isfinite(state).all())


def test_solve_model_end_to_end_8192_points(dev, monkeypatch):
    """solve_model (best of K, retry stages) on 4 synthetic 8192-point pairs reaches the new kernel and does as well as the
    un-fused path on the same pairs: mean rotation error no worse than the un-fused path's + 2 degrees (the paths sum in
    different orders, so trajectories part after a few dozen iterations; a symmetric object may land another restart)."""
    from houv_amd import solver, synthetic
    from houv_amd.models.houv import HOUV, solve_model
    src, tgt, pose = synthetic.make_pairs(4, 8192, seed=2021)
    src, tgt, pose = src.to(dev), tgt.to(dev), pose.to(dev)
    kernel, epochs = 26, 60
    solver.LAUNCH_LOG = []
    try:
        r_new, t_new, ans = solve_model(HOUV(4 * kernel, 0), src, tgt, pose, kernel=kernel, num_epochs=epochs)
        torch.cuda.synchronize()
        log = solver.LAUNCH_LOG
    finally:
        solver.LAUNCH_LOG = None
    assert log and all(e[4] == 8192 for e in log)
    a = ans.cpu().numpy()
    assert a.shape == (4, 4, 4) and np.all(a[:, 3, :] == 0) and np.isfinite(a).all()
    assert bool(torch.isfinite(r_new).all()) and bool(torch.isfinite(t_new).all())
    monkeypatch.setattr(solver, "LARGE_IMPL", "unfused")
    r_unf, t_unf, _ = solve_model(HOUV(4 * kernel, 0), src, tgt, pose, kernel=kernel, num_epochs=epochs)
    assert float(r_new.mean()) <= float(r_unf.mean()) + 2.0, (r_new, r_unf)


def test_train_utils_solve_reaches_the_large_kernel(dev):
    """train_utils.solve (float64 leaves, no view terms, want_last_params) on 6000 x 5000-point pairs runs on the new kernel."""
    from houv_amd import solver, synthetic, train_utils
    src, tgt, pose = synthetic.make_pairs(2, 6000, seed=14)
    src, tgt, pose = src.to(dev), tgt[:, :5000].contiguous().to(dev), pose.to(dev)
    solver.LAUNCH_LOG = []
    try:
        r_err, t_err, ans = train_utils.solve(src, tgt, pose, kernel=26, _iters=5)
        torch.cuda.synchronize()
        log = solver.LAUNCH_LOG
    finally:
        solver.LAUNCH_LOG = None
    assert log and all((e[4], e[5], e[6]) == (6000, 5000, False) for e in log)
    assert bool(torch.isfinite(r_err).all()) and bool(torch.isfinite(ans).all())
