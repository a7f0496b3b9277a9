"""CPU checks of houv_amd/csrc/houv_math.h (the per-instance math the HIP kernels inline) against the oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import houv_ref_cpu as orc
from tests import hostmath

F = ctypes.POINTER(ctypes.c_float)
D = ctypes.POINTER(ctypes.c_double)


def fp(a):
    return a.ctypes.data_as(F)


def dp(a):
    return a.ctypes.data_as(D)


@pytest.fixture(scope="module")
def hm():
    return hostmath.load()


def pack(V, a, tc, ts):
    return np.ascontiguousarray(np.concatenate([V, a, tc, ts], axis=1), dtype=np.float32)


@pytest.mark.parametrize("mode", ["houv", "solve"])
@pytest.mark.parametrize("base", [0, 1, 2, 3])
def test_pose_forward_and_backward(hm, base, mode):
    n = 64
    V, a, tc, ts = orc.houv_init_params(n, seed=5)
    P = pack(V, a, tc, ts)
    R = np.zeros((n, 9), np.float32)
    T = np.zeros((n, 3), np.float32)
    tm = 0 if mode == "houv" else 1
    hm.hm_pose_forward(fp(P), n, base, tm, fp(R), fp(T))
    tv = [torch.tensor(x, requires_grad=True) for x in (V, a, tc, ts)]
    src = torch.tensor(np.random.default_rng(0).standard_normal((n, 17, 3)).astype(np.float32))
    moved, Rr, Tr = orc.houv_forward(src, *tv, base, mode)
    np.testing.assert_allclose(R.reshape(n, 3, 3), Rr.detach().numpy(), atol=3e-7)
    np.testing.assert_allclose(T, Tr.detach().numpy()[:, 0], atol=1e-7)
    # backward: random upstream gradient G on the moved cloud
    G = torch.tensor(np.random.default_rng(1).standard_normal((n, 17, 3)).astype(np.float32))
    (moved * G).sum().backward()
    gT = G.sum(1).numpy().astype(np.float32)
    M = torch.einsum("bni,bnj->bij", G, src).numpy().astype(np.float32).reshape(n, 9)
    g = np.zeros((n, 8), np.float32)
    hm.hm_pose_backward(fp(P), n, base, tm, fp(np.ascontiguousarray(gT)), fp(np.ascontiguousarray(M)), fp(g))
    ref = np.concatenate([t.grad.numpy() for t in tv], axis=1)
    scale = np.abs(ref).max(axis=0, keepdims=True) + 1e-6
    np.testing.assert_allclose(g / scale, ref / scale, atol=2e-5)


def test_adam_matches_torch_f32_and_f64(hm):
    rng = np.random.default_rng(3)
    for dt, fn, cp in ((np.float32, "hm_adam_f32", fp), (np.float64, "hm_adam_f64", dp)):
        n = 50
        p0 = rng.standard_normal(n).astype(dt)
        p = p0.copy(); m = np.zeros(n, dt); v = np.zeros(n, dt)
        tp = torch.tensor(p0.copy(), requires_grad=True)
        opt = torch.optim.Adam([tp], lr=0.01)
        for step in range(1, 30):
            g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n)).astype(dt)
            getattr(hm, fn)(cp(p), cp(m), cp(v), cp(g), n, step, ctypes.c_double(0.01), ctypes.c_double(0.9),
                            ctypes.c_double(0.999), ctypes.c_double(1e-8))
            tp.grad = torch.tensor(g.copy())
            opt.step()
            tol = 2e-7 if dt == np.float32 else 1e-15
            np.testing.assert_allclose(p, tp.detach().numpy(), rtol=tol, atol=tol)


@pytest.mark.parametrize("B,N,M,k", [(2, 1, 1, 1), (2, 57, 300, 32), (1, 40, 1025, 17), (1, 9, 33, 33)])
def test_knn_cross_host_function_equals_float64_sort(hm, B, N, M, k):
    """hm_knn_cross_fmaf on a tie-free cloud: the same lists, in the same order, as a stable float64 sort of the exact squared
    distances of the same fp32 differences; the distances within three roundings of them."""
    import pointops_host as host
    q, r = host.knn_inputs("random", B, N, M)
    idx, dist = host.knn_cross(q, r, k)
    d = r[:, None, :, :] - q[:, :, None, :]
    assert d.dtype == np.float32
    exact = (d.astype(np.float64) ** 2).sum(-1)
    order = np.argsort(exact, axis=-1, kind="stable")[..., :k]
    srt = np.take_along_axis(exact, order, -1)
    if M > 1:
        assert (np.diff(np.sort(exact, -1), axis=-1)[..., :k] > 8 * 2.0 ** -24 * np.sort(exact, -1)[..., 1:k + 1]).all()  # tie-free
    assert np.array_equal(idx, order)
    assert (np.abs(dist.astype(np.float64) - srt) <= 3 * 2.0 ** -24 * srt).all()


def test_knn_cross_host_function_orders_ties_by_index(hm):
    import pointops_host as host
    q, r = host.knn_inputs("identical", 2, 11, 40)
    idx, dist = host.knn_cross(q, r, 32)
    assert (idx == np.arange(32)).all() and (dist == dist[..., :1]).all()
    q, r = host.knn_inputs("repeat", 1, 13, 64)
    idx, dist = host.knn_cross(q, r, 32)
    assert (dist[..., 0::2] == dist[..., 1::2]).all() and (idx[..., 1::2] == idx[..., 0::2] + 32).all()
    q, r = host.knn_inputs("copies", 2, 20, 50)
    idx, dist = host.knn_cross(q, r, 3)
    assert (dist[..., 0] == 0).all() and (np.take_along_axis(r, idx[..., :1].astype(np.int64), 1) == q).all()
    # "descending": nearly every reference enters the 8-list of the references before it (the queued kernels' enqueue test)
    q, r = host.knn_inputs("descending", 1, 5, 500)
    d = ((r[:, None].astype(np.float64) - q[:, :, None]) ** 2).sum(-1)[0]
    assert (np.linalg.norm(q, axis=-1) <= 0.05 + 1e-6).all()
    enters = [d[n, j] < np.sort(d[n, :j])[7] for n in range(5) for j in range(8, 500)]
    assert np.mean(enters) > 0.9
    # a prefix of the 32-list is the shorter list
    for k in (1, 5, 17):
        a = host.knn_expected("lattice", 2, 7, 100, k)
        b = host.knn_cross(*host.knn_inputs("lattice", 2, 7, 100), k)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == np.ascontiguousarray(b[1]).tobytes()


def test_svd_and_kabsch(hm, golden):
    rng = np.random.default_rng(9)
    n = 200
    H = rng.standard_normal((n, 3, 3)).astype(np.float32)
    H[:20] *= np.array([1, 1e-3, 1e-6], np.float32)      # ill conditioned
    H[20:30, :, 2] = H[20:30, :, 0]                      # rank deficient
    H[30] = 0
    Hc = np.ascontiguousarray(H.reshape(n, 9))
    U = np.zeros((n, 9), np.float32); S = np.zeros((n, 3), np.float32); V = np.zeros((n, 9), np.float32)
    hm.hm_svd3x3_f32(fp(Hc), n, fp(U), fp(S), fp(V))
    U = U.reshape(n, 3, 3); V = V.reshape(n, 3, 3)
    rec = U @ (S[:, :, None] * V.transpose(0, 2, 1))
    np.testing.assert_allclose(rec, H, atol=2e-6 * max(1.0, np.abs(H).max()))
    np.testing.assert_allclose(S, np.linalg.svd(H.astype(np.float64), compute_uv=False), atol=3e-6)
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3))
    np.testing.assert_allclose(V.transpose(0, 2, 1) @ V, eye, atol=2e-6)
    np.testing.assert_allclose(U.transpose(0, 2, 1) @ U, eye, atol=2e-5)
    # Kabsch rotation against the reference's SVDHead outputs (G7): build H the way model_utils.py:221-227 does
    g = golden("g7_svdhead.npz")
    src, corr = g["src"], g["corr"]
    Hk = (src - src.mean(2, keepdims=True)) @ (corr - corr.mean(2, keepdims=True)).transpose(0, 2, 1)
    Hk = np.ascontiguousarray(Hk.reshape(-1, 9).astype(np.float32))
    R = np.zeros((len(Hk), 9), np.float32)
    hm.hm_kabsch_rotation_f32(fp(Hk), len(Hk), fp(R))
    np.testing.assert_allclose(R.reshape(-1, 3, 3), g["R"], atol=2e-5)


# ---- solve_tail: the scalar tail both fused solve kernels run per hypothesis and iteration ---------------------------------
ACC_STRIDE = 16          # kAccStride: acc[8][16] floats per hypothesis, slot = metric*2 + dir, entries S, G[3], GP[9]
TAIL_N, TAIL_KFULL, TAIL_KVIEW = 16, 8, 16
ADAM = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8)


def run_tail(hm, nmet, acc, state, loss_scale, trans_mode=0, base=0, f64=0, step=1, k_full=TAIL_KFULL, k_view=TAIL_KVIEW):
    """-> dict(score, loss, cd[n,4,2], g[n,8], R[n,3,3], T[n,3]); `state` [n,24] float64 is stepped in place."""
    n = len(state)
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    assert acc.shape == (n, 8, ACC_STRIDE) and state.dtype == np.float64 and state.flags.c_contiguous
    sl, cd, g = np.zeros((n, 2), np.float32), np.full((n, 8), -1, np.float32), np.zeros((n, 8), np.float32)
    R, T = np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32)
    ok = hm.hm_solve_tail(nmet, n, fp(acc), dp(state), k_full, k_view, ctypes.c_float(loss_scale), trans_mode, base, f64, step,
                          ctypes.c_double(ADAM["lr"]), ctypes.c_double(ADAM["b1"]), ctypes.c_double(ADAM["b2"]),
                          ctypes.c_double(ADAM["eps"]), fp(sl), fp(cd), fp(g), fp(R), fp(T))
    assert ok == 1
    return dict(score=sl[:, 0], loss=sl[:, 1], cd=cd.reshape(n, 4, 2), g=g, R=R.reshape(n, 3, 3), T=T)


def tail_sums(moved, src, tgt, nmet):
    """acc[8,16] of one hypothesis from brute-force nearest neighbours, in float64: per metric (0 full, 1..3 one coordinate
    dropped) and direction (0 over the target points, 1 over the moved points) S = sum sqrt(d) over the k smallest d,
    G = sum c, GP = sum c p^T with c = d(sqrt d)/d(moved point) and p the un-moved source point."""
    acc = np.zeros((8, ACC_STRIDE))
    for m in range(nmet):
        keep = np.ones(3)
        if m:
            keep[m - 1] = 0.0
        diff = (moved[:, None, :].astype(np.float64) - tgt[None, :, :]) * keep          # [N, M, 3]: moved_i - target_j
        d = (diff ** 2).sum(-1)
        for direction in (0, 1):
            if direction == 1:
                nn = d.argmin(1)
                dist, c, p = d.min(1), diff[np.arange(len(moved)), nn], src
            else:
                nn = d.argmin(0)
                dist, c, p = d.min(0), diff[nn, np.arange(len(tgt))], src[nn]
            sel = np.argsort(dist, kind="stable")[:TAIL_KFULL if m == 0 else TAIL_KVIEW]
            c = c[sel] / np.sqrt(dist[sel])[:, None]
            row = acc[m * 2 + direction]
            row[0], row[1:4], row[4:13] = np.sqrt(dist[sel]).sum(), c.sum(0), (c[:, :, None] * p[sel][:, None, :]).sum(0).ravel()
    return acc


@pytest.mark.parametrize("mode", ["houv", "solve"])
@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("nmet", [1, 4])
def test_solve_tail_matches_one_oracle_step(hm, nmet, f64, mode):
    """One iteration of the oracle's loop (forward, loss, mean, backward, Adam) on 26 hypotheses over one 16-point pair against
    solve_tail fed with the 8 x 13 sums of the same moved cloud.  Score, loss, cd and gradient: the tolerance of the
    pose_backward test; stepped parameters and their pose: those of the Adam and pose_forward tests.  Adam is compared the way
    the Adam test does it, on the SAME gradient (the tail's, handed to torch): at step 1 the update is lr g / (|g| + eps), so
    the rounding noise the gradient tolerance allows would otherwise be divided by |g|."""
    from houv_amd import synthetic
    n, base, tm = 26, 1, (0 if mode == "houv" else 1)
    src, tgt, _ = synthetic.make_pairs(1, TAIL_N, seed=7)
    s, t = src.expand(n, -1, -1).contiguous(), tgt.expand(n, -1, -1).contiguous()
    dt = torch.float64 if f64 else torch.float32
    leaves = [torch.tensor(x, dtype=dt, requires_grad=True) for x in orc.houv_init_params(n, seed=11)]
    opt = torch.optim.Adam(leaves, lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"])
    moved, _, _ = orc.houv_forward(s, *[x.float() for x in leaves], base, mode)
    cds = [orc.calc_cd_percent(moved, t, percent=0.5)] + [orc.loss_view(moved, t, dim=d) for d in range(3)]
    mins = [torch.minimum(c0, c1) for c0, c1 in cds[:nmet]]
    loss = mins[0] * 6 if nmet == 1 else mins[0] * 6 + (mins[1] + mins[2] + mins[3])
    loss.mean().backward()

    acc = np.stack([tail_sums(moved[i].detach().numpy(), src[0].numpy(), tgt[0].numpy(), nmet) for i in range(n)])
    state = np.zeros((n, 24))
    state[:, :8] = np.concatenate([x.detach().numpy() for x in leaves], axis=1)
    out = run_tail(hm, nmet, acc, state, 1.0 / n, tm, base, f64)

    def close(got, ref):
        scale = np.abs(ref).max(axis=0, keepdims=True) + 1e-6
        np.testing.assert_allclose(got / scale, ref / scale, atol=2e-5)
    close(out["score"], mins[0].detach().numpy())
    close(out["loss"], loss.detach().numpy())
    ref_cd = np.zeros((n, 4, 2), np.float32)
    for m in range(nmet):
        ref_cd[:, m, 0], ref_cd[:, m, 1] = cds[m][0].detach().numpy(), cds[m][1].detach().numpy()
    close(out["cd"].reshape(n, 8), ref_cd.reshape(n, 8))
    assert (out["cd"][:, nmet:] == 0).all()
    close(out["g"], np.concatenate([x.grad.numpy() for x in leaves], axis=1).astype(np.float32))

    for x, cols in zip(leaves, ((0, 3), (3, 4), (4, 7), (7, 8))):
        x.grad = torch.tensor(out["g"][:, cols[0]:cols[1]], dtype=dt)
    opt.step()
    tol = 1e-15 if f64 else 2e-7
    np.testing.assert_allclose(state[:, :8], np.concatenate([x.detach().numpy() for x in leaves], axis=1), rtol=tol, atol=tol)
    if not f64:
        assert np.array_equal(state, state.astype(np.float32).astype(np.float64))
    _, Rr, Tr = orc.houv_forward(s, *[x.detach().float() for x in leaves], base, mode)
    np.testing.assert_allclose(out["R"], Rr.numpy(), atol=3e-7)
    np.testing.assert_allclose(out["T"], Tr.numpy()[:, 0], atol=1e-7)


def _hand_made(n=1, seed=0):
    """Finite, generic sums and a generic state: every slot differs from every other."""
    rng = np.random.default_rng(seed)
    acc = rng.uniform(0.5, 2.0, (n, 8, ACC_STRIDE)).astype(np.float32)
    acc[:, :, 1:] -= 1.25
    state = np.zeros((n, 24))
    state[:, :8] = rng.standard_normal((n, 8))
    state[:, 8:16] = rng.standard_normal((n, 8)) * 1e-3
    state[:, 16:] = rng.uniform(1e-7, 1e-5, (n, 8))
    return acc, state


@pytest.mark.parametrize("nmet", [1, 4])
def test_solve_tail_first_direction_wins_ties(hm, nmet):
    for m in range(nmet):
        acc, state = _hand_made()
        acc[0, m * 2 + 1, 0] = acc[0, m * 2 + 0, 0]
        ref = run_tail(hm, nmet, acc, state.copy(), 0.5, step=3)
        assert ref["cd"][0, m, 0] == ref["cd"][0, m, 1]
        other, st_other = acc.copy(), state.copy()
        other[0, m * 2 + 1, 1:13] += 1.0                       # the losing direction's G / GP are not read
        got = run_tail(hm, nmet, other, st_other, 0.5, step=3)
        assert got["g"].tobytes() == ref["g"].tobytes()
        winner = acc.copy()
        winner[0, m * 2 + 0, 1:13] += 1.0                      # the winning direction's are
        assert not np.array_equal(run_tail(hm, nmet, winner, state.copy(), 0.5, step=3)["g"], ref["g"])


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("nmet", [1, 4])
def test_solve_tail_nan_in_any_direction_poisons_the_step(hm, nmet, f64):
    for m in range(nmet):
        for direction in (0, 1):
            acc, state = _hand_made()
            acc[0, m * 2 + direction, 0] = np.nan
            out = run_tail(hm, nmet, acc, state, 0.5, f64=f64, step=2)
            assert np.isnan(out["score"][0]) == (m == 0)       # the score is metric 0's alone
            assert np.isnan(out["loss"][0]) and np.isnan(out["g"]).all()
            assert np.isnan(state).all()                       # parameters, m and v are stepped with NaN
            assert np.isnan(out["cd"][0, m, direction]) and np.isfinite(np.delete(out["cd"].ravel(), m * 2 + direction)).all()


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("nmet", [1, 4])
def test_solve_tail_later_step_matches_torch_adam(hm, nmet, f64):
    """Step 5 with non-zero first and second moments (the bias corrections are not 1 - beta): parameters, m and v against
    torch.optim.Adam resumed from the same state and given the tail's gradient; the Adam test's tolerances."""
    n, step = 6, 5
    acc, state = _hand_made(n=n, seed=9)
    dt, npdt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
    state[:] = state.astype(npdt)
    leaf = torch.tensor(state[:, :8], dtype=dt, requires_grad=True)
    opt = torch.optim.Adam([leaf], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"])
    opt.state[leaf] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.tensor(state[:, 8:16], dtype=dt),
                           exp_avg_sq=torch.tensor(state[:, 16:], dtype=dt))
    out = run_tail(hm, nmet, acc, state, 0.5, f64=f64, step=step)
    leaf.grad = torch.tensor(out["g"], dtype=dt)
    opt.step()
    tol = 1e-15 if f64 else 2e-7
    for got, ref in ((state[:, :8], leaf.detach()), (state[:, 8:16], opt.state[leaf]["exp_avg"]),
                     (state[:, 16:], opt.state[leaf]["exp_avg_sq"])):
        np.testing.assert_allclose(got, ref.numpy(), rtol=tol, atol=tol)


def test_solve_tail_single_metric_pads_cd_with_zeros_and_ignores_view_slots(hm):
    acc, state = _hand_made()
    ref = run_tail(hm, 1, acc, state.copy(), 0.5)
    assert (ref["cd"][0, 1:] == 0).all() and (ref["cd"][0, 0] > 0).all()
    assert ref["loss"][0] == np.float32(ref["score"][0] * np.float32(6))
    junk = acc.copy()
    junk[0, 2:] = np.nan
    st = state.copy()
    got = run_tail(hm, 1, junk, st, 0.5)
    assert all(got[k].tobytes() == ref[k].tobytes() for k in ref) and np.isfinite(st).all()


@pytest.mark.parametrize("nmet", [1, 4])
def test_solve_tail_state_holds_float_rounded_values_without_f64_params(hm, nmet):
    acc, state = _hand_made(n=5, seed=4)
    s32, s64 = state.copy(), state.copy()
    run_tail(hm, nmet, acc, s32, 0.5, f64=0, step=7)
    run_tail(hm, nmet, acc, s64, 0.5, f64=1, step=7)
    assert np.array_equal(s32, s32.astype(np.float32).astype(np.float64))
    assert not np.array_equal(s64, s64.astype(np.float32).astype(np.float64))
