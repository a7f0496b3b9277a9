"""GPU: houv_icp_refine against oracle/icp_ref.py (numpy restatement of Open3D's published point-to-point ICP).
PARITY UNPINNED w.r.t. Open3D itself (not installed, no fixtures in the reference) -- see oracle/icp_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import icp_ref  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _perturb(T, rng, ang_deg, tr):
    ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
    a = np.deg2rad(ang_deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    P = np.eye(4); P[:3, :3] = R; P[:3, 3] = rng.standard_normal(3) * tr
    return (P @ T).astype(np.float32)


@pytest.mark.parametrize("N", [200, 700, 2048])
def test_icp_matches_oracle(dev, N):
    from houv_amd import ops, synthetic
    P = 6
    src, tgt, pose = synthetic.make_pairs(P, N, seed=31)
    rng = np.random.default_rng(N)
    init = np.stack([_perturb(pose[i].numpy(), rng, 4.0, 0.01) for i in range(P)])
    out = ops.icp_refine(src.to(dev), tgt.to(dev), torch.tensor(init).to(dev), 0.04, 60)
    for i in range(P):
        T, fit, rmse, it = icp_ref.icp_point_to_point(src[i].numpy(), tgt[i].numpy(), init[i], 0.04, 60)
        Tg = out["T"][i].cpu().numpy()
        assert np.array_equal(Tg[3], [0, 0, 0, 1])
        # fp32 kernel vs float64 oracle: same fixed point, same correspondences up to threshold near-ties
        np.testing.assert_allclose(Tg, T, atol=2e-3)
        assert abs(float(out["fitness"][i]) - fit) <= 3.0 / N
        assert abs(float(out["inlier_rmse"][i]) - rmse) <= 2e-4
        assert abs(int(out["iterations"][i]) - it) <= max(3, it // 4)


def test_icp_zero_iterations_and_identity(dev):
    from houv_amd import ops, synthetic
    src, tgt, pose = synthetic.make_pairs(3, 300, seed=5)
    out = ops.icp_refine(src.to(dev), tgt.to(dev), pose.to(dev), 0.02, 0)
    np.testing.assert_allclose(out["T"].cpu().numpy(), pose.numpy(), atol=1e-6)       # no update applied
    assert (out["iterations"].cpu() == 0).all()
    # identical clouds, identity init: already converged
    out = ops.icp_refine(src.to(dev), src.to(dev), None, 0.02, 50)
    np.testing.assert_allclose(out["T"].cpu().numpy(), np.broadcast_to(np.eye(4, dtype=np.float32), (3, 4, 4)), atol=1e-6)
    assert float(out["fitness"].min()) == 1.0 and float(out["inlier_rmse"].max()) < 1e-6


def test_houv_plus_icp_improves_or_keeps_alignment(dev):
    """cfg4 shape: HOUV answer -> ICP refine.  On pairs HOUV already solves, ICP must not make them worse."""
    from houv_amd import synthetic
    from houv_amd.icp import solve_model_icp
    from houv_amd.models.houv import HOUV, solve_model
    src, tgt, pose = synthetic.make_pairs(8, 512, seed=123)
    s, t, p = src.to(dev), tgt.to(dev), pose.to(dev)
    r0, t0, _ = solve_model(HOUV(8 * 32, 0), s, t, p, kernel=32, num_epochs=100)
    r1, t1, T = solve_model_icp(HOUV(8 * 32, 0), s, t, p, kernel=32, num_epochs=100)
    good = r0 < 3.0
    assert bool(good.any())
    assert bool((r1[good] <= r0[good] + 1.0).all())
    assert T.shape == (8, 4, 4) and bool((T[:, 3, 3] == 1).all())


# ---------------------------------------------------------------------------------------------------------------------------
# Float64 parity on every launch path, edge and stop rule.  The yardstick is tests/icp_host.py: the kernel's loop restated in
# numpy, run in float64 (the reference) and in float32 (what the formula itself loses); bound = 4 x that loss + a floor of a few
# roundings (icp_host.reference_and_bounds).  The inputs keep every decision of the loop far from its threshold
# (tests/test_icp_host.py checks that on the CPU), so the kernel has to take the reference's correspondences and stop where it stops.
# DESIGN.md section 9.1 tabulates the measured error / yardstick ratios.
# ---------------------------------------------------------------------------------------------------------------------------
import icp_host as host  # noqa: E402

BOTTOM = np.array([0, 0, 0, 1], np.float32)


def _batch(dev, cases, srcs=None):
    """-> (src, tgt, init or None) on the device for cases of one (N, M)."""
    src = torch.tensor(np.stack([c.src for c in cases] if srcs is None else srcs)).to(dev)
    tgt = torch.tensor(np.stack([c.tgt for c in cases])).to(dev)
    init = None if cases[0].init is None else torch.tensor(np.stack([c.init for c in cases])).to(dev)
    return src, tgt, init


def _refine(dev, cases, cap=30, rel=(1e-6, 1e-6), srcs=None):
    from houv_amd import ops
    src, tgt, init = _batch(dev, cases, srcs)
    out = ops.icp_refine(src, tgt, init, cases[0].max_dist, cap, rel[0], rel[1])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b, i=None, j=None):
    """Bit-equal results (of pair i of a and pair j of b, or of all pairs)."""
    for k in ("T", "fitness", "inlier_rmse", "iterations"):
        x, y = (a[k], b[k]) if i is None else (a[k][i], b[k][j])
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y), k


def _check(tag, out, i, case, ref):
    """Pair i of `out` against the float64 restatement `ref` of `case`; returns the error / yardstick ratios (R, t, rmse)."""
    N = len(case.src)
    T, fit, rmse, it = out["T"][i], out["fitness"][i], out["inlier_rmse"][i], int(out["iterations"][i])
    assert np.array_equal(T[3], BOTTOM), T[3]
    assert np.isfinite(T).all()
    eR, et = host.errors(T, ref)
    er = abs(float(rmse) - ref.rmse)
    ratio = tuple(e / y if y > 0 else float("inf" if e > 0 else "nan") for e, y in zip((eR, et, er), ref.yard))
    print(f"ICP {tag} N={N} M={len(case.tgt)} pair={i} it={it} err_R={eR:.2e} yard_R={ref.yard[0]:.2e} bound_R={ref.bound[0]:.2e} "
          f"err_t={et:.2e} yard_t={ref.yard[1]:.2e} bound_t={ref.bound[1]:.2e} err_rmse={er:.2e} yard_rmse={ref.yard[2]:.2e} "
          f"bound_rmse={ref.bound[2]:.2e} RATIO R={ratio[0]:.2f} t={ratio[1]:.2f} rmse={ratio[2]:.2f}")
    assert it == ref.iterations, (it, ref.iterations)
    assert fit.view(np.int32) == (np.float32(ref.count) / np.float32(N)).view(np.int32), (fit, ref.count, N)
    assert eR <= ref.bound[0], (eR, ref.bound[0])
    assert et <= ref.bound[1], (et, ref.bound[1])
    assert er <= ref.bound[2], (er, ref.bound[2])
    return ratio


@pytest.mark.parametrize("path,N,M", host.PATH_CASES, ids=[f"{p}-{n}x{m}" for p, n, m in host.PATH_CASES])
def test_icp_every_launch_path_within_four_float32_yardsticks(dev, path, N, M):
    """Both ends of every kernel path's range of N (the first one with a tail of idle lanes), targets that end inside a tracking
    unit, inside a sub-tile and on their borders, N != M, a batch whose pairs differ in clouds, poses and inits; 20 % outliers."""
    cases = [host.separated_case(N, M, s) for s in range(host.pairs_of(N))]
    out = _refine(dev, cases)
    for i, case in enumerate(cases):
        ref = host.reference_and_bounds(case)
        assert ref.iterations == 2 and ref.count == case.inlier.sum() and not ref.degenerate
        _check(path, out, i, case, ref)


@pytest.mark.parametrize("path,N,M", host.TAIL_CASES, ids=[f"{p}-{n}x{m}" for p, n, m in host.TAIL_CASES])
def test_icp_lanes_past_the_end_of_the_cloud_do_not_count(dev, path, N, M):
    """The first N of every path, where all but one lane of the last chunk are idle and carry the point (0, 0, 0), with the source
    frame placed so that this point lands on a target (icp_host.tail_case): counted, it would change fitness, means and T."""
    cases = [host.tail_case(N, M, s) for s in range(2)]
    out = _refine(dev, cases)
    for i, case in enumerate(cases):
        _check(f"tail {path}", out, i, case, host.reference_and_bounds(case))


def test_icp_largest_target_cloud_gets_its_lds(dev):
    """The documented limit of M: the largest cloud whose 1024-thread launch fits 160 KiB of LDS by the host's own formula is
    accepted and launched on both block sizes (the second asks for all but 320 B of the 160 KiB); one point more is refused."""
    from houv_amd import _lib, ops
    limit = host.largest_m()
    for N, M in host.lds_cases():
        assert M == limit
        case = host.separated_case(N, M, 0)
        out = _refine(dev, [case], cap=1)
        _check(f"lds {host.smem_bytes(M, 256 if N <= 1024 else 1024)} B", out, 0, case, host.reference_and_bounds(case, 1))
    with pytest.raises(_lib.HouvHipError, match="too large"):
        ops.icp_refine(torch.zeros(1, 8, 3, device=dev), torch.zeros(1, limit + 1, 3, device=dev), None, 0.1, 1)


@pytest.mark.parametrize("N,M", host.STOP_CASES)
def test_icp_iteration_cap_and_stop_rule(dev, N, M):
    case = host.separated_case(N, M, 0)
    for cap in (0, 1, 2, 5):                                   # thresholds 0: nothing is ever < 0, only the cap stops the loop
        out = _refine(dev, [case], cap, (0.0, 0.0))
        ref = host.reference_and_bounds(case, cap, 0.0, 0.0)
        assert ref.iterations == cap
        _check(f"cap {cap}", out, 0, case, ref)
    out = _refine(dev, [case], 30, (1e30, 1e30))               # everything is < 1e30: the first comparison stops it
    ref = host.reference_and_bounds(case, 30, 1e30, 1e30)
    assert ref.iterations == 1
    _check("always", out, 0, case, ref)


@pytest.mark.parametrize("N,M", host.STOP_CASES)
def test_icp_cap_zero_returns_init_bit_for_bit(dev, N, M):
    from houv_amd import ops
    case = host.separated_case(N, M, 0)
    src, tgt, init = _batch(dev, [case])
    init[0, 3] = torch.tensor([7.0, float("nan"), -3.0, 5.0], device=dev)           # the bottom row is not read
    out = {k: v.cpu().numpy() for k, v in ops.icp_refine(src, tgt, init, case.max_dist, 0).items()}
    assert np.array_equal(out["T"][0, :3].view(np.int32), case.init[:3].view(np.int32))
    _check("cap 0, bottom row", out, 0, case, host.reference_and_bounds(case, 0))   # fitness and rmse of the initial pose


def test_icp_pair_without_correspondence_stops_alone(dev):
    N, M = host.NO_CORRESPONDENCE_CASE
    cases = [host.separated_case(N, M, s) for s in range(3)]
    pushed, clearance = host.pushed_away(cases[1])
    assert clearance >= 2
    out = _refine(dev, cases, srcs=[cases[0].src, pushed, cases[2].src])
    assert out["iterations"][1] == 0 and out["fitness"][1] == 0 and out["inlier_rmse"][1] == 0
    assert np.array_equal(out["T"][1, :3].view(np.int32), cases[1].init[:3].view(np.int32)) and np.array_equal(out["T"][1, 3], BOTTOM)
    for i in (0, 2):
        _check("next to an empty pair", out, i, cases[i], host.reference_and_bounds(cases[i]))
        _same(out, _refine(dev, [cases[i]]), i, 0)


def test_icp_radius_is_strict(dev):
    """Distances exactly at, 2^-10 inside and 2^-10 outside the radius, all exact in fp32: only those inside correspond.  Two source
    points near the origin, far from every target, correspond to nothing: the pad slots of the target cloud are not points."""
    from houv_amd import ops
    case = host.threshold_case()
    src, tgt, _ = _batch(dev, [case])
    eye = torch.eye(4, device=dev)[None].contiguous()
    runs = [{k: v.cpu().numpy() for k, v in ops.icp_refine(src, tgt, init, case.max_dist, 0).items()} for init in (None, eye)]
    want = float(np.sqrt(7 * (0.125 - 2.0 ** -10) ** 2 / 11))
    assert case.inlier.sum() == 11
    for out in runs:
        assert out["fitness"][0].view(np.int32) == (np.float32(case.inlier.sum()) / np.float32(len(case.src))).view(np.int32)
        assert abs(float(out["inlier_rmse"][0]) - want) <= 8 * host.EPS32 * want
        assert out["iterations"][0] == 0 and np.array_equal(out["T"][0], np.eye(4, dtype=np.float32))
    _same(runs[0], runs[1])


@pytest.mark.parametrize("flip", [False, True], ids=["a+", "b+"])
@pytest.mark.parametrize("a,b", host.TIE_PAIRS)
def test_icp_lowest_index_wins_an_exact_tie(dev, a, b, flip):
    """Two targets exactly 1/8 from a source point, in one tracking unit, in the two units of a sub-tile, across sub-tiles and in
    the last, padded one; whichever of the two comes first in memory order of x.  Taking the other moves T by 2e-2."""
    case = host.tie_case(a, b, flip)
    ref = host.reference_and_bounds(case, 1, 0.0, 0.0)
    assert ref.iterations == 1 and ref.count == host.TIE_N and not ref.degenerate
    _check(f"tie {a}/{b}", _refine(dev, [case], 1, (0.0, 0.0)), 0, case, ref)


@pytest.mark.parametrize("N,M", host.DEGENERATE_CASES)
def test_icp_degenerate_covariance_still_gives_a_rigid_motion(dev, N, M):
    """One or two distinct pairs: H has rank 0 or 1 and the rotation is arbitrary in any arithmetic, but it is a rotation, T carries
    the inliers' mean onto their targets' mean, and fitness, rmse and the stop do not depend on the rotation taken."""
    cases = [host.separated_case(N, M, s) for s in range(3)]
    out = _refine(dev, cases)
    for i, case in enumerate(cases):
        ref = host.reference_and_bounds(case)
        assert ref.degenerate
        T = out["T"][i].astype(np.float64)
        assert np.isfinite(out["T"][i]).all() and np.array_equal(out["T"][i][3], BOTTOM)
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(T[:3, :3]) - 1) <= 1e-5
        res, er = host.mean_residual(T, case), abs(float(out["inlier_rmse"][i]) - ref.rmse)
        print(f"ICP degenerate N={N} M={M} pair={i} mean_residual={res:.2e} yard={ref.yard[1]:.2e} bound={ref.bound[1]:.2e} "
              f"err_rmse={er:.2e} bound_rmse={ref.bound[2]:.2e}")
        assert res <= ref.bound[1], (res, ref.bound[1])
        assert out["fitness"][i].view(np.int32) == (np.float32(ref.count) / np.float32(N)).view(np.int32)
        assert er <= ref.bound[2], (er, ref.bound[2])
        assert int(out["iterations"][i]) == ref.iterations


def _plumbing(dev):
    N, M = host.PLUMBING_CASE
    cases = [host.separated_case(N, M, s) for s in range(3)]
    return cases, _batch(dev, cases)


def test_icp_is_deterministic_and_stream_ordered(dev):
    from houv_amd import ops
    cases, (src, tgt, init) = _plumbing(dev)
    first = {k: v.cpu().numpy() for k, v in ops.icp_refine(src, tgt, init, cases[0].max_dist, 30).items()}
    _same(first, {k: v.cpu().numpy() for k, v in ops.icp_refine(src, tgt, init, cases[0].max_dist, 30).items()})
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = ops.icp_refine(src, tgt, init, cases[0].max_dist, 30)
    side.synchronize()
    _same(first, {k: v.cpu().numpy() for k, v in out.items()})
    for i, case in enumerate(cases):
        _check("plumbing", first, i, case, host.reference_and_bounds(case))


def test_icp_empty_batch_and_null_outputs(dev):
    from houv_amd import _lib, ops
    cases, (src, tgt, init) = _plumbing(dev)
    out = ops.icp_refine(src[:0], tgt[:0], init[:0], cases[0].max_dist, 30)
    assert out["T"].shape == (0, 4, 4) and out["fitness"].shape == out["inlier_rmse"].shape == out["iterations"].shape == (0,)
    want = ops.icp_refine(src, tgt, init, cases[0].max_dist, 30)["T"]
    T = torch.full((3, 4, 4), float("nan"), device=dev)
    ok = _lib.load().houv_icp_refine(_lib.ptr(src), _lib.ptr(tgt), 3, src.shape[1], tgt.shape[1], _lib.ptr(init), cases[0].max_dist,
                                     30, 1e-6, 1e-6, _lib.ptr(T), None, None, None, _lib.stream_of(src))
    assert ok == 1, _lib.last_error()
    assert torch.equal(T, want)


def test_icp_python_wrapper_converts_its_inputs(dev):
    from houv_amd import icp, ops
    cases, (src, tgt, init) = _plumbing(dev)
    want = ops.icp_refine(src, tgt, init, cases[0].max_dist, 30)["T"]
    wide = torch.zeros(3, src.shape[1], 6, device=dev)
    wide[..., :3] = src
    assert not wide[..., :3].is_contiguous()
    zero_row = init.clone()
    zero_row[:, 3, :] = 0
    for s, i0 in ((src.double(), init), (wide[..., :3], init), (src, zero_row), (src, init.double().cpu())):
        assert torch.equal(icp.icp_refine(s, tgt, i0, cases[0].max_dist, 30), want)
    assert torch.equal(zero_row[:, 3, :], torch.zeros(3, 4, device=dev))               # the caller's init is not written


def test_icp_refusals_launch_nothing(dev):
    """Every refusal of the C entry: status 0, the reason in houv_last_error, and the outputs untouched (nothing was launched);
    ops.icp_refine raises it as HouvHipError.  What ops refuses itself never reaches the library."""
    from houv_amd import _lib, ops
    cases, (src, tgt, init) = _plumbing(dev)
    md, limit = cases[0].max_dist, host.largest_m()
    P, N, M = 3, src.shape[1], tgt.shape[1]
    big_src = torch.zeros(1, host.MAX_N + 1, 3, device=dev)
    big_tgt = torch.zeros(1, limit + 1, 3, device=dev)
    lib = _lib.load()
    c_level = [("N = 0", src[:, :0].contiguous(), tgt, init, md, 30, "bad argument"),
               ("M = 0", src, tgt[:, :0].contiguous(), init, md, 30, "bad argument"),
               ("max_iteration = -1", src, tgt, init, md, -1, "bad argument"),
               ("max_dist = 0", src, tgt, init, 0.0, 30, "bad argument"),
               ("max_dist = -1", src, tgt, init, -1.0, 30, "bad argument"),
               ("max_dist = NaN", src, tgt, init, float("nan"), 30, "bad argument"),
               ("N = 8193", big_src, tgt[:1], None, md, 30, "too large"),
               ("M = limit + 1", src[:1], big_tgt, None, md, 30, "too large")]
    for what, s, t, i0, d, cap, text in c_level:
        p = s.shape[0]
        T = torch.full((p, 4, 4), -7.0, device=dev)
        fit, rmse = torch.full((p,), -7.0, device=dev), torch.full((p,), -7.0, device=dev)
        iters = torch.full((p,), -7, dtype=torch.int32, device=dev)
        ok = lib.houv_icp_refine(_lib.ptr(s), _lib.ptr(t), p, s.shape[1], t.shape[1], _lib.ptr(i0), d, cap, 1e-6, 1e-6,
                                 _lib.ptr(T), _lib.ptr(fit), _lib.ptr(rmse), _lib.ptr(iters), _lib.stream_of(src))
        assert ok == 0 and text in _lib.last_error(), (what, ok, _lib.last_error())
        torch.cuda.synchronize(dev)
        assert bool((T == -7).all() and (fit == -7).all() and (rmse == -7).all() and (iters == -7).all()), what
        with pytest.raises(_lib.HouvHipError) as e:
            ops.icp_refine(s, t, i0, d, cap)
        assert text in str(e.value) and text in _lib.last_error(), (what, str(e.value))
    ok = lib.houv_icp_refine(None, _lib.ptr(tgt), P, N, M, None, md, 30, 1e-6, 1e-6, _lib.ptr(torch.zeros(P, 4, 4, device=dev)),
                             None, None, None, _lib.stream_of(src))
    assert ok == 0 and "null pointer" in _lib.last_error()
    before = _lib.last_error()
    py_level = [("CPU src", src.cpu(), tgt, init, "CPU tensor"), ("CPU tgt", src, tgt.cpu(), init, "CPU tensor"),
                ("CPU init", src, tgt, init.cpu(), "CPU tensor"), ("P mismatch", src, tgt[:2], init, r"src\[P,N,3\], tgt\[P,M,3\]"),
                ("init [P,3,4]", src, tgt, init[:, :3].contiguous(), r"init must be \[P,4,4\]"),
                ("init [2,4,4]", src, tgt, init[:2], r"init must be \[P,4,4\]")]
    for what, s, t, i0, text in py_level:
        with pytest.raises(_lib.HouvHipError, match=text):
            ops.icp_refine(s, t, i0, md, 30)
        assert _lib.last_error() == before, what
