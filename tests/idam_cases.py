"""Inputs, float64 yardsticks and bounds of tests/test_gpu_idam.py, shared with the CPU.

    python tests/idam_cases.py

measures, on exactly the inputs the GPU tests use, the float32 restatement (tests/idam_host.py) against its float64 run, and the
share of flagged rows of every case.  TOL_ROWMAX / TOL_SCORE below are 4x the maximum over all cases (the margin DeepGMR uses:
it covers a different but equally careful summation order); they are NOT taken from the kernel.  The script fails when a
constant below is more than 5 % from what it measures, or when a case has more than MAX_FLAGGED flagged rows."""
import numpy as np

import idam_host as host

# (B, Ms, Mt, E): a single pair; ragged; one full tile; one row past two tiles and 31 columns; whole tiles; a second column chunk;
# the config's own M = 2048 // 6 (several tiles per row in both directions); the smallest E
SIM_SHAPES = [(1, 1, 1, 64), (2, 5, 7, 64), (2, 16, 16, 64), (1, 33, 31, 64), (3, 64, 64, 64), (1, 65, 130, 64),
              (2, 341, 341, 64), (2, 33, 31, 4)]
CLAMP_SHAPES = [(2, 5, 7, 64), (1, 65, 130, 64)]
EDGE_SHAPES = [(1, 12, 12, 3, 4), (2, 13, 12, 64, 64), (1, 65, 5, 8, 8), (2, 300, 12, 64, 64)]     # (B, N, k, C, ldo)
MAX_FLAGGED = 0.02

MEASURED_ROWMAX, MEASURED_SCORE = 1.26e-06, 1.35e-05     # float32 restatement vs float64, maximum over SIM_SHAPES (this script)
TOL_ROWMAX, TOL_SCORE = 4 * MEASURED_ROWMAX, 4 * MEASURED_SCORE


def sim_params(rng, E, b4=None):
    """W1, s1, t1, W2, b2, W3, s3, t3, w4, b4: uniform(-1, 1) * 2 / sqrt(fan_in) weights, folded-BatchNorm-like scale/shift; w4
    is scaled so that the scores spread over about +-20 and some of them clamp."""
    u = lambda *shape: rng.uniform(-1, 1, shape)
    W1 = u(32, 2 * E + 4) * 2 / np.sqrt(2 * E + 4)
    W2, W3 = u(32, 32) * 2 / np.sqrt(32), u(32, 32) * 2 / np.sqrt(32)
    s1, s3 = rng.uniform(0.5, 1.5, 32), rng.uniform(0.5, 1.5, 32)
    t1, t3 = rng.normal(0, 0.2, 32), rng.normal(0, 0.2, 32)
    b2 = rng.uniform(-0.1, 0.1, 32)
    w4 = u(32) * 20 / np.sqrt(32)
    b4 = np.array([rng.uniform(-0.1, 0.1) if b4 is None else b4])
    return tuple(a.astype(np.float32) for a in (W1, s1, t1, W2, b2, W3, s3, t3, w4, b4))


def sim_case(B, Ms, Mt, E, b4=None):
    """-> (src, tgt, es, et, par).  Source point 0 of every pair equals target point Mt - 1 (d = 0, so u = 0 and not NaN); when
    Mt >= 4 the target points 1 and Mt - 2 are copies of point 2, embedding included: equal scores, the lowest j wins."""
    rng = np.random.default_rng(1000 * Ms + 10 * Mt + E + B)
    src = rng.uniform(-0.5, 0.5, (B, Ms, 3)).astype(np.float32)
    tgt = rng.uniform(-0.5, 0.5, (B, Mt, 3)).astype(np.float32)
    es = rng.standard_normal((B, Ms, E)).astype(np.float32)
    et = rng.standard_normal((B, Mt, E)).astype(np.float32)
    if Mt >= 4:
        tgt[:, 1], et[:, 1] = tgt[:, 2], et[:, 2]
        tgt[:, Mt - 2], et[:, Mt - 2] = tgt[:, 2], et[:, 2]
    src[:, 0] = tgt[:, Mt - 1]
    return src, tgt, es, et, sim_params(rng, E, b4)


def sim_yardstick(case):
    """-> (the float64 restatement's dict, flagged[B,Ms])."""
    y = host.simmat(*case, dtype=np.float64)
    return y, host.flagged_rows(y["scores"], TOL_SCORE)


def check_sim(rowmax, scores, cidx, corr, case, y, flagged, what):
    """The kernel's outputs (NumPy; None = not asked for) against the yardstick; prints each figure before it asserts."""
    tgt = case[1]
    if rowmax is not None:
        e = float(np.abs(rowmax - y["rowmax"]).max())
        print(what, "rowmax error", e, "bound", TOL_ROWMAX)
        assert e <= TOL_ROWMAX, what
    if scores is not None:
        e = float(np.abs(scores - y["scores"]).max())
        print(what, "score error", e, "bound", TOL_SCORE)
        assert e <= TOL_SCORE, what
    print(what, "flagged rows", int(flagged.sum()), "of", flagged.size)
    assert flagged.mean() <= MAX_FLAGGED, what
    if cidx is not None:
        assert cidx.dtype == np.int32 and (cidx >= 0).all() and (cidx < tgt.shape[1]).all()
        assert np.array_equal(cidx[~flagged], y["corr_idx"][~flagged]), what
        picked = np.take_along_axis(y["scores"], cidx[..., None].astype(np.int64), axis=-1)[..., 0]
        assert (y["scores"].max(-1) - picked <= TOL_SCORE).all(), what
    if corr is not None and cidx is not None:
        want = np.swapaxes(tgt[np.arange(len(tgt))[:, None], cidx], 1, 2)
        assert np.array_equal(corr.view(np.int32), np.ascontiguousarray(want).view(np.int32)), what


def edge_case(B, N, k, C):
    """x[B,N,C], idx[B,N,k + 2] (a row pitch wider than k): entries outside 0..N-1 (clamped) and repeated entries included."""
    rng = np.random.default_rng(7 * N + k + C)
    x = rng.standard_normal((B, N, C)).astype(np.float32)
    idx = rng.integers(0, N, (B, N, k + 2)).astype(np.int32)
    idx[:, :, 0] = np.arange(N)                     # the point itself: an exact zero row
    idx[:, 0, 1] = -3                               # below the range
    idx[:, N - 1, k - 1] = N + 5                    # above it
    idx[:, 1, 2:4] = idx[:, 1, 1:2]                 # repeated
    return x, idx


def main():
    worst_r = worst_s = 0.0
    for shape in SIM_SHAPES:
        case = sim_case(*shape)
        y, flagged = sim_yardstick(case)
        f = host.simmat(*case, dtype=np.float32)
        er, es = float(np.abs(f["rowmax"] - y["rowmax"]).max()), float(np.abs(f["scores"] - y["scores"]).max())
        top = y["scores"].max(-1)
        print(shape, f"rowmax f32-f64 {er:.3g}, scores {es:.3g}, flagged {int(flagged.sum())}/{flagged.size}, rows with the maximum "
              f"at the clamp {int((np.abs(top) == 20).sum())}, |rowmax| up to {np.abs(y['rowmax']).max():.3g}")
        check_sim(f["rowmax"], f["scores"], f["corr_idx"], None, case, y, flagged, f"float32 restatement {shape}")
        worst_r, worst_s = max(worst_r, er), max(worst_s, es)
    print(f"maximum over the cases: rowmax {worst_r:.3g}, scores {worst_s:.3g}")
    # within 5 %: another host's sqrt or BLAS-free sums may differ in the last place, a changed input or formula does not hide in that
    assert abs(worst_r / MEASURED_ROWMAX - 1) <= 0.05 and abs(worst_s / MEASURED_SCORE - 1) <= 0.05, "update MEASURED_*"


if __name__ == "__main__":
    main()
