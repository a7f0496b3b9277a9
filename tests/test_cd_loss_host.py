"""CPU: the host restatement of the Chamfer loss node (tests/cd_loss_host.py, the reference of tests/test_gpu_cd_loss.py) is the
gradient of calc_cd's loss -- against central differences of the float64 loss along seeded directions, and against torch autograd
of the gather-based composition -- its float32 form stays within the rounding of its own sums, both summation paths are covered,
and each planted fault changes the result."""
import numpy as np
import pytest

import cd_loss_host as host

STEP = 1e-6
# (B, N, M): a single point on either side, lists on both sides of host.LONG (M = 2 with N = 80: at least 40 entries in one list)
SHAPES = [(2, 12, 9), (1, 1, 3), (2, 5, 1), (1, 80, 2), (3, 33, 40)]


def _case(B, N, M, seed):
    rng = np.random.default_rng(seed)
    out = rng.uniform(-0.5, 0.5, (B, M, 3)).astype(np.float32)
    gt = rng.uniform(-0.5, 0.5, (B, N, 3)).astype(np.float32)
    g_p = rng.uniform(0.5, 1.5, B).astype(np.float32)
    g_t = rng.uniform(-1.5, 1.5, B).astype(np.float32)
    d1, i1 = host.nearest(gt, out)
    d2, i2 = host.nearest(out, gt)
    return out, gt, d1, d2, i1, i2, g_p, g_t


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_is_the_gradient_of_the_loss(shape):
    # no arg-min may flip within the step: a point moves by at most sqrt(3) STEP, so clouds are drawn until every
    # nearest-neighbour margin exceeds 1000 STEP
    for seed in range(91, 123):
        out, gt, d1, d2, i1, i2, g_p, g_t = _case(*shape, seed=seed)
        if min(host.margins(gt, out), host.margins(out, gt)) > 1e3 * STEP:
            break
    else:
        raise AssertionError(f"{shape}: no seed in 91..122 gives clouds with margins above {1e3 * STEP}")
    g64 = host.backward(out, gt, d1, d2, i1, i2, g_p, g_t, np.float64)
    total = lambda o: sum((c * v).sum() for c, v in zip((g_p.astype(np.float64), g_t.astype(np.float64)), host.loss(o, gt)))
    rng = np.random.default_rng(92)
    for _ in range(4):
        D = rng.uniform(-1, 1, out.shape)
        o = out.astype(np.float64)
        fd = (total(o + STEP * D) - total(o - STEP * D)) / (2 * STEP)
        an = float((g64 * D).sum())
        print(f"{shape}: central difference {fd:.10e}, restatement {an:.10e}")
        assert abs(fd - an) <= 1e-6 * max(abs(an), np.abs(g64).sum() * 1e-3)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_against_autograd_of_the_gather_composition(shape):
    out, gt, d1, d2, i1, i2, g_p, g_t = _case(*shape, seed=93)
    ref, r1, r2 = host.composition_grad(out, gt, i1, i2, g_p, g_t)
    assert np.allclose(r1, d1, rtol=1e-12, atol=0) and np.allclose(r2, d2, rtol=1e-12, atol=0)
    g64, mag, length = host.backward(out, gt, d1, d2, i1, i2, g_p, g_t, np.float64, want_mag=True)
    assert np.abs(g64 - ref).max() <= 1e-12 * mag.max()
    B, N, M = shape
    if N == 80:
        assert length.max() > host.LONG                                          # the butterfly path ran
    # float32: each term carries a few roundings (difference, square root, quotient, two products, one sum) and a sum of L
    # terms L more; (L + 8) ulps of the sum of the terms' magnitudes bounds it
    g32 = host.backward(out, gt, d1, d2, i1, i2, g_p, g_t, np.float32)
    assert g32.dtype == np.float32
    err = np.abs(g32.astype(np.float64) - g64).max(-1)
    assert (err <= (length + 8) * 2.0 ** -23 * mag).all()
    assert err.max() > 0 or N * M == 1


def test_long_and_short_paths_sum_the_same_terms():
    """One output row, every ground-truth point in its list, at the lengths around the path switch: the float64 sums of both
    paths equal the plain float64 sum of the terms."""
    rng = np.random.default_rng(94)
    for N in (host.LONG - 1, host.LONG, host.LONG + 1, host.LONG + 2, 65, 200):
        out = rng.uniform(-0.5, 0.5, (1, 1, 3))
        gt = rng.uniform(-0.5, 0.5, (1, N, 3))
        d1, i1 = host.nearest(gt, out)
        d2, i2 = host.nearest(out, gt)
        g = host.backward(out, gt, d1, d2, i1, i2, [1.0], [0.5], np.float64)
        ref, _, _ = host.composition_grad(out, gt, i1, i2, [1.0], [0.5])
        assert np.abs(g - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("fault", host.FAULTS)
def test_planted_faults_change_the_result(fault):
    out, gt, d1, d2, i1, i2, g_p, g_t = _case(2, 12, 9, seed=95)
    good = host.backward(out, gt, d1, d2, i1, i2, g_p, g_t, np.float64)
    bad = host.backward(out, gt, d1, d2, i1, i2, g_p, g_t, np.float64, fault=fault)
    assert np.abs(bad - good).max() > 1e-3 * np.abs(good).max(), fault


def test_a_coincident_pair_is_not_finite_and_indices_are_clamped():
    out, gt, d1, d2, i1, i2, g_p, g_t = _case(1, 6, 4, seed=96)
    gt[0, 2] = out[0, 1]
    d1, i1 = host.nearest(gt, out)
    d2, i2 = host.nearest(out, gt)
    assert d1[0, 2] == 0 and d2[0, 1] == 0 and i1[0, 2] == 1 and i2[0, 1] == 2
    for dt in (np.float32, np.float64):
        g = host.backward(out, gt, d1, d2, i1, i2, g_p, g_t, dt)
        assert not np.isfinite(g[0, 1]).any() and np.isfinite(np.delete(g[0], 1, 0)).all()
    wild1, wild2 = i1.copy(), i2.copy()
    wild1[0, 0], wild1[0, 5], wild2[0, 0], wild2[0, 3] = -7, 99, 1 << 30, -1
    a = host.backward(out, gt, d1, d2, wild1, wild2, g_p, g_t, np.float32)
    b = host.backward(out, gt, d1, d2, np.clip(wild1, 0, 3), np.clip(wild2, 0, 5), g_p, g_t, np.float32)
    assert np.array_equal(a, b, equal_nan=True)
