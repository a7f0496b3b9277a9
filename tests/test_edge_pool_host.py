"""CPU: the NumPy restatement of houv_edge_pool / houv_edge_pool_backward (tests/edge_pool_host.py) is what it claims to be --
gather plus max on finite inputs, the derivative of that by central differences -- and is sharp enough that the faults a kernel
could carry (the wrong tie, a dropped centre term, an unclamped index) change its result."""
import numpy as np

import edge_pool_host as host


def _case(seed, B=2, N=23, S=9, C=5, pk=6, dtype=np.float64):
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((B, N, C)).astype(dtype)
    p_idx = rng.integers(0, N, (B, S)).astype(np.int32)
    pn_idx = rng.integers(0, N, (B, S, pk)).astype(np.int32)
    g = rng.standard_normal((B, S, 2 * C)).astype(dtype)
    return feat, p_idx, pn_idx, g


def test_forward_is_gather_plus_max_on_finite_inputs():
    for dtype in (np.float32, np.float64):
        feat, p_idx, pn_idx, _ = _case(1, dtype=dtype)
        out, arg = host.forward(feat, p_idx, pn_idx)
        C = feat.shape[2]
        for b in range(feat.shape[0]):
            nb = feat[b, pn_idx[b]]                                       # (S,pk,C)
            assert np.array_equal(out[b, :, :C], feat[b, p_idx[b]])
            assert np.array_equal(out[b, :, C:], nb.max(axis=1))
            assert np.array_equal(arg[b], nb.argmax(axis=1))               # numpy's argmax is the first maximum too
        assert out.dtype == dtype and arg.dtype == np.int8


def test_backward_is_the_derivative_by_central_differences():
    feat, p_idx, pn_idx, g = _case(2)                                     # continuous random values: no ties
    out, arg = host.forward(feat, p_idx, pn_idx)
    got = host.backward(g, p_idx, pn_idx, arg, feat.shape[1])
    loss = lambda f: float((host.forward(f, p_idx, pn_idx)[0] * g).sum())
    h = 1e-6                                                              # far below the gap between a maximum and its runner-up
    num = np.zeros_like(feat)
    for i in np.ndindex(*feat.shape):
        fp, fm = feat.copy(), feat.copy()
        fp[i] += h
        fm[i] -= h
        num[i] = (loss(fp) - loss(fm)) / (2 * h)
    # the loss is piecewise linear in feat, so the difference quotient is exact up to the rounding of the two sums
    np.testing.assert_allclose(got, num, rtol=0, atol=1e-8)


def test_float32_backward_adds_in_the_stated_order():
    # three terms on one row whose float32 sum depends on the order: (1e8 + 1) - 1e8 = 0 in this order, 1 in another
    feat = np.zeros((1, 2, 1), dtype=np.float32)
    p_idx = np.array([[0, 0, 0]], dtype=np.int32)
    pn_idx = np.ones((1, 3, 1), dtype=np.int32)
    g = np.zeros((1, 3, 2), dtype=np.float32)
    g[0, :, 0] = (1e8, 1.0, -1e8)
    arg = host.forward(feat, p_idx, pn_idx)[1]
    got = host.backward(g, p_idx, pn_idx, arg, 2)
    assert got[0, 0, 0] == np.float32(np.float32(np.float32(1e8) + np.float32(1)) + np.float32(-1e8)) == 0
    assert got.dtype == np.float32


def test_planted_faults_change_the_result():
    feat, p_idx, pn_idx, g = _case(3)
    N = feat.shape[1]
    pn_idx[:, :, -1] = N + 7                                              # out of range: clamps to the last row
    pn_idx[0, 0, :3] = (4, 9, 11)
    feat[0, (4, 11)] = 5.0                                                # the maximum of sample (0, 0) repeats at slots 0 and 2
    out, arg = host.forward(feat, p_idx, pn_idx)
    assert (arg[0, 0] == 0).all()
    good = host.backward(g, p_idx, pn_idx, arg, N)
    # highest slot in place of the lowest: the gradient moves from row 4 to row 11
    out_hi, arg_hi = host.forward(feat, p_idx, pn_idx, highest_slot=True)
    assert np.array_equal(out_hi, out) and (arg_hi[0, 0] == 2).all()
    assert not np.array_equal(host.backward(g, p_idx, pn_idx, arg_hi, N), good)
    assert not np.array_equal(host.backward(g, p_idx, pn_idx, arg, N, drop_centre=True), good)
    assert not np.array_equal(host.backward(g, p_idx, pn_idx, arg, N, unclamped=True), good)
    # and the clamped lists are what an out-of-range entry means
    assert np.array_equal(host.backward(g, p_idx, host.clamp(pn_idx, N).astype(np.int32), arg, N), good)


def test_special_values():
    nan = np.float32(np.nan)
    feat = np.array([[[0.0, -0.0, nan, nan, 1.0], [0.0, 0.0, 2.0, nan, nan], [0.0, -0.0, nan, nan, 3.0]]], dtype=np.float32)
    p_idx = np.array([[1]], dtype=np.int32)
    pn_idx = np.array([[[0, 1, 2]]], dtype=np.int32)
    out, arg = host.forward(feat, p_idx, pn_idx)
    assert arg[0, 0].tolist() == [0, 0, 1, -1, 2]
    pooled = out[0, 0, 5:]
    assert pooled[0] == 0 and not np.signbit(pooled[0])
    assert pooled[1] == 0 and np.signbit(pooled[1])                        # -0 at slot 0 stays: +0 is not greater
    assert pooled[2] == 2 and np.isnan(pooled[3]) and pooled[4] == 3
    g = np.ones((1, 1, 10), dtype=np.float32)
    gfeat = host.backward(g, p_idx, pn_idx, arg, 3)
    assert gfeat[0, :, 3].tolist() == [0, 1, 0]                            # the all-NaN column: the centre's term only
