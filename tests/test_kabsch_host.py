"""CPU: the NumPy restatement of houv_kabsch's contract (tests/kabsch_host.py) against the torch oracle and the reference's
golden, and the properties of its input builders that tests/test_gpu_kabsch.py relies on."""
import numpy as np
import pytest
import torch

import kabsch_host as host
from oracle import houv_ref_cpu as orc


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("reflect", [False, True])
def test_float64_restatement_equals_the_oracle(weighted, offset, reflect):
    for B, N in ((5, 37), (4, 40), (2, 257)):
        src, corr, w = host.make_case(B, N, weighted, offset, reflect)
        R, t = host.kabsch(src, corr, w, np.float64)
        Ro, to = orc.kabsch_svd(torch.tensor(src).double(), torch.tensor(corr).double(),
                                None if w is None else torch.tensor(w).double())
        assert Ro.dtype == torch.float64
        # 1e-12 of the largest value: the weighted t of an offset cloud is a sum of N terms of size 100
        np.testing.assert_allclose(R, Ro.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(t, to.numpy(), rtol=0, atol=1e-12 * max(1.0, np.abs(to.numpy()).max()))
        assert (np.linalg.det(R) > 0.999999).all()


@pytest.mark.parametrize("dtype,atol", [(np.float64, 2e-5), (np.float32, 2e-5)])
def test_restatement_reproduces_the_svdhead_golden(golden, dtype, atol):
    g = golden("g7_svdhead.npz")
    R, t = host.kabsch(g["src"], g["corr"], None, dtype)
    np.testing.assert_allclose(R, g["R"], atol=atol)
    np.testing.assert_allclose(t, g["t"], atol=atol)
    Rw, tw = host.kabsch(g["src"], g["corr"], g["w"], dtype)
    np.testing.assert_allclose(Rw, g["R_w"], atol=atol)
    np.testing.assert_allclose(tw, g["t_w"], atol=atol)


def test_builders_make_what_the_gpu_tests_rely_on():
    for N in (3, 37, 64, 257, 2048):
        src, corr, w = host.make_case(5, N, True, True, False)
        assert src.dtype == corr.dtype == w.dtype == np.float32 and src.shape == corr.shape == (5, 3, N) and w.shape == (5, 1, N)
        assert ((w == 0).sum(axis=(1, 2)) == N // 10).all() and (w >= 0).all() and (w < 1).all()
        assert np.abs(src.mean(2) - np.array([100.0, -100.0, 100.0])).max() < 0.5          # unit extent, far from the origin
        assert (np.ptp(src, axis=2) <= 1.0 + 1e-4).all()
        assert host.polar_gap(src, corr, w) >= 0.05
    # the mirrored correspondences put H on the reflection branch (det(V U^T) < 0 before the fix), the plain ones do not
    for reflect in (False, True):
        src, corr, _ = host.make_case(5, 65, False, False, reflect)
        s = src.astype(np.float64)
        c = corr.astype(np.float64)
        H = (s - s.mean(2, keepdims=True)) @ np.swapaxes(c - c.mean(2, keepdims=True), 1, 2)
        U, S, Vt = np.linalg.svd(H)
        d = np.linalg.det(np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2))
        assert ((d < 0) == reflect).all()
        assert (S[:, 0] > 1.3 * S[:, 1]).all() and (S[:, 1] > 1.3 * S[:, 2]).all()          # distinct singular values
        R, _ = host.kabsch(src, corr, None, np.float64)
        assert (np.linalg.det(R) > 0.999999).all()


def test_bound_is_four_yardsticks_plus_the_floor():
    R64, t64, yard, bound = host.reference_and_bounds(5, 257, True, True, False)
    src, corr, w = host.make_case(5, 257, True, True, False)
    R32, t32 = host.kabsch(src, corr, w, np.float32)
    assert R32.dtype == np.float32
    assert yard == host.errors(R32, t32, R64, t64) and yard[0] > 0 and yard[1] > 0
    assert bound[0] == 4 * yard[0] + 8 * 2.0 ** -24 * np.abs(R64).max()
    assert bound[1] == 4 * yard[1] + 8 * 2.0 ** -24 * np.abs(t64).max()
