"""CPU: tests/ef_expand_host.py, the restatement that houv_ef_expand and houv_ef_expand_backward are tested against (DESIGN.md
section 9.16).  Its float64 forward is EF_expansion as tests/ecg_host.py states it (which pins the reinterpretation of conv2's
channels as sub-rows), its backward matches central differences, and each planted fault changes the result."""
import numpy as np
import pytest

import ecg_host
import ef_expand_host as host


def make_case(C, O, r, k, N=9, B=2, seed=0, out_of_range=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, N, C))
    idx = rng.integers(0, N, size=(B, N, k)).astype(np.int32)
    idx[:, :, 0] = np.arange(N)
    if out_of_range:
        idx[0, 1, -1], idx[-1, 2, -1], idx[0, 3, 0] = N + 3, -2, 2 * N + 1
    s = lambda *shape: rng.standard_normal(shape) / np.sqrt(shape[-1])
    return dict(x=x, idx=idx, W1=s(O, 2 * C), b1=s(O), W2=s(O * r, O + 2 * C), b2=s(O * r), W3=s(O, O), b3=s(O), r=r)


def run_forward(c, dtype=np.float64, faults=()):
    proj, W2a = host.projections(c["x"], c["W1"], c["b1"], c["W2"], c["b2"], dtype)
    return host.forward(proj, c["idx"], W2a, c["W3"], c["b3"], c["r"], dtype, faults)


@pytest.mark.parametrize("C,O", [(12, 8), (8, 12)])
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 4])
def test_forward_is_ef_expansion(C, O, r, k):
    c = make_case(C, O, r, k, seed=7 * r + k)
    out, arg = run_forward(c)
    ref = ecg_host.ef_expansion(np.transpose(c["x"], (0, 2, 1)), c["idx"], c["W1"], c["b1"], c["W2"], c["b2"], c["W3"], c["b3"], r)
    ref = np.transpose(ref, (0, 2, 1))                                            # [B, N r, O]
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() <= 1e-12 * np.abs(ref).max()
    assert arg.min() >= 0 and arg.max() < k


def _loss(c, G):
    return float((run_forward(c)[0] * G).sum())


@pytest.mark.parametrize("C,O,r,k", [(6, 4, 2, 4), (4, 6, 3, 3), (5, 4, 1, 1)])
def test_backward_matches_central_differences(C, O, r, k):
    c = make_case(C, O, r, k, N=7, seed=11, out_of_range=True)
    rng = np.random.default_rng(5)
    proj, W2a = host.projections(c["x"], c["W1"], c["b1"], c["W2"], c["b2"])
    out, arg = host.forward(proj, c["idx"], W2a, c["W3"], c["b3"], r)
    G = rng.standard_normal(out.shape)
    g = host.backward(proj, c["idx"], arg, W2a, c["W3"], G, r)

    def loss(p, w2a, w3, b3):
        return float((host.forward(p, c["idx"], w2a, w3, b3, r)[0] * G).sum())

    base = (proj, W2a, c["W3"], c["b3"])
    for which, grad in enumerate((g["gproj"], g["gW2a"], g["gW3"], g["gb3"])):
        for trial in range(3):
            d = rng.standard_normal(base[which].shape)
            h = 1e-6
            hi = [a + h * d if i == which else a for i, a in enumerate(base)]
            lo = [a - h * d if i == which else a for i, a in enumerate(base)]
            fd = (loss(*hi) - loss(*lo)) / (2 * h)
            an = float((grad * d).sum())
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (which, trial, fd, an)


def test_backward_through_the_projections_reaches_x_and_both_convolutions():
    """The chain the autograd graph adds around the node: proj's gradient through the four column slices."""
    C, O, r, k = 5, 4, 2, 3
    c = make_case(C, O, r, k, N=6, seed=3)
    rng = np.random.default_rng(9)
    G = rng.standard_normal((2, 6 * r, O))
    proj, W2a = host.projections(c["x"], c["W1"], c["b1"], c["W2"], c["b2"])
    _, arg = host.forward(proj, c["idx"], W2a, c["W3"], c["b3"], r)
    gp = host.backward(proj, c["idx"], arg, W2a, c["W3"], G, r)["gproj"]
    gU, gV, gP, gQ = gp[..., :O], gp[..., O:2 * O], gp[..., 2 * O:2 * O + O * r], gp[..., 2 * O + O * r:]
    W1, W2 = c["W1"], c["W2"]
    gx = gU @ W1[:, :C] + gV @ W1[:, C:] + (gP @ W2[:, O:O + C] + gQ @ W2[:, O + C:]) * (c["x"] > 0)
    d = rng.standard_normal(c["x"].shape)
    h = 1e-6
    fd = (_loss(dict(c, x=c["x"] + h * d), G) - _loss(dict(c, x=c["x"] - h * d), G)) / (2 * h)
    assert abs(fd - float((gx * d).sum())) <= 1e-6 * max(1.0, abs(fd))


@pytest.mark.parametrize("fault", ["stride", "highest", "no_P", "unclamped"])
def test_planted_faults_change_the_result(fault):
    c = make_case(6, 4, 2, 4, seed=2, out_of_range=True)
    if fault == "highest":                                                        # a tie: two slots list the same point
        c["idx"][:, :, 3] = c["idx"][:, :, 1]
    out, arg = run_forward(c)
    bad_out, bad_arg = run_forward(c, faults=(fault,))
    if fault == "highest":
        assert np.array_equal(out, bad_out) and not np.array_equal(arg, bad_arg)
        assert (arg != 3).all() and (bad_arg != 1).all()
    else:
        assert np.abs(out - bad_out).max() > 1e-3


def test_nan_and_ties():
    c = make_case(6, 4, 2, 3, seed=4)
    c["idx"][0, 2, :] = 5                                                         # one point three times: slot 0 wins every column
    c["x"][1, 4, 0] = np.nan                                                      # a NaN row: NaN wherever it is centre or neighbour
    out, arg = run_forward(c)
    r = c["r"]
    assert (arg[0, 2 * r:3 * r] == 0).all()
    assert (arg[1, 4 * r:5 * r] == -1).all() and np.isnan(out[1, 4 * r:5 * r]).all()
    lists4 = (c["idx"][1] == 4)
    for n in range(c["idx"].shape[1]):
        if n != 4 and not lists4[n].all():
            assert not np.isnan(out[1, n * r:(n + 1) * r]).any()
            for j in np.nonzero(lists4[n])[0]:
                assert (arg[1, n * r:(n + 1) * r] != j).all()
    proj, W2a = host.projections(c["x"], c["W1"], c["b1"], c["W2"], c["b2"])
    g = host.backward(proj, c["idx"], arg, W2a, c["W3"], np.ones_like(out), r)
    assert all(np.isfinite(v).all() for v in g.values())
    assert (g["gproj"][1, 4, :4] == 0).all()                                     # gU of the NaN row: nothing lands
