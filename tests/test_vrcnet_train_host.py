"""CPU: the float64 restatement of the latent head of VRCNet's "train" prefix (tests/vrcnet_train_host.py) against the REAL
reference's float32 values and autograd gradients stored by tests/golden/make_golden_vrcnet_train.py (which ran the reference's
own lines): within 4x the stored float32 spread on every value, both feature gradients and the kept entries of all 24 parameter
gradients; the stored float64 numbers are this restatement's; and the gradient is the derivative of the loss it restates
(central differences along seeded directions)."""
import numpy as np
import pytest

import vrcnet_train_host as host

FILE = "g33_vrcnet_train_head.npz"
NAMES = [("", n) for n in host.VALUES] + [("grad_", n) for n in ("feat_x", "feat_y") + tuple(n for n, _ in host.spec())]


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden(FILE)
    a = host.case(int(g["seed"]))
    for n, v in zip(("feat_x", "feat_y", "eps_q", "eps_p"), a[1:5]):
        assert np.array_equal(v, g[n]), n                          # the case is a function of the seed
    return g, a, host.head(*a, np.float64)


def test_fixture_is_complete_and_qualifies(fixture):
    g, _, _ = fixture
    assert bool(g["qualifies"])
    for kind, n in NAMES:
        assert f"ref_{kind}{n}" in g.files and f"f64_{kind}{n}" in g.files and float(g[f"spread_{kind}{n}"]) > 0, kind + n
    assert sum(f.endswith("_idx") for f in g.files) == 12          # the weights are subsampled, the biases and features whole


@pytest.mark.parametrize("kind,name", NAMES, ids=[k + n for k, n in NAMES])
def test_float64_restatement_against_the_reference(fixture, kind, name):
    g, _, (values, grads) = fixture
    mine = (grads if kind else values)[name].reshape(-1)
    key = f"{kind}{name}_idx"
    if key in g.files:
        mine = mine[g[key].astype(np.int64)]
    spread = float(g[f"spread_{kind}{name}"])
    assert np.allclose(mine, g[f"f64_{kind}{name}"], rtol=1e-9, atol=1e-9 * spread)
    err = float(np.abs(g[f"ref_{kind}{name}"].astype(np.float64) - mine).max())
    print(f"{kind}{name}: reference vs float64 restatement {err:.3g}, {err / spread:.2f}x the float32 spread")
    assert err <= 4 * spread


def test_restated_gradient_is_the_derivative_of_the_restated_loss(fixture):
    _, (state, fx, fy, eq, ep, G), (base, grads) = fixture
    fix = (base["p_mu"], base["p_std"])                  # dl_g's first distribution is detached: it stays where it is

    def loss(st, x, y):
        v, _ = host.head(st, x, y, eq, ep, G, np.float64, prior_fix=fix)
        return 20 * (v["dl_rec"].mean() + v["dl_g"].mean()) + (G.astype(np.float64) * v["global_feat"]).sum()

    rng = np.random.default_rng(5)
    h = 1e-6
    st64 = {n: np.asarray(v, np.float64) for n, v in state.items()}
    for n in ("feat_x", "feat_y", "prior_infer.conv2.weight", "generator.conv1.bias", "posterior_infer1.conv_res.weight"):
        D = rng.standard_normal(grads[n].shape)
        if n.startswith("feat"):
            D = D * (np.abs(fx if n == "feat_x" else fy) > 1e-3)            # a leaf at a ReLU kink does not move across it
            x1, x0 = (fx + s * h * D if n == "feat_x" else fx for s in (1, -1))
            y1, y0 = (fy + s * h * D if n == "feat_y" else fy for s in (1, -1))
            fd = (loss(st64, x1, y1) - loss(st64, x0, y0)) / (2 * h)
        else:
            up, dn = dict(st64), dict(st64)
            up[n], dn[n] = st64[n] + h * D, st64[n] - h * D
            fd = (loss(up, fx, fy) - loss(dn, fx, fy)) / (2 * h)
        an = float((grads[n] * D).sum())
        print(f"{n}: central difference {fd:.8e}, restated gradient {an:.8e}")
        assert abs(fd - an) <= 1e-5 * max(abs(an), 1.0)
