"""CPU: the NumPy backward of SA_SKN_Res_encoder (tests/vrcnet_enc_grad_host.py) is the derivative of its forward -- central
differences in float64 along seeded directions, over all parameters at once, over single tensors of every kind of layer, and over
the input with the coordinates held fixed -- its forward is vrcnet_host.encoder's, and the fixture of
tests/golden/make_golden_vrcnet_enc_grad.py (the REAL reference's gradients) agrees with it."""
import numpy as np
import pytest

import ecg_host as eh
import vrcnet_cases as cases
import vrcnet_enc_grad_cases as ec
import vrcnet_enc_grad_host as egh
import vrcnet_host as vh

ARGS = (cases.ENC_K, cases.ENC_PK, cases.ENC_PTS)


@pytest.fixture(scope="module")
def case():
    state = {n: np.asarray(v, np.float64) for n, v in cases.encoder_state().items()}
    x, G = ec.inputs_encoder(1, 3)
    d = eh._Decisions(None)
    want = vh.encoder(state, x, d, *ARGS, np.float64, prefix="")
    dec = {n: d.used[n] for n in egh.decision_names(cases.ENC_K)}
    out, bw = egh.encoder(state, x, dec, *ARGS)
    gx, grads = bw(G)
    return state, x.astype(np.float64), G.astype(np.float64), dec, want, out, gx, grads


def test_forward_is_the_restatement_of_the_inference_tests(case):
    _, _, _, _, want, out, _, _ = case
    assert np.array_equal(out, want)


def test_every_parameter_has_a_gradient_of_its_shape(case):
    state, _, _, _, _, _, gx, grads = case
    assert sorted(grads) == sorted(state) and all(grads[n].shape == state[n].shape for n in state)
    assert gx.shape == (1, 3, cases.ENC_PTS[0])
    for n, g in grads.items():
        assert np.isfinite(g).all()
        assert g.any() != (".fc" in n and "sam_res" in n), n               # one list: the branch softmax is exactly 1


def _quotient(state, x, G, dec, direction, h, coords):
    loss = lambda sgn: float((egh.encoder({n: v + sgn * h * direction.get(n, 0) for n, v in state.items()},
                                          x + sgn * h * direction.get("x", 0), dec, *ARGS, coords=coords)[0] * G).sum())
    return (loss(+1) - loss(-1)) / (2 * h)


@pytest.mark.parametrize("which", ["all parameters", "input", "sam_res1.conv1.weight", "sam_res3.sam.1.sams.0.conv_w.1.weight", "conv5.bias",
                                   "fc1.weight", "fc2.bias", "conv6.weight", "conv8.weight", "conv_out.weight", "sam_res4.conv_res.weight"])
def test_backward_against_central_differences(case, which):
    state, x, G, dec, _, _, gx, grads = case
    rng = np.random.default_rng([37] + [ord(c) for c in which])
    names = list(state) if which == "all parameters" else [] if which == "input" else [which]
    direction = {n: rng.standard_normal(state[n].shape) for n in names}
    if which == "input":
        direction["x"] = rng.standard_normal(x.shape)
    want = sum(float((grads[n] * d).sum()) for n, d in direction.items() if n != "x") + float((gx * direction.get("x", 0)).sum())
    # the network is smooth between its kinks: the quotient's error is O(h^2) plus rounding of the two losses over h.  The step
    # stays below the distance of the nearest ReLU input to 0 along these directions: at 1e-6 the direction over all parameters
    # crosses kinks of sam_res2 .. 4 (1 to 2 % off), at 1e-7 every group agrees to 1e-8
    got = _quotient(state, x, G, dec, direction, 1e-7, x)
    scale = max(abs(want), 1e-3 * float(np.sqrt(sum((grads[n] ** 2).sum() * (d ** 2).sum() for n, d in direction.items() if n != "x") + 1e-300)))
    print(f"{which}: analytic {want:.9e}, central difference {got:.9e}")
    assert abs(got - want) <= 1e-5 * scale, (which, got, want)


def test_fixture_agrees_with_the_restatement(golden):
    g = golden(ec.FILE)
    assert str(g["kind"]) == "pool_upsample"              # no seed below the cap qualified for the whole encoder: DESIGN.md 9.15
    feat, pts, G = ec.inputs_narrow(int(g["seed"]))
    dec = {n: g[f"dec_{n}"].astype(np.int64) for n in ("fps1", "knn_pt1", "three_nn1")}

    def run(dt):
        f, pbw = egh._pool(np.asarray(feat, dtype=dt)[:, :, None, :], dec["fps1"], dec["knn_pt1"], None, "")
        p = pts.astype(dt)
        _, ubw = egh._upsample(f, p, np.take_along_axis(p, dec["fps1"][:, :, None], axis=1), dec["three_nn1"])
        return pbw(ubw(np.asarray(G, dtype=dt)[:, :, None, :]))[:, :, 0].reshape(-1)
    at, spread = g["at_feat"].astype(np.int64), float(g["spread_feat"])
    f64, f32 = run(np.float64), run(np.float32)
    assert np.array_equal(at, ec.sample("feat", f64.size))
    assert np.abs(f64[at] - g["f64_feat"]).max() <= 1e-12
    assert abs(float(np.abs(f32.astype(np.float64) - f64).max()) - spread) <= 1e-12
    assert np.abs(g["ref_feat"].astype(np.float64) - f64[at]).max() <= 4 * spread
