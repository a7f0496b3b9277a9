"""CPU: tests/pcn_grad_host.py, the NumPy backward that tests/test_gpu_pcn_grad.py measures houv_mlp2_max_backward against, is
itself checked against central differences of tests/pcn_host.py's forward in float64.

L = <G, pooled> + <Gy, y> is linear in the block's outputs, so the restatement's gradients under (gpooled, gy) = (G, Gy) are
dL/dparameter.  24 seeded entries per shape (5 each of x, W1, shift1 and W2, 4 of b2) are compared with the central difference
quotient at two steps, 1e-5 and 1e-6.  L is piecewise quadratic in one entry of W1, shift1 or x and linear in one of W2 or b2,
so while no ReLU input and no pool decision changes inside the step -- the seed search below keeps every ReLU input 2e-5 and
every pool's runner-up 1e-4 away -- the central quotient is exact and only its rounding remains, about eps * |L| / step.
Measured: the largest disagreement over both shapes is 3.9e-10 at step 1e-5 and 6.2e-9 at step 1e-6, for gradients of order
0.1 to 10.  The bounds are 10x those."""
import numpy as np
import pytest

import pcn_cases as cases
import pcn_grad_host as ghost
import pcn_host as host

BOUND = {1e-5: 4e-9, 1e-6: 6.2e-8}


def _case(Cin, H, Cout):
    B, N = 1, 5
    for seed in range(64):
        x, W1, s1, W2, b2 = (a.astype(np.float64) for a in cases.mlp_case(B, N, Cin, H, Cout, seed=50 + seed))
        y = host.mlp2_max(x, W1, s1, W2, b2)[1]
        top = np.sort(y, 1)
        if ghost.clear_of_kinks(x, W1, s1) and float(np.abs(ghost.hidden_pre(x, W1, s1)).min()) > 2e-5 \
                and float((top[:, -1] - top[:, -2]).min()) > 1e-4:
            return x, W1, s1, W2, b2
    raise AssertionError("no seed below 64 keeps the ReLU inputs and the pool margins clear of the difference step")


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_block_backward_agrees_with_central_differences(Cin, H, Cout):
    x, W1, s1, W2, b2 = _case(Cin, H, Cout)
    rng = np.random.default_rng(Cin)
    G, Gy = rng.uniform(-1, 1, (1, Cout)), rng.uniform(-0.1, 0.1, (1, 5, Cout))
    params = dict(x=x, W1=W1, shift1=s1, W2=W2, b2=b2)

    def loss():
        pooled, y = host.mlp2_max(params["x"], params["W1"], params["shift1"], params["W2"], params["b2"])
        return float((G * pooled).sum() + (Gy * y).sum())
    arg = host.mlp2_max(x, W1, s1, W2, b2)[1].argmax(1)
    g = ghost.mlp2_max_backward(x, W1, s1, W2, arg, G, Gy)
    grads = dict(x=g["gx"], W1=g["gW1"], shift1=g["gshift1"], W2=g["gW2"], b2=g["gb2"])
    worst = {step: 0.0 for step in BOUND}
    for name, count in (("x", 5), ("W1", 5), ("shift1", 5), ("W2", 5), ("b2", 4)):
        p = params[name]
        for flat in rng.choice(p.size, count, replace=False):
            i = np.unravel_index(flat, p.shape)
            keep = p[i]
            for step in BOUND:
                p[i] = keep + step
                up = loss()
                p[i] = keep - step
                down = loss()
                p[i] = keep
                worst[step] = max(worst[step], abs((up - down) / (2 * step) - grads[name][i]))
    print((Cin, H, Cout), "largest disagreement with the central quotient per step", worst)
    for step, bound in BOUND.items():
        assert worst[step] <= bound, (step, worst[step])


def test_float32_restatement_is_float32_and_close():
    x, W1, s1, W2, b2 = cases.mlp_case(2, 9, 3, 128, 256, seed=1)
    arg = host.mlp2_max(x, W1, s1, W2, b2)[1].argmax(1)
    G = np.random.default_rng(0).uniform(-1, 1, (2, 256)).astype(np.float32)
    a, b = ghost.mlp2_max_backward(x, W1, s1, W2, arg, G, dtype=np.float32), ghost.mlp2_max_backward(x, W1, s1, W2, arg, G)
    for k in a:
        assert a[k].dtype == np.float32 and np.abs(a[k] - b[k]).max() <= 1e-4 * max(1.0, np.abs(b[k]).max()), k


# ---------------------------------------------------------------------------------------------------- fold, encoder, whole model
# 10x the measured disagreement: fold 1.1e-9 at step 1e-6 and 4.0e-9 at 1e-7; whole model 4.1e-9 and 2.5e-8 (gradients of
# order 0.01 to 10; what remains is the quotient's own rounding, about eps * |L| / step)
FOLD_BOUND = {1e-6: 1.1e-8, 1e-7: 4e-8}
MODEL_BOUND = {1e-6: 4.2e-8, 1e-7: 2.5e-7}


def _quotients(loss, params, grads, picks, steps, rng):
    """Largest |central quotient - gradient| per step over `picks` seeded entries of every tensor in `params`."""
    worst = {step: 0.0 for step in steps}
    for name, p in params.items():
        for flat in rng.choice(p.size, min(picks, p.size), replace=False):
            i = np.unravel_index(flat, p.shape)
            keep = p[i]
            for step in steps:
                p[i] = keep + step
                up = loss()
                p[i] = keep - step
                down = loss()
                p[i] = keep
                worst[step] = max(worst[step], abs((up - down) / (2 * step) - grads[name][i]))
    return worst


def test_fold_backward_agrees_with_central_differences():
    """pcn_grad_host.fold_backward (the yardstick of houv_pcn_fold_backward) against central differences of pcn_host.fold_rows
    on L = <G, fine>: 3 seeded entries of each of coarse, cvec, Wgp, W2, b2, W3, b3 at steps 1e-6 and 1e-7.  B = 2, nc = 3,
    scale = 2; the first seed whose ReLU inputs all lie 2e-5 from zero.  Measured and bounded as stated at FOLD_BOUND."""
    for seed in range(64):
        case = [a.astype(np.float64) for a in cases.fold_case(2, 3, 2, seed=70 + seed)]
        G = np.random.default_rng(seed).uniform(-1, 1, (2, 6, 3))
        r = ghost.fold_backward(*case, G)
        if min(float(np.abs(r["pre1"]).min()), float(np.abs(r["pre2"]).min())) > 2e-5:
            break
    else:
        raise AssertionError("no seed below 64 keeps the fold's ReLU inputs clear of the difference step")
    names = ("gcoarse", "gcvec", None, "gWgp", "gW2", "gb2", "gW3", "gb3")
    params = {n: case[i] for i, n in enumerate(names) if n}
    worst = _quotients(lambda: float((host.fold_rows(*case) * G).sum()), params, r, 3, FOLD_BOUND, np.random.default_rng(7))
    print("fold: largest disagreement with the central quotient per step", worst)
    for step, bound in FOLD_BOUND.items():
        assert worst[step] <= bound, (step, worst[step])


def test_model_backward_agrees_with_central_differences():
    """pcn_grad_host.model_backward -- the un-split encoder_backward, the three linear layers, the coarse view / transpose and
    fold_cat_backward with the 1029-channel concatenation -- against central differences of pcn_host.model on
    L = <G1, out1> + <G2, out2>: one seeded entry of each of the 20 parameter tensors at steps 1e-6 and 1e-7.  B = 1, N = 5,
    num_points 8, num_coarse 4; the first cloud seed whose ReLU inputs all lie 2e-5 from zero and whose pools lead their
    runners-up by 1e-4.  Measured and bounded as stated at MODEL_BOUND."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import pcn_weights
    state = {k: v.astype(np.float64) for k, v in pcn_weights.make_state(4).items()}
    rng = np.random.default_rng(11)
    G1, G2 = rng.uniform(-1, 1, (1, 4, 3)), rng.uniform(-1, 1, (1, 8, 3))
    for seed in range(64):
        x = np.random.default_rng(seed).uniform(-0.5, 0.5, (1, 3, 5))
        r = ghost.model_backward(state, x, G1, G2, 8, 4)
        tops = [np.sort(a, 1) for a in r["pools"]]
        if min(float(np.abs(a).min()) for a in r["relu"]) > 2e-5 and min(float((t[:, -1] - t[:, -2]).min()) for t in tops) > 1e-4:
            break
    else:
        raise AssertionError("no cloud seed below 64 keeps the model clear of its kinks")

    def loss():
        f = host.model(state, x, 8, 4)
        return float((G1 * f["out1"]).sum() + (G2 * f["out2"]).sum())
    worst = _quotients(loss, state, r["grads"], 1, MODEL_BOUND, np.random.default_rng(13))
    print("model: largest disagreement with the central quotient per step", worst, "cloud seed", seed)
    for step, bound in MODEL_BOUND.items():
        assert worst[step] <= bound, (step, worst[step])


# ---------------------------------------------------------------------------------------------------- the reference's gradients
GRAD_CASES = {"b1n33p32c8": (32, 8), "b2n65p64c16": (64, 16)}


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_float32_restatement_vs_the_reference_autograd(name):
    """tests/golden/g28_pcn_grad.npz holds the gradients of L = <G1, out1> + <G2, out2> that the reference's own pcn.py gives
    under float32 autograd (make_golden_pcn_grad.py), on up to 2048 seeded entries of each of the 20 parameter tensors.  The
    float32 restatement is within 4x its own stored float32-vs-float64 spread of them, and the float64 restatement reproduces the
    stored float64 values: what the GPU tests measure the model against is the reference's gradient, not this repository's idea
    of it."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import pcn_weights
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_pcn_grad.npz"), allow_pickle=False)
    num_points, num_coarse = GRAD_CASES[name]
    state = pcn_weights.make_state(num_coarse)
    x, G1, G2 = g[f"{name}_x"], g[f"{name}_G1"], g[f"{name}_G2"]
    r32 = ghost.model_backward(state, x, G1, G2, num_points, num_coarse, np.float32)
    r64 = ghost.model_backward(state, x, G1, G2, num_points, num_coarse, np.float64)
    ok, margin = ghost.clear_margins(ghost.model_kinks(state, x, num_points, num_coarse, np.float64),
                                     ghost.model_kinks(state, x, num_points, num_coarse, np.float32))
    assert ok, margin                                                                 # the stored cloud is the chosen one
    for k in state:
        idx, ref, f64, spread = g[f"{name}_{k}_idx"], g[f"{name}_{k}_ref"], g[f"{name}_{k}_f64"], float(g[f"{name}_{k}_spread"])
        assert len(idx) == min(2048, state[k].size) and r32["grads"][k].dtype == np.float32
        own32, own64 = r32["grads"][k].reshape(-1)[idx], r64["grads"][k].reshape(-1)[idx]
        err = float(np.abs(own32.astype(np.float64) - ref).max())
        print(name, k, "float32 restatement vs the reference", err, "bound", 4 * spread)
        assert err <= 4 * spread, (name, k)
        assert np.abs(own64 - f64).max() <= 1e-12 * max(1.0, np.abs(f64).max()), (name, k)
