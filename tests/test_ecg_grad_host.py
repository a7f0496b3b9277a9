"""CPU: the NumPy Dense_conv backward of tests/ecg_grad_host.py (the yardstick of houv_dense_conv_backward; DESIGN.md section
9.13) against central differences of L = <gout, out> in float64, its forward against ecg_host.dense_conv, and its conventions
(the clamped neighbour row, arg = -1, the pass-through columns)."""
import numpy as np
import pytest

import ecg_grad_host as gh
import ecg_host as host

NAMES = ("x", "W0", "b0", "W1", "b1", "W2", "b2")


@pytest.mark.parametrize("C,N,k,relu_out", [(24, 9, 4, False), (48, 7, 5, True), (24, 5, 1, True)])
def test_backward_matches_central_differences(C, N, k, relu_out):
    c = gh.random_case(11, 2, N, C, k, margin=1e-4)
    c["idx"][0, 0, :] = [-3, N + 5, 0, 1, 2][:k]                              # out of range: clamped to rows 0 and N - 1
    res = gh.dense_conv_backward(**c, relu_out=relu_out)
    assert min(np.abs(res["z0"]).min(), np.abs(res["z1"]).min()) >= 1e-5
    # exact ties of the pooling (a repeated neighbour, several edges at relu's 0) carry the same derivative whoever wins
    rng = np.random.default_rng(5)
    h = 1e-6
    for n, g in zip(NAMES, gh.GRADS):
        for _ in range(3):
            v = rng.standard_normal(c[n].shape)
            hi, lo = dict(c), dict(c)
            hi[n] = c[n].astype(np.float64) + h * v
            lo[n] = c[n].astype(np.float64) - h * v
            fd = (gh.loss(**hi, relu_out=relu_out) - gh.loss(**lo, relu_out=relu_out)) / (2 * h)
            an = float((res[g] * v).sum())
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (n, fd, an)


@pytest.mark.parametrize("C", [24, 48])
def test_forward_equals_ecg_host_dense_conv(C):
    c = gh.random_case(3, 2, 17, C, 6)
    res = gh.dense_conv_backward(**c)
    w = {n: c[n] for n in ("W0", "b0", "W1", "b1", "W2", "b2")}
    want = host.dense_conv(np.swapaxes(c["x"], 1, 2), c["idx"].astype(np.int64), **w)
    assert np.abs(res["out"] - np.swapaxes(want, 1, 2)).max() <= 1e-12
    for dt in (np.float32, np.float64):
        r = gh.dense_conv_backward(**c, dtype=dt)
        assert all(r[g].dtype == dt for g in gh.GRADS)


def test_injected_arg_minus_one_sends_no_gradient_and_zero_gout_gives_zeros():
    c = gh.random_case(4, 1, 6, 24, 3)
    arg = gh.dense_conv_backward(**c)["arg"]
    off = np.full_like(arg, -1)
    r = gh.dense_conv_backward(**c, arg=off)
    assert np.array_equal(r["gx"], c["gout"][..., gh.G:gh.G + 24].astype(np.float64))     # the pass-through columns alone
    assert all(not r[g].any() for g in gh.GRADS[1:])
    c["gout"][:] = 0
    r = gh.dense_conv_backward(**c, arg=arg)
    assert all(not r[g].any() for g in gh.GRADS)


@pytest.mark.parametrize("name", [f"c{C}n{N}r{r}" for C in (24, 48) for N in (17, 33) for r in (0, 1)])
def test_fixture_a_is_consistent_with_the_restatement(golden, name):
    """g29_ecg_grad.npz (a): the stored float64 gradients are the restatement's under the stored lists, the reference's float32
    gradients lie within 4x the stored spread of them, and the chosen input is clear of its kinks by the stored margin."""
    g = golden("g29_ecg_grad.npz")
    shape, relu_out = name[:-2], bool(int(name[-1]))
    w = {n: g[f"{shape}_{n}"] for n in ("W0", "b0", "W1", "b1", "W2", "b2")}
    rows = np.ascontiguousarray(np.swapaxes(g[f"{name}_x"], 1, 2))
    gout = np.ascontiguousarray(np.swapaxes(g[f"{name}_G"], 1, 2))
    assert g[f"{name}_idx"].shape == rows.shape[:2] + (16,) and g[f"{name}_margin"][0] >= g[f"{name}_margin"][1] > 0
    r64 = gh.dense_conv_backward(rows, g[f"{name}_idx"], **w, gout=gout, relu_out=relu_out)
    for n in gh.GRADS:
        a64 = np.swapaxes(r64[n], 1, 2) if n == "gx" else r64[n]
        assert np.abs(a64 - g[f"{name}_f64_{n}"]).max() <= 1e-12 * max(1.0, np.abs(a64).max()), n
        assert g[f"{name}_ref_{n}"].dtype == np.float32 and g[f"{name}_spread_{n}"] > 0
        assert np.abs(g[f"{name}_ref_{n}"] - a64).max() <= 4 * float(g[f"{name}_spread_{n}"]), n


def test_torch_restatement_forward_equals_ecg_host_model(golden):
    """ecg_grad_host.torch_model in float64 against ecg_host.model under the same (the reference's) decisions, to round-off; and
    fixture (c) holds one positive relative error per parameter."""
    import torch

    import ecg_cases as cases
    g26, g29 = golden("g26_ecg.npz"), golden("g29_ecg_grad.npz")
    name = "p512"
    num_points, num_coarse, _ = cases.GOLDEN_CASES[name]
    state = cases.state(name)
    dec = {n: g26[f"{name}_{n}"] for n in host.DECISIONS if f"{name}_{n}" in g26.files}
    want = host.model(state, g26[f"{name}_x"], num_points, num_coarse, np.float64, dec)[0]
    got = gh.torch_model({n: torch.tensor(v, dtype=torch.float64) for n, v in state.items()}, g26[f"{name}_x"], num_points, num_coarse, dec)
    for n in want:
        assert np.abs(got[n].numpy() - want[n]).max() <= 1e-11, n
    assert sorted(k[len(name) + 5:] for k in g29.files if k.startswith(name + "_rel_")) == sorted(state)
    assert all(0 < float(g29[f"{name}_rel_{n}"]) < 1e-2 for n in state)


def test_fixture_b_is_consistent_with_the_restatement(golden):
    """g29_ecg_grad_b.npz: the stored float64 entries are the torch restatement's under the stored (the reference's) decisions, the
    reference's float32 gradients lie within 4x the stored spread of them, every parameter of the encoder is present with at most
    2048 entries, and the input cleared its margins."""
    import torch
    from ecg_cases import ecg_weights
    g = golden("g29_ecg_grad_b.npz")
    state = {n[len("decoder.encoder."):]: v for n, v in ecg_weights.make_state(512, 1).items() if n.startswith("decoder.encoder.")}
    dec = {n: g[n] for n in g.files if n.startswith(("fps", "knn_", "three_nn"))}
    assert len(dec) == 13 and g["x"].shape == (2, 3, 48) and float(g["margin"][0]) >= 1
    assert [dec[f"fps{i}"].shape[1] for i in (1, 2, 3)] == [32, 24, 16] and dec["knn_feat1"].shape == (2, 48, 16)
    _, g64 = gh.torch_encoder_grads(state, g["x"], dec, g["G"], torch.float64)
    assert sorted(g64) == sorted(k[4:] for k in g.files if k.startswith("idx_"))
    for n in g64:
        idx = g[f"idx_{n}"]
        assert len(idx) == min(2048, g64[n].size) and len(np.unique(idx)) == len(idx)
        a64 = g64[n].reshape(-1)[idx]
        assert np.abs(a64 - g[f"f64_{n}"]).max() <= 1e-11 * max(1.0, np.abs(a64).max()), n
        assert g[f"ref_{n}"].dtype == np.float32 and np.abs(g[f"ref_{n}"] - a64).max() <= 4 * float(g[f"spread_{n}"]), n
