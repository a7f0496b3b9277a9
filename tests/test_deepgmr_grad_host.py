"""CPU: the restatements of the DeepGMR training kernels (tests/deepgmr_grad_host.py) against the golden gradients of the
reference's training step (tests/golden/g2x_deepgmr_grad.npz, made by tests/golden/make_golden_deepgmr_grad.py), the closed-form
register backward against float64 autograd of the reference's formula, the test-case generators' own preconditions, and the C
ABI of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import deepgmr_grad_cases as cases
import deepgmr_grad_host as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20


@pytest.fixture(scope="module")
def steps(golden):
    """The restated training step at both fixture shapes in both precisions, computed once."""
    g = golden("g2x_deepgmr_grad.npz")
    return {(name, dt): cases.restated_step(g, name, dt) for name in cases.FIXTURE_CASES for dt in (np.float64, np.float32)}


@pytest.mark.parametrize("name", cases.FIXTURE_CASES)
def test_restated_step_in_float64_reproduces_the_golden_gradients(golden, steps, name):
    """All 23 gradients, the loss, the max-pool rows and the BatchNorm buffers of the reference's float64 step.  The golden values
    are stored rounded to float32 (2^-24 relative), the only slack given."""
    g, r = golden("g2x_deepgmr_grad.npz"), steps[(name, np.float64)]
    assert abs(r["loss"] - float(g[f"{name}_loss_f64"])) <= 1e-12
    assert np.array_equal(r["pool1"], g[f"{name}_pool1"]) and np.array_equal(r["pool2"], g[f"{name}_pool2"])
    names = [str(k) for k in g["param_names"]]
    assert len(names) == 23 and sorted(r["grads"]) == names
    for k in names:
        got, ref, scale = cases.against_golden(g, name, k, r["grads"][k])
        assert np.abs(got - ref).max() <= 2.0 ** -23 * scale + 1e-12, k
        if f"{name}_gradsum_{k}" in g.files:
            full = r["grads"][k]
            np.testing.assert_allclose([full.sum(), (full * full).sum()], g[f"{name}_gradsum_{k}"], rtol=1e-9, atol=1e-12)
    for key, want in cases.golden_buffers(g, name).items():
        np.testing.assert_allclose(cases.buffers_after(r["stats"])[key], want, rtol=1e-11, atol=1e-12, err_msg=key)


@pytest.mark.parametrize("name", cases.FIXTURE_CASES)
def test_restated_step_in_float32_stays_within_the_gradient_tolerance(golden, steps, name):
    """The float32 restatement -- what the formulas themselves lose in fp32 -- under the tolerance the GPU test applies: 8 x the
    recorded fp32-vs-fp64 spread of each parameter."""
    g, r = golden("g2x_deepgmr_grad.npz"), steps[(name, np.float32)]
    worst = 0.0
    for k in (str(k) for k in g["param_names"]):
        got, ref, scale = cases.against_golden(g, name, k, r["grads"][k])
        ratio = np.abs(got - ref).max() / (float(g[f"{name}_spread_{k}"]) * scale)
        worst = max(worst, ratio)
        assert ratio <= cases.GRAD_SPREADS, (k, ratio)
    print(name, "worst error of the float32 restatement, in spreads:", worst)
    assert float(g["worst_spread"]) < 1e-4


def _reference_register(pi_s, mu_s, mu_t, sigma):
    """gmm_register of registration/models/deepgmr.py:123-143 on float64 tensors (sigma the scalar of sigma * eye(3))."""
    c_s = pi_s.unsqueeze(1) @ mu_s
    c_t = pi_s.unsqueeze(1) @ mu_t
    Ms = torch.sum((pi_s.unsqueeze(2) * (mu_s - c_s)).unsqueeze(3) @ (mu_t - c_t).unsqueeze(2) / sigma[:, :, None, None], dim=1)
    U, _, Vh = torch.linalg.svd(Ms)
    V = Vh.transpose(1, 2)
    S = torch.eye(3, dtype=Ms.dtype).unsqueeze(0).repeat(U.shape[0], 1, 1)
    S[:, 2, 2] = torch.det(V @ U.transpose(1, 2))
    R = V @ S @ U.transpose(1, 2)
    t = c_t.transpose(1, 2) - R @ c_s.transpose(1, 2)
    bot = torch.tensor([[[0, 0, 0, 1]]], dtype=Ms.dtype).repeat(R.shape[0], 1, 1)
    return torch.cat([torch.cat([R, t], dim=2), bot], dim=1), S[:, 2, 2]


@pytest.mark.parametrize("B,J", cases.REGISTER_SHAPES)
def test_closed_form_register_backward_equals_float64_autograd(B, J):
    """The polar form against autograd through torch.linalg.svd, on the GPU test's own cases: both signs of det(V U^T) occur."""
    c = cases.register_case(B, J)
    leaves = [torch.tensor(c[k].astype(np.float64), requires_grad=True) for k in ("pi_s", "mu_s", "mu_t", "sigma_t")]
    T, det = _reference_register(*leaves)
    (T * torch.tensor(c["g_T"].astype(np.float64))).sum().backward()
    assert (det < 0).any() and ((det > 0).any() or B == 1)
    mine = host.gmm_register_backward(c["pi_s"], c["mu_s"], c["mu_t"], c["sigma_t"], c["g_T"], np.float64)
    for got, leaf in zip(mine, leaves):
        ref = leaf.grad.numpy()
        assert np.abs(got - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max())


def test_restatements_equal_torch_autograd():
    """BatchNorm rows (forward, group maxima, backward) against nn.BatchNorm1d in train mode, and the GMM parameters' backward
    against autograd of the reference's gmm_params behind a softmax, in float64."""
    rng = np.random.default_rng(5)
    R, C, NG = 300, 7, 100
    z = torch.tensor(rng.standard_normal((R, C)) * 2 + 3, requires_grad=True)
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor(rng.uniform(0.5, 1.5, C)))
        bn.bias.copy_(torch.tensor(rng.normal(0, 0.2, C)))
    y = torch.relu(bn(z))
    gy = rng.standard_normal((R, C))
    (y * torch.tensor(gy)).sum().backward()
    w, b, zz = bn.weight.detach().numpy(), bn.bias.detach().numpy(), z.detach().numpy()
    mean, var = host.bn_rows_stats(zz)
    np.testing.assert_allclose(mean, zz.mean(0), atol=1e-13)
    np.testing.assert_allclose(var, zz.var(0), atol=1e-13)
    np.testing.assert_allclose(bn.running_var.numpy(), 0.9 + 0.1 * var * R / (R - 1), atol=1e-13)
    yy, gmax, garg = host.bn_relu_rows(zz, mean, var, w, b, n_group=NG)
    np.testing.assert_allclose(yy, y.detach().numpy(), atol=1e-13)
    assert np.array_equal(gmax, yy.reshape(R // NG, NG, C).max(1)) and np.array_equal(yy[garg, np.arange(C)], gmax)
    gz, gw, gb = host.bn_relu_rows_backward(gy, zz, mean, var, w, b)
    np.testing.assert_allclose(gz, z.grad.numpy(), atol=1e-13)
    np.testing.assert_allclose(gw, bn.weight.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(gb, bn.bias.grad.numpy(), atol=1e-12)

    B, N, J = 2, 33, 5
    logits = torch.tensor(rng.standard_normal((B, N, J)), requires_grad=True)
    pts = torch.tensor(rng.standard_normal((B, N, 3)))
    gamma = torch.softmax(logits, 2)
    pi = gamma.mean(1)
    npi = pi * N
    mu = gamma.transpose(1, 2) @ pts / npi.unsqueeze(2)
    diff = pts.unsqueeze(2) - mu.unsqueeze(1)
    sigma = ((diff * diff).sum(-1) * gamma).sum(1) / npi
    gp, gm, gs = rng.standard_normal((B, J)), rng.standard_normal((B, J, 3)), rng.standard_normal((B, J))
    ((pi * torch.tensor(gp)).sum() + (mu * torch.tensor(gm)).sum() + (sigma * torch.tensor(gs)).sum()).backward()
    mine = host.gmm_params_backward(gamma.detach().numpy(), pts.numpy(), pi.detach().numpy(), mu.detach().numpy(),
                                    sigma.detach().numpy(), gp, gm, gs)
    np.testing.assert_allclose(mine, logits.grad.numpy(), atol=1e-13)


def test_case_generators_meet_their_preconditions():
    """What the GPU tests' inputs promise: a gap under every lam_i + lam_j of the register cases with both determinant signs
    present, no normalised value next to the ReLU's kink in the BatchNorm cases, and positive kernel bounds."""
    for B, J in cases.REGISTER_SHAPES:
        c = cases.register_case(B, J)
        assert c["gap"] >= cases.REGISTER_GAP and c["negative"] >= 1
    for R, C in ((65, 16), (cases.CHUNK + 1, 100)):
        c = cases.bn_case(R, C)
        assert c["kink"] >= cases.BN_KINK
        assert all(v > 0 for v in c["bounds"].values())
    c = cases.bn_case(2 * cases.CHUNK + 3, 64)
    assert np.all(c["ref"]["var"][c["constant_column"]] == 0) and np.all(c["ref"]["y"][:, c["masked_column"]] == 0)


_PROTOS = {
    "houv_gmm_params_backward": (ctypes.c_int, 13),
    "houv_gmm_register_backward": (ctypes.c_int, 12),
    "houv_bn_rows_workspace_bytes": (ctypes.c_longlong, 3),
    "houv_bn_rows_stats": (ctypes.c_int, 9),
    "houv_bn_relu_rows": (ctypes.c_int, 18),
    "houv_bn_relu_rows_backward": (ctypes.c_int, 19),
}


@pytest.mark.parametrize("name", sorted(_PROTOS))
def test_training_entry_points_are_declared_exported_and_bound(name):
    from houv_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    restype, nargs = _PROTOS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "houv_hip.h")).read(), flags=re.S)
    m = re.search(r"\b(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m and len(m.group(2).split(",")) == nargs
    assert name in _lib.exported_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    fn = getattr(_lib.load(), name)
    assert fn.restype is restype and len(fn.argtypes) == nargs
    assert _lib.load().houv_abi_version() == _lib.ABI_VERSION == 2          # additive: the ABI version stays
    for op in ("gmm_params_backward", "gmm_register_backward", "bn_rows_stats", "bn_relu_rows", "bn_relu_rows_backward"):
        assert callable(getattr(ops, op))


def test_workspace_size_follows_the_documented_partition():
    from houv_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    f = _lib.load().houv_bn_rows_workspace_bytes
    assert f(cases.CHUNK, 64, 0) == 2 * 64 * 4 and f(cases.CHUNK + 1, 64, 0) == 2 * 2 * 64 * 4
    assert f(300, 5, 150) == 2 * 2 * 2 * 5 * 4                               # 2 groups x 2 splits x (max, arg)
    assert f(6, 3, 2) == ((2 * 3 * 3 * 4 + 15) // 16) * 16                   # 3 groups of one split each outweigh the one chunk
    assert f(0, 64, 0) == 0 and f(64, 0, 0) == 0 and f(64, 64, -1) == 0


def test_trainable_model_refuses_the_tnet_and_keeps_the_reference_names(golden):
    from argparse import Namespace
    from houv_amd.models.deepgmr import Model
    with pytest.raises(NotImplementedError):
        Model(Namespace(use_rri=False, rri_size=20, num_groups=16, use_tnet=True), trainable=True)
    net = Model(Namespace(use_rri=True, rri_size=20, num_groups=16, use_tnet=False), trainable=True)
    assert sorted(net.state_dict()) == [str(k) for k in golden("g2x_deepgmr_grad.npz")["state_keys"]]
    assert len(list(net.parameters())) == 23
