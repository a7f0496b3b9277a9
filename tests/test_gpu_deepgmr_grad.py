"""GPU: the DeepGMR training kernels -- houv_bn_rows_stats, houv_bn_relu_rows, houv_bn_relu_rows_backward,
houv_gmm_params_backward, houv_gmm_register_backward -- against the float64 restatements of tests/deepgmr_grad_host.py.  Inputs and
bounds come from tests/deepgmr_grad_cases.py: a bound is 4 x what the float32 restatement itself loses against float64 on the same
inputs, never a figure taken from the kernels.  Every kernel is called twice and must return the same bits."""
import numpy as np
import pytest
import torch

import deepgmr_grad_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _close(got, ref, bound, what):
    err = float(np.abs(_np(got).astype(np.float64) - ref).max())
    print(f"{what}: error {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{what}: error {err} > bound {bound}"


@pytest.mark.parametrize("R", cases.BN_ROWS)
def test_bn_rows_kernels_match_float64(dev, R):
    """Statistics, normalisation (+ ReLU, + group maxima) and backward at every column count and both row strides: ld = C + 4 takes
    the 16-byte path where C is a multiple of 4, ld = C + 1 the scalar path.  The padding columns of y and gz stay untouched."""
    from houv_amd import ops
    for C in cases.BN_COLS:
        for pad in cases.BN_PADS:
            c = cases.bn_case(R, C, pad)
            what = f"R={R} C={C} ld={c['ld']}"
            T = lambda a: torch.tensor(a, device=dev)
            zw, gyw = T(c["z"]), T(c["gy"])
            z, gy = zw[:, :C], gyw[:, :C]
            weight, bias, mean_in, var_in = T(c["weight"]), T(c["bias"]), T(c["mean_in"]), T(c["var_in"])
            ref, bounds, ng = c["ref"], c["bounds"], c["n_group"]

            mean, var = ops.bn_rows_stats(z)
            mean2, var2 = ops.bn_rows_stats(z)
            assert torch.equal(mean, mean2) and torch.equal(var, var2)
            _close(mean, ref["mean"], bounds["mean"], what + " mean")
            _close(var, ref["var"], bounds["var"], what + " var")

            y, gmax, garg = ops.bn_relu_rows(z, mean_in, var_in, weight, bias, cases.BN_EPS, True, ng)
            y2, gmax2, garg2 = ops.bn_relu_rows(z, mean_in, var_in, weight, bias, cases.BN_EPS, True, ng)
            assert torch.equal(y, y2) and torch.equal(gmax, gmax2) and torch.equal(garg, garg2)
            _close(y, ref["y"], bounds["y"], what + " y")
            _close(gmax, ref["gmax"], bounds["y"], what + " gmax")
            lin = ops.bn_relu_rows(z, mean_in, var_in, weight, bias, cases.BN_EPS, False)
            _close(lin, ref["lin"], bounds["lin"], what + " y without ReLU")
            # garg: the LOWEST row of the group whose y equals the group's maximum, judged on the kernel's own y, bit for bit
            yn, an = _np(y).reshape(R // ng, ng, C), _np(garg)
            first = yn.argmax(1) + np.arange(R // ng)[:, None] * ng
            assert np.array_equal(_np(gmax), yn.max(1)) and np.array_equal(an, first), what + " garg"
            # and the reference's row wherever its maximum stands clear of every other distinct value by more than the bound
            y64 = ref["y"].reshape(R // ng, ng, C)
            runner_up = np.where(y64 < y64.max(1, keepdims=True), y64, -np.inf).max(1)
            clear = y64.max(1) - runner_up > 2 * bounds["y"]
            assert np.array_equal(an[clear], ref["garg"][clear]), what + " garg against float64"

            out = torch.full_like(gyw, float(c["pad_fill"]))
            out[:, :C] = gy
            gz, gweight, gbias = ops.bn_relu_rows_backward(gy, z, mean_in, var_in, weight, bias, cases.BN_EPS, True)
            gz2, gweight2, gbias2 = ops.bn_relu_rows_backward(out[:, :C], z, mean_in, var_in, weight, bias, cases.BN_EPS, True,
                                                              inplace=True)          # gz written over gy, in a strided buffer
            assert torch.equal(gz, gz2) and torch.equal(gweight, gweight2) and torch.equal(gbias, gbias2)
            assert gz2.data_ptr() == out.data_ptr() and bool((out[:, C:] == float(c["pad_fill"])).all()), what + " padding"
            _close(gz, ref["gz"], bounds["gz"], what + " gz")
            _close(gweight, ref["gweight"], bounds["gweight"], what + " gweight")
            _close(gbias, ref["gbias"], bounds["gbias"], what + " gbias")
            if c["masked_column"] is not None:
                m, k = c["masked_column"], c["constant_column"]
                assert not _np(y)[:, m].any() and not _np(gz)[:, m].any() and _np(gweight)[m] == 0 and _np(gbias)[m] == 0
                assert _np(var)[k] == 0 and np.array_equal(_np(y)[:, k], np.full(R, c["bias"][k]))
    torch.cuda.synchronize()


def test_bn_rows_refuses_bad_arguments(dev):
    from houv_amd import _lib, ops
    z = torch.zeros((8, 16), device=dev)
    v = torch.ones(16, device=dev)
    with pytest.raises(_lib.HouvHipError):
        ops.bn_relu_rows(z, v, v, v, v, 1e-5, True, 3)                       # 3 does not divide 8
    with pytest.raises(_lib.HouvHipError):
        ops.bn_rows_stats(z[:1])                                             # one row has no batch statistics
    with pytest.raises(_lib.HouvHipError):
        ops.bn_relu_rows(z, v[:8], v, v, v)
    with pytest.raises(_lib.HouvHipError):
        ops.bn_rows_stats(z.t())                                             # columns must be contiguous
    lib = _lib.load()
    ws = torch.zeros(64, device=dev)
    assert lib.houv_bn_rows_stats(_lib.ptr(z), 8, 16, 16, _lib.ptr(v), _lib.ptr(v), _lib.ptr(ws), 16, _lib.stream_of(z)) == 0
    assert "workspace" in _lib.last_error()
    assert lib.houv_bn_rows_stats(_lib.ptr(z), 8, 16, 8, _lib.ptr(v), _lib.ptr(v), _lib.ptr(ws), 256, _lib.stream_of(z)) == 0
    assert "ld" in _lib.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,N,J", cases.PARAMS_SHAPES)
def test_gmm_params_backward_matches_float64(dev, B, N, J):
    from houv_amd import ops
    c = cases.params_case(B, N, J)
    args = [torch.tensor(a, device=dev) for a in c["args"]]
    g = ops.gmm_params_backward(*args)
    assert torch.equal(g, ops.gmm_params_backward(*args))
    assert tuple(g.shape) == (B, N, J)
    _close(g, c["ref"], c["bound"], f"g_logits B={B} N={N} J={J}")
    # softmax backward: the gradient of every point sums to zero over the components, up to the rounding of J terms
    assert float(g.sum(2).abs().max()) <= 1e-5 * max(1.0, float(g.abs().max()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,J", cases.REGISTER_SHAPES)
def test_gmm_register_backward_matches_float64(dev, B, J):
    """Pairs with det(V U^T) < 0 included (every third); min (lam_i + lam_j) >= REGISTER_GAP is asserted by the generator."""
    from houv_amd import ops
    c = cases.register_case(B, J)
    assert c["gap"] >= cases.REGISTER_GAP and c["negative"] >= 1
    args = [torch.tensor(c[k], device=dev) for k in ("pi_s", "mu_s", "mu_t", "sigma_t", "g_T")]
    outs = ops.gmm_register_backward(*args)
    again = ops.gmm_register_backward(*args)
    for name, got, twice, ref, bound in zip(("g_pi_s", "g_mu_s", "g_mu_t", "g_sigma_t"), outs, again, c["ref"], c["bounds"]):
        assert torch.equal(got, twice)
        _close(got, ref, bound, f"{name} B={B} J={J}")
    torch.cuda.synchronize()


def test_torch_ops_are_registered(dev):
    from houv_amd import ops
    ops.register_torch_ops()
    c = cases.bn_case(65, 16)
    z = torch.tensor(c["z"], device=dev)[:, :16]
    mean, var = torch.ops.houv.bn_rows_stats(z)
    assert torch.equal(mean, ops.bn_rows_stats(z)[0]) and torch.equal(var, ops.bn_rows_stats(z)[1])
    p = cases.params_case(2, 33, 16)
    args = [torch.tensor(a, device=dev) for a in p["args"]]
    assert torch.equal(torch.ops.houv.gmm_params_backward(*args), ops.gmm_params_backward(*args))
    torch.cuda.synchronize()
