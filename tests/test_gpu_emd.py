"""GPU: the auction EMD kernels (houv_emd_forward / houv_emd_backward) against the host restatement tests/emd_host.py, BIT FOR
BIT -- dist, assignment and the iterations run -- on both sides of the 4096-point boundary between the in-LDS and the
streamed kernel, with ties forced by duplicated and grid-quantised points."""
import numpy as np
import pytest
import torch

import emd_host

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _clouds(B, N, seed, kind="rand"):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand((B, N, 3), generator=g)
    x2 = torch.rand((B, N, 3), generator=g)
    if kind == "grid":                              # coarse grid: equal distances, equal values and equal increments
        x1 = torch.round(x1 * 4) / 4
        x2 = torch.round(x2 * 4) / 4
    elif kind == "dup":                             # duplicated targets: equal values for distinct objects
        x2[:, 1::2] = x2[:, 0:N - 1:2] if N > 1 else x2[:, 1::2]
    return x1, x2


def _check(x1, x2, eps, iters):
    from houv_amd import ops
    dist, assign, run = ops.emd_forward(x1.to(DEV), x2.to(DEV), eps, iters)
    hd, ha, hr = emd_host.emd(x1.numpy(), x2.numpy(), eps, iters)
    np.testing.assert_array_equal(run.cpu().numpy(), hr)
    np.testing.assert_array_equal(assign.cpu().numpy(), ha)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), hd.view(np.uint32))
    return dist, assign, run


CASES = []
for n_i, N in enumerate([1, 2, 63, 64, 257, 1000, 2048, 4096]):
    for k_i, iters in enumerate([1, 2, 7, 50]):
        CASES.append((N, iters, (0.005, 0.05)[(n_i + k_i) % 2], 2 + (n_i + k_i) % 3 if N < 2048 else 2,
                      ("rand", "grid", "dup")[(n_i + 2 * k_i) % 3]))


@pytest.mark.parametrize("N,iters,eps,B,kind", CASES)
def test_emd_bit_equal_in_lds(N, iters, eps, B, kind):
    x1, x2 = _clouds(B, N, seed=N * 100 + iters, kind=kind)
    _check(x1, x2, eps, iters)


@pytest.mark.parametrize("N,iters,kind", [(4097, 1, "rand"), (4097, 3, "grid"), (8192, 2, "dup"), (8192, 3, "rand")])
def test_emd_bit_equal_streamed(N, iters, kind):
    from houv_amd import _lib
    assert _lib.load().houv_emd_workspace_bytes(1, N) > 0 and _lib.load().houv_emd_workspace_bytes(1, 4096) == 0
    x1, x2 = _clouds(1, N, seed=N + iters, kind=kind)
    _check(x1, x2, 0.05, iters)


def test_emd_early_exit():
    x1, x2 = _clouds(3, 256, seed=11)
    _, _, run = _check(x1, x2, 0.005, 100000)
    assert (run.cpu() < 100000).all()


def test_emd_deterministic_and_stream():
    from houv_amd import ops
    x1, x2 = _clouds(4, 2048, seed=12, kind="grid")
    x1, x2 = x1.to(DEV), x2.to(DEV)
    a = ops.emd_forward(x1, x2, 0.005, 50)
    b = ops.emd_forward(x1, x2, 0.005, 50)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = ops.emd_forward(x1, x2, 0.005, 50)
    torch.cuda.current_stream().wait_stream(s)
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)


def test_emd_autograd_and_torch_ops():
    from houv_amd import ops
    from houv_amd.metrics import emd
    x1, x2 = _clouds(3, 500, seed=13)
    x1 = x1.to(DEV).requires_grad_(True)
    x2 = x2.to(DEV).requires_grad_(True)
    dist, assign = emd()(x1, x2, 0.01, 30)
    assert not assign.requires_grad
    g = torch.rand_like(dist)
    (dist * g).sum().backward()
    y = torch.gather(x2.detach(), 1, assign.long().unsqueeze(-1).expand(-1, -1, 3))
    assert torch.equal(x1.grad, (2 * g).unsqueeze(-1) * (x1.detach() - y))
    assert torch.equal(x2.grad, torch.zeros_like(x2))
    ops.register_torch_ops()
    d2, a2, r2 = torch.ops.houv.emd_forward(x1.detach(), x2.detach(), 0.01, 30)
    assert torch.equal(d2, dist.detach()) and torch.equal(a2, assign)
    gr = torch.ops.houv.emd_backward(x1.detach(), x2.detach(), g, assign)
    assert torch.equal(gr, x1.grad)


def test_calc_emd_and_input_forms():
    from houv_amd.metrics import emd
    from houv_amd.model_utils_completion import calc_emd
    x1, x2 = _clouds(2, 300, seed=14)
    x1, x2 = x1.to(DEV), x2.to(DEV)
    dist, _ = emd()(x1, x2, 0.005, 50)
    assert torch.equal(calc_emd(x1, x2), torch.sqrt(dist).mean(1))
    # fp64 and non-contiguous inputs: converted to contiguous fp32, same result
    d64, a64 = emd()(x1.double(), x2.double(), 0.005, 50)
    assert torch.equal(d64, dist)
    t1 = x1.transpose(1, 2).contiguous().transpose(1, 2)
    t2 = x2.transpose(1, 2).contiguous().transpose(1, 2)
    assert not t1.is_contiguous()
    dn, an = emd()(t1, t2, 0.005, 50)
    assert torch.equal(dn, dist) and torch.equal(an, a64)


def test_emd_errors():
    from houv_amd import _lib, ops
    x = torch.rand((2, 64, 3), device=DEV)
    for args, what in [((x, torch.rand((2, 65, 3), device=DEV), 0.01, 5), "N=64 M=65"),
                       ((x, x, 0.01, 0), "iters=0"), ((x, x, 0.0, 5), "eps=0"), ((x, x, -1.0, 5), "eps=-1")]:
        with pytest.raises(_lib.HouvHipError):
            ops.emd_forward(*args)
        assert what in _lib.last_error()
    big = torch.rand((1, 16385, 3), device=DEV)
    with pytest.raises(_lib.HouvHipError):
        ops.emd_forward(big, big, 0.01, 1)
    assert "N=16385" in _lib.last_error()
    with pytest.raises(_lib.HouvHipError):
        ops.emd_forward(x.cpu(), x.cpu(), 0.01, 5)
