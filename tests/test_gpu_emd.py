"""GPU: the auction EMD kernels (houv_emd_forward / houv_emd_backward) against the host restatement tests/emd_host.py, BIT FOR
BIT -- dist, assignment and the iterations run -- on both sides of the 4096-point boundary between the in-LDS and the
streamed kernel, with ties forced by duplicated and grid-quantised points, on every branch of the bid phase (the case tables
of tests/emd_cases.py; tests/test_emd_host.py shows on the CPU that they reach all of them), with batches whose clouds stop
at different iterations, at the largest cloud, under the workspace contract, and the backward kernel value for value."""
import numpy as np
import pytest
import torch

import emd_cases
import emd_host
from emd_cases import clouds as _clouds

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _check(x1, x2, eps, iters):
    from houv_amd import ops
    dist, assign, run = ops.emd_forward(x1.to(DEV), x2.to(DEV), eps, iters)
    hd, ha, hr = emd_host.emd(x1.numpy(), x2.numpy(), eps, iters)
    np.testing.assert_array_equal(run.cpu().numpy(), hr)
    np.testing.assert_array_equal(assign.cpu().numpy(), ha)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), hd.view(np.uint32))
    return dist, assign, run


CASES = emd_cases.LDS_CASES


@pytest.mark.parametrize("N,iters,eps,B,kind", CASES)
def test_emd_bit_equal_in_lds(N, iters, eps, B, kind):
    x1, x2 = emd_cases.lds_clouds((N, iters, eps, B, kind))
    _check(x1, x2, eps, iters)


@pytest.mark.parametrize("N,iters,kind", [(c[0], c[1], c[4]) for c in emd_cases.STREAM_CASES_OLD])
def test_emd_bit_equal_streamed(N, iters, kind):
    from houv_amd import _lib
    assert _lib.load().houv_emd_workspace_bytes(1, N) > 0 and _lib.load().houv_emd_workspace_bytes(1, 4096) == 0
    x1, x2 = emd_cases.stream_clouds((N, iters, 0.05, 1, kind))
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


# ---------------------------------------------------------------------------------------------------
# Streamed kernel: every bid branch, batches, the maximum size, the workspace contract
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,iters,eps,kind", [(c[0], c[1], c[2], c[4]) for c in emd_cases.STREAM_CASES_NEW])
def test_emd_bit_equal_streamed_every_branch(N, iters, eps, kind):
    x1, x2 = emd_cases.stream_clouds((N, iters, eps, 1, kind))
    _, _, run = _check(x1, x2, eps, iters)
    if (N, iters, eps, 1, kind) == emd_cases.STREAM_COMPLETE:
        assert int(run[0]) < iters                              # the early exit: cnt == 0


def _bits(out):
    dist, assign, run = out
    return dist.cpu().numpy().view(np.uint32), assign.cpu().numpy(), run.cpu().numpy()


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(_bits(a), _bits(b)))


def test_emd_streamed_batch_mixed_iterations():
    from houv_amd import _lib, ops
    N, iters, eps = emd_cases.BATCH_N, emd_cases.BATCH_ITERS, emd_cases.BATCH_EPS
    x1, x2 = emd_cases.batch_clouds()
    _, _, run = _check(x1, x2, eps, iters)
    run = run.cpu().tolist()
    assert run[0] == 1 and run[2] == iters and 1 < run[1] < iters
    # each cloud uses only its own slice of the workspace: 20 * emd_stride(N) bytes, five arrays of emd_stride(N) words of
    # which the kernel uses the first N -- the pad word of every array keeps the fill, the third array holds the assignment
    stride = (N + 3) & ~3
    need = _lib.load().houv_emd_workspace_bytes(3, N)
    assert need == 3 * 20 * stride and stride != N
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    fwd = ops.emd_forward(x1.to(DEV), x2.to(DEV), eps, iters, workspace=ws)
    words = ws.cpu().numpy().view(np.int32).reshape(3, 5, stride)
    assert (words[:, :, N:] == -1).all()
    assert np.array_equal(words[:, 2, :N], fwd[1].cpu().numpy())
    # the same clouds in reverse order: the reversed outputs
    r1, r2 = emd_cases.batch_clouds(order=(2, 1, 0))
    rev = ops.emd_forward(r1.to(DEV), r2.to(DEV), eps, iters)
    assert _same(tuple(t.flip(0) for t in rev), fwd)


def test_emd_maximum_size():
    from houv_amd import _lib
    N, iters, eps, B, kind = emd_cases.STREAM_MAX
    assert N == 16384 and _lib.load().houv_emd_workspace_bytes(1, 16384) == 20 * 16384
    assert _lib.load().houv_emd_workspace_bytes(1, 16385) == 0
    x1, x2 = emd_cases.stream_clouds(emd_cases.STREAM_MAX)
    _, assign, _ = _check(x1, x2, eps, iters)
    assert bool((assign >= 3 * 4096).any()) and bool((assign < 4096).any())     # objects of the first and the fourth tile are taken


def test_emd_workspace_contract():
    from houv_amd import _lib, ops
    B, N, iters, eps = 2, 4099, 8, 0.05
    x1, x2 = _clouds(B, N, seed=21)
    base = _check(x1, x2, eps, iters)
    x1, x2 = x1.to(DEV), x2.to(DEV)
    need = _lib.load().houv_emd_workspace_bytes(B, N)
    assert need == B * 20 * 4100
    # contents on entry are ignored: zeros, 0xFF bytes, what another call left behind
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    assert _same(ops.emd_forward(x1, x2, eps, iters, workspace=ws), base)
    ws.fill_(0xFF)
    assert _same(ops.emd_forward(x1, x2, eps, iters, workspace=ws), base)
    o1, o2 = _clouds(B, N, seed=22, kind="grid")
    ops.emd_forward(o1.to(DEV), o2.to(DEV), 0.005, 11, workspace=ws)
    assert _same(ops.emd_forward(x1, x2, eps, iters, workspace=ws), base)
    # no alignment beyond 4 bytes, and nothing outside the houv_emd_workspace_bytes bytes is touched
    big = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    off = (4 - big.data_ptr()) % 16
    view = big[off:off + need]
    assert view.data_ptr() % 16 == 4 and view.numel() == need
    assert _same(ops.emd_forward(x1, x2, eps, iters, workspace=view), base)
    assert bool((big[:off] == 0xA5).all()) and bool((big[off + need:] == 0xA5).all())
    # one byte short
    with pytest.raises(_lib.HouvHipError):
        ops.emd_forward(x1, x2, eps, iters, workspace=big[:need - 1])


def _capi_forward(x1, x2, eps, iters, with_run, workspace):
    """houv_emd_forward through the C ABI; outputs prefilled so that a call that launches nothing leaves them as they are."""
    from houv_amd import _lib
    B, N, _ = x1.shape
    dist = torch.full((B, N), -7.0, dtype=torch.float32, device=DEV)
    assign = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    run = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ok = _lib.load().houv_emd_forward(_lib.ptr(x1), _lib.ptr(x2), B, N, N, float(eps), int(iters), _lib.ptr(dist),
                                      _lib.ptr(assign), _lib.ptr(run) if with_run else None, _lib.ptr(workspace),
                                      _lib.stream_of(x1))
    torch.cuda.synchronize()
    return ok, dist, assign, run


def test_emd_null_workspace_is_refused():
    from houv_amd import _lib
    x1, x2 = _clouds(1, 4097, seed=23)
    ok, dist, assign, run = _capi_forward(x1.to(DEV), x2.to(DEV), 0.05, 2, True, None)
    assert ok == 0 and "needs a workspace" in _lib.last_error()
    assert bool((dist == -7.0).all()) and bool((assign == -7).all()) and bool((run == -7).all())   # nothing launched


@pytest.mark.parametrize("N", [300, 4097])
def test_emd_iters_run_null(N):
    from houv_amd import ops
    x1, x2 = _clouds(2, N, seed=24 + N)
    x1, x2 = x1.to(DEV), x2.to(DEV)
    ws = ops.emd_workspace(2, N, DEV)
    ok, dist, assign, run = _capi_forward(x1, x2, 0.05, 5, True, ws)
    assert ok == 1 and bool((run >= 1).all())
    ok, dist0, assign0, run0 = _capi_forward(x1, x2, 0.05, 5, False, ws)
    assert ok == 1 and bool((run0 == -7).all())
    assert _same((dist0, assign0, run), (dist, assign, run))
    assert _same(ops.emd_forward(x1, x2, 0.05, 5), (dist, assign, run))


# ---------------------------------------------------------------------------------------------------
# Backward: value for value against emd_host.emd_backward
# ---------------------------------------------------------------------------------------------------
def _backward_inputs(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand((B, N, 3), generator=g)
    x2 = torch.rand((B, N, 3), generator=g)
    gd = torch.randn((B, N), generator=g)
    assign = torch.rand((B, N), generator=g).argsort(dim=1).to(torch.int32)   # a random permutation per cloud
    return x1, x2, gd, assign


# (4195, 1000): 4,195,000 points, just over the 16384 x 256 that one trip of the grid-stride loop covers
@pytest.mark.parametrize("B,N", [(1, 1), (3, 255), (2, 257), (2, 4097), (4195, 1000)])
def test_emd_backward_exact(B, N):
    from houv_amd import ops
    assert (B * N > 16384 * 256) == (B == 4195)
    x1, x2, gd, assign = _backward_inputs(B, N, seed=B * 7 + N)
    got = ops.emd_backward(x1.to(DEV), x2.to(DEV), gd.to(DEV), assign.to(DEV)).cpu().numpy()
    want = emd_host.emd_backward(x1.numpy(), x2.numpy(), gd.numpy(), assign.numpy())
    assert np.array_equal(got, want)


def test_emd_backward_many_to_one():
    from houv_amd import ops
    x1, x2 = _clouds(2, 1000, seed=31)
    _, assign, _ = ops.emd_forward(x1.to(DEV), x2.to(DEV), 0.05, 1)           # the forced last step alone: no bijection
    a = assign.cpu().numpy()
    assert all(len(np.unique(row)) < 1000 for row in a)
    gd = torch.randn((2, 1000), generator=torch.Generator().manual_seed(32))
    got = ops.emd_backward(x1.to(DEV), x2.to(DEV), gd.to(DEV), assign).cpu().numpy()
    assert np.array_equal(got, emd_host.emd_backward(x1.numpy(), x2.numpy(), gd.numpy(), a))


def test_emd_backward_accumulates_into_the_callers_buffer():
    from houv_amd import _lib
    B, N = 2, 257
    x1, x2, g1, assign = _backward_inputs(B, N, seed=33)
    g2 = torch.randn((B, N), generator=torch.Generator().manual_seed(34))
    pattern = torch.randn((B, N, 3), generator=torch.Generator().manual_seed(35))
    d = [t.to(DEV) for t in (x1, x2, g1, g2, assign)]

    def call(gd, buf):
        ok = _lib.load().houv_emd_backward(_lib.ptr(d[0]), _lib.ptr(d[1]), B, N, _lib.ptr(gd), _lib.ptr(d[4]), _lib.ptr(buf),
                                           _lib.stream_of(buf))
        assert ok == 1
        torch.cuda.synchronize()

    buf = torch.zeros((B, N, 3), dtype=torch.float32, device=DEV)
    call(d[2], buf)
    call(d[3], buf)
    want = emd_host.emd_backward(x1.numpy(), x2.numpy(), g1.numpy(), assign.numpy())
    want = emd_host.emd_backward(x1.numpy(), x2.numpy(), g2.numpy(), assign.numpy(), into=want)
    assert np.array_equal(buf.cpu().numpy(), want)
    buf = pattern.to(DEV)
    call(d[2], buf)
    want = emd_host.emd_backward(x1.numpy(), x2.numpy(), g1.numpy(), assign.numpy(), into=pattern.numpy().copy())
    assert np.array_equal(buf.cpu().numpy(), want)
    assert not np.array_equal(want, pattern.numpy())


# ---------------------------------------------------------------------------------------------------
# Non-finite coordinates: properties only (the sign of the default NaN differs between host and GPU: no host parity)
# ---------------------------------------------------------------------------------------------------
def test_emd_non_finite_coordinates_stay_in_range():
    from houv_amd import ops
    B, N, iters, eps = 3, 300, 20, 0.05
    x1, x2 = _clouds(B, N, seed=41)
    x1[1, 7] = float("nan")
    x2[1, 11] = float("inf")
    dist, assign, run = ops.emd_forward(x1.to(DEV), x2.to(DEV), eps, iters)
    keep = [0, 2]
    clean = ops.emd_forward(x1[keep].to(DEV), x2[keep].to(DEV), eps, iters)
    assert _same((dist[keep], assign[keep], run[keep]), clean)               # the finite clouds do not notice cloud 1
    _check(x1[keep], x2[keep], eps, iters)
    a = assign[1].cpu().numpy()
    assert a.min() >= 0 and a.max() < N
    # bidder 7's increment is NaN, whose bits outrank every finite key: it takes object 0 (no value ever compares greater,
    # so its bid object stays at the guard's 0) at t = 0 and keeps it
    assert a[7] == 0
    assert np.isnan(dist[1, 7].item())
    assert not (a == 11).any()                                   # value -inf: never greater than any best
    assert 1 <= int(run[1]) <= iters
