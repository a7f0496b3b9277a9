"""GPU: every dispatch branch and launch edge of the DCP feature-head kernels (houv_amd/csrc/dcp_ops.hip, gemm.hip, attention.hip)
through the wrappers of houv_amd/ops.py, each against a plain reference of the same operation from tests/dcp_ops_host.py:

* exact where the contract is exact: k-NN lists against the std::fmaf brute force of tests/hostmath, index for index, for every
  query; max_over_k against act.view(npts, k, C).max(1);
* float64 elsewhere.  edgeconv1 has a derived elementwise bound.  layernorm, softmax_rows_ and softmax_corr are held to
  host.margin: 4x the error of the same formula composed from fp32 torch operations on the CPU (measured per case, against the
  same float64 reference), plus 2 ulp of the output magnitude; layernorm adds the derived rounding of the row mean
  (host.layernorm_margin).  gemm and attention keep the measures of tests/test_gpu_dcp.py.

tests/test_dcp_ops_host.py checks the references and the inputs' properties without a GPU.  Every test prints its figures (-s)."""
import numpy as np
import pytest
import torch

import dcp_ops_host as host

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# knn: knn_kernel<1|3|8|16|20> (one and several 1024-stages, partial blocks) and knn_split_kernel<16|20> (N >= 512)
# ---------------------------------------------------------------------------------------------------------------------
def _knn(dev, x, k, split):
    from houv_amd import _lib, ops
    try:
        _lib.debug_set("knn_split", split)
        return ops.knn(x.to(dev), k).cpu().long()
    finally:
        _lib.debug_set("knn_split", 1)


@pytest.mark.parametrize("k,N", [(k, N) for k in host.KNN_K for N in host.knn_sizes(k)])
def test_knn_lists_equal_the_host_lists_for_every_query(dev, k, N):
    """Tie-free clouds (asserted on the CPU): both kernels must return the (distance, index)-lexicographic list, exactly."""
    x = host.knn_cloud(N)
    want = host.knn_lists(N)[0][..., :k]
    for split in ((1, 0) if N >= 512 else (1,)):
        got = _knn(dev, x, k, split)
        assert got.shape == (host.KNN_B, N, k)
        bad = (got != want).any(-1)
        assert not bool(bad.any()), (f"knn_split={split}: {int(bad.sum())} of {bad.numel()} lists differ, first at "
                                     f"(batch, query) {bad.nonzero()[0].tolist()}: {got[bad][0].tolist()} != {want[bad][0].tolist()}")


@pytest.mark.parametrize("k", [3, 8, 16, 20])
@pytest.mark.parametrize("N", host.KNN_DUP_N)
def test_knn_with_duplicate_points(dev, N, k):
    """Exact duplicates in different quarters and different 1024-stages (asserted on the CPU).  The split kernel (k = 16, 20) merges
    its quarters by (distance, quarter): the lexicographic list exactly.  The single scan's insertion lets a displaced entry leapfrog
    its equals, so among tied entries its order -- and which copy survives at the k-th place -- is not defined: its distances must
    equal the host's entry by entry (bit for bit: tied entries are copies of one point) and every list holds k distinct valid
    indices."""
    x = host.knn_dup_cloud(N)
    want = host.knn_lists(N, dup=True)[0][..., :k]

    def dist(idx):
        xd = x.double()
        nb = xd.reshape(-1, 3)[(idx + torch.arange(host.KNN_B).view(-1, 1, 1) * N).reshape(-1)].reshape(host.KNN_B, N, k, 3)
        return ((nb - xd.unsqueeze(2)) ** 2).sum(-1)

    if k in (16, 20):
        assert torch.equal(_knn(dev, x, k, 1), want)
    single = _knn(dev, x, k, 0)
    assert int(single.min()) >= 0 and int(single.max()) < N
    assert bool((single.sort(-1)[0].diff(dim=-1) > 0).all())
    assert torch.equal(dist(single), dist(want))
    assert not torch.equal(want, host.knn_lists(N)[0][..., :k])      # the duplicates reach the lists


def test_knn_refuses_k_above_n_and_unsupported_k(dev):
    from houv_amd import _lib, ops
    x = host.knn_cloud(64).to(dev)
    with pytest.raises(_lib.HouvHipError, match="k must be one of"):
        ops.knn(x, 5)
    with pytest.raises(_lib.HouvHipError, match="bad argument"):
        ops.knn(x[:, :7].contiguous(), 8)
    with pytest.raises(_lib.HouvHipError):
        ops.knn(x[:, ::2], 3)                                        # strided view


# ---------------------------------------------------------------------------------------------------------------------
# edgeconv1: one launch of up to 16384 blocks; above 262,144 edges the grid-stride loop repeats
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k", host.EDGECONV_CASES)
def test_edgeconv1_against_float64(dev, B, N, k):
    from houv_amd import ops
    xyz, idx, W, scale, shift = host.edgeconv_inputs(B, N, k)
    if k in host.KNN_K and k <= N:
        idx = ops.knn(xyz.to(dev), k).cpu()                          # the model's own neighbours
    out = ops.edgeconv1(xyz.to(dev), idx.to(dev), W.to(dev), scale.to(dev), shift.to(dev))
    assert out.shape == (B * N * k, 64) and out.dtype == torch.float32
    pre, ref, bound = host.edgeconv1_ref(xyz, idx, W, scale, shift)
    if N > 1:
        assert bool((pre > 0).any()) and bool((pre < 0).any())       # ReLU clips some outputs and passes others
    ratio = (out.cpu().double() - ref).abs() / bound
    print(f"edgeconv1 B={B} N={N} k={k}: {B * N * k} edges, max error / bound = {float(ratio.max()):.3f}")
    bad = ratio > 1
    assert not bool(bad.any()), f"{int(bad.sum())} outputs outside the bound, first (edge, channel) {bad.nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# max_over_k
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts,k,C", [(1, 1, 4), (11, 20, 64), (300, 7, 256), (70000, 2, 256)])
def test_max_over_k_is_exact_and_writes_only_its_columns(dev, npts, k, C):
    """(70000, 2, 256): npts * C / 4 > 16384 * 256, the grid-stride loop repeats.  The output is a slice (row stride > width) of a
    wider buffer; columns outside [col0, col0 + C) and the buffer's padding keep their sentinel bit for bit."""
    from houv_amd import ops
    gen = torch.Generator().manual_seed(npts + k + C)
    act = torch.randn(npts, k, C, generator=gen)
    g = torch.arange(npts)
    place = torch.tensor([0, k - 1, k // 2])[g % 3]                  # the maximum first, last and in the middle of its group
    act[g, place] += 10.0
    act[g % 5 == 0] -= 100.0                                         # all-negative groups: a maximum that starts at 0 fails
    want = act.max(1)[0]
    assert bool((want[g % 5 == 0] < 0).all()) and bool((act.argmax(1) == place.view(-1, 1)).all())
    width, stride = 3 * C, 3 * C + 8
    act_d, want_d = act.reshape(npts * k, C).to(dev), want.to(dev)
    for col0 in sorted({0, C, width - C}):
        buf = torch.full((npts, stride), SENTINEL, device=dev)
        out = buf[:, :width]
        ops.max_over_k(act_d, k, out, col0)
        assert torch.equal(_bits(buf[:, col0:col0 + C]), _bits(want_d)), f"col0={col0}"
        keep = torch.ones(stride, dtype=torch.bool, device=dev)
        keep[col0:col0 + C] = False
        assert bool((_bits(buf[:, keep]) == _bits(torch.full((1,), SENTINEL, device=dev))).all()), f"col0={col0}"


def test_max_over_k_refuses_views_off_a_16_byte_boundary(dev):
    """The kernel moves float4: a col0 that is no multiple of 4, or an out / act base 4 bytes into an allocation, is refused by the
    wrapper before any launch (the output keeps its sentinel)."""
    from houv_amd import _lib, ops
    act = torch.randn(6 * 3, 8, device=dev)
    buf = torch.full((6, 24), SENTINEL, device=dev)
    for col0 in (1, 2, 3, 6):
        with pytest.raises(_lib.HouvHipError, match="16-byte"):
            ops.max_over_k(act, 3, buf, col0)
    flat = torch.full((6 * 24 + 4,), SENTINEL, device=dev)
    shifted = flat[1:1 + 6 * 24].view(6, 24)
    assert shifted.data_ptr() % 16 == 4
    with pytest.raises(_lib.HouvHipError, match="16-byte"):
        ops.max_over_k(act, 3, shifted, 0)
    act_shifted = torch.randn(6 * 3 * 8 + 4, device=dev)[1:1 + 6 * 3 * 8].view(18, 8)
    assert act_shifted.is_contiguous() and act_shifted.data_ptr() % 16 == 4
    with pytest.raises(_lib.HouvHipError, match="16-byte"):
        ops.max_over_k(act_shifted, 3, buf, 0)
    ops.max_over_k(act, 3, shifted, 3)                               # 4 + 12 bytes: aligned again, and accepted
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and torch.equal(shifted[:, 3:11], act.view(6, 3, 8).max(1)[0])
    assert bool((flat[:4] == SENTINEL).all()) and bool((shifted[:, :3] == SENTINEL).all()) and bool((shifted[:, 11:] == SENTINEL).all())
    with pytest.raises(_lib.HouvHipError):
        ops.max_over_k(act, 3, buf, 20)                              # col0 + C beyond the row
    with pytest.raises(_lib.HouvHipError):
        ops.max_over_k(act, 4, buf, 0)                               # 18 rows are no multiple of k


# ---------------------------------------------------------------------------------------------------------------------
# layernorm: one wave per row, four rows per block
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", host.LN_D)
def test_layernorm_against_float64(dev, D):
    from houv_amd import ops
    worst, failures = (-1.0, ""), []
    for rows in host.LN_ROWS:
        for variant in host.LN_VARIANTS:
            x, a, b, r = host.layernorm_inputs(D, rows, variant)
            xd, ad, bd, rd = (t.to(dev) for t in (x, a, b, r))
            for res, res_d in ((None, None), (r, rd)):
                ref = host.layernorm_ref(x, a, b, res)
                out = ops.layernorm(xd, ad, bd, host.LN_EPS, res_d)
                assert out.shape == x.shape
                err = host.max_err(out.cpu(), ref)
                err_c = host.max_err(host.layernorm_f32(x, a, b, res), ref)
                lim = host.layernorm_margin(x, a, err_c, float(ref.abs().max()))
                what = f"D={D} rows={rows} x{variant} residual={res is not None}: kernel {err:.3e} composition {err_c:.3e} margin {lim:.3e}"
                worst = max(worst, (err / host.ulp32(float(ref.abs().max())), what))
                if not err <= lim:
                    failures.append(what)
    print(f"layernorm D={D}: largest kernel error {worst[0]:.2f} ulp of the output magnitude ({worst[1]})")
    assert not failures, "\n".join(failures)


def test_layernorm_refuses_what_its_kernel_cannot_read(dev):
    from houv_amd import _lib, ops
    a, b = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    x = torch.randn(5, 8, device=dev)
    with pytest.raises(_lib.HouvHipError, match="multiple of 4"):
        ops.layernorm(torch.randn(5, 6, device=dev), torch.ones(6, device=dev), torch.zeros(6, device=dev))      # D = 6
    with pytest.raises(_lib.HouvHipError, match="contiguous"):
        ops.layernorm(torch.randn(5, 16, device=dev)[:, :8], a, b)                                               # row stride 16
    with pytest.raises(_lib.HouvHipError, match="contiguous"):
        ops.layernorm(torch.randn(8, 5, device=dev).t(), a, b)
    with pytest.raises(_lib.HouvHipError, match="contiguous"):
        ops.layernorm(x, a, b, residual=torch.randn(8, 5, device=dev).t())
    shifted = torch.randn(5 * 8 + 4, device=dev)[1:41].view(5, 8)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    for args in ((shifted, a, b), (x, a, b, 1e-6, shifted), (x, torch.ones(12, device=dev)[1:9], b), (x, a, torch.ones(12, device=dev)[1:9])):
        with pytest.raises(_lib.HouvHipError, match="16-byte"):
            ops.layernorm(*args)
    with pytest.raises(_lib.HouvHipError):
        ops.layernorm(x, torch.ones(4, device=dev), b)


# ---------------------------------------------------------------------------------------------------------------------
# softmax_rows_: register path (L % 4 == 0, L <= 4096, 16-byte aligned rows) and three-pass path
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_in_buffer(dev, x, offset):
    """Run softmax_rows_ on a view that starts `offset` floats into a sentinel-filled allocation; the values, and the check that
    nothing outside the view changed."""
    from houv_amd import ops
    rows, L = x.shape
    buf = torch.full((rows * L + 16,), SENTINEL, device=dev)
    view = buf[offset:offset + rows * L].view(rows, L)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    view.copy_(x.to(dev))
    assert ops.softmax_rows_(view) is view
    got = view.cpu()
    assert bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + rows * L:] == SENTINEL).all())
    return got


@pytest.mark.parametrize("L", host.SM_L)
def test_softmax_rows_against_float64(dev, L):
    worst, failures = (-1.0, ""), []
    for rows in host.SM_ROWS:
        for variant in host.SM_VARIANTS:
            x = host.softmax_inputs(L, rows, variant)
            ref = host.softmax_ref(x)
            err_c = host.max_err(host.softmax_f32(x), ref)
            lim = host.margin(err_c, float(ref.max()))
            runs = [("aligned", _softmax_in_buffer(dev, x, 4))]
            if L % 4 == 0 and rows == 5:
                runs.append(("base 4 bytes off", _softmax_in_buffer(dev, x, 1)))     # the three-pass path on register-path shapes
            for name, got in runs:
                err = host.max_err(got, ref)
                rowsum = float((got.double().sum(-1) - 1).abs().max())
                what = (f"L={L} rows={rows} x{variant} {name}: kernel {err:.3e} composition {err_c:.3e} margin {lim:.3e} "
                        f"|row sum - 1| {rowsum:.3e}")
                worst = max(worst, (err / host.ulp32(float(ref.max())), what))
                if not (err <= lim and rowsum <= L * host.EPS32) or not bool(torch.isfinite(got).all()):
                    failures.append(what)
                if variant == "special":
                    assert bool((got[torch.isinf(x)] == 0).all())
    print(f"softmax_rows L={L}: largest kernel error {worst[0]:.2f} ulp of the output magnitude ({worst[1]})")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------
# softmax_corr
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", host.SC_VARIANTS)
@pytest.mark.parametrize("P,N,M", host.SC_CASES)
def test_softmax_corr_against_float64(dev, P, N, M, variant):
    from houv_amd import ops
    scores, pts = host.softmax_corr_inputs(P, N, M, variant)
    ref = host.softmax_corr_ref(scores, pts)
    out = ops.softmax_corr(scores.to(dev), pts.to(dev))
    assert out.shape == (P, 3, N)
    err = host.per_coordinate_err(out.cpu(), ref)
    err_c = host.per_coordinate_err(host.softmax_corr_f32(scores, pts), ref)
    mag = ref.abs().amax(dim=(0, 2))
    lim = [host.margin(float(err_c[c]), float(mag[c])) for c in range(3)]
    print(f"softmax_corr P={P} N={N} M={M} {variant}: kernel {[f'{float(e):.3e}' for e in err]} composition "
          f"{[f'{float(e):.3e}' for e in err_c]} margin {[f'{m:.3e}' for m in lim]} "
          f"(kernel, ulp of the magnitude: {[round(float(err[c]) / host.ulp32(float(mag[c])), 2) for c in range(3)]})")
    assert all(float(err[c]) <= lim[c] for c in range(3))


def test_softmax_corr_refuses_strided_operands(dev):
    from houv_amd import _lib, ops
    s, pts = torch.randn(2, 8, 12, device=dev), torch.randn(2, 12, 3, device=dev)
    with pytest.raises(_lib.HouvHipError, match="contiguous"):
        ops.softmax_corr(torch.randn(2, 12, 8, device=dev).transpose(1, 2), pts)
    with pytest.raises(_lib.HouvHipError, match="contiguous"):
        ops.softmax_corr(s, torch.randn(2, 3, 12, device=dev).transpose(1, 2))
    with pytest.raises(_lib.HouvHipError, match="contiguous"):
        ops.softmax_corr(s, torch.randn(2, 12, 4, device=dev)[..., :3])
    with pytest.raises(_lib.HouvHipError):
        ops.softmax_corr(s, pts[:, :11].contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# gemm: errors in units of sum_k |a||b| against float64, as test_gemm_on_the_bf16_pipe_is_fp32_grade measures them
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_modes(fn, modes=(0, 6)):
    from houv_amd import _lib
    out = {}
    try:
        for mode in modes:
            _lib.debug_set("gemm_split", mode)
            out[mode] = fn()
    finally:
        _lib.debug_set("gemm_split", 6)
    return out


def _assert_fp32_grade(err, what):
    print(f"gemm {what}: error in units of sum|a||b|: fp32-input {err[0]:.3e}, split {err[6]:.3e}")
    assert err[0] < 8e-7 and err[6] < 1.5 * err[0], (what, err)


@pytest.mark.parametrize("M,N,K", [(128, 64, 32), (256, 128, 64), (384, 256, 1024)])
def test_gemm_kn_operand_on_full_tiles(dev, M, N, K):
    """trans_b=False with every tile full: gemm_f32_kernel<64|128, false, false> (the split kernels take [N,K] operands only, so both
    settings of gemm_split run it)."""
    from houv_amd import ops
    gen = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(M, K, generator=gen) * torch.rand(M, 1, generator=gen).mul(6).exp()).to(dev)
    B = torch.randn(K, N, generator=gen).to(dev)
    ref = A.double() @ B.double()
    unit = A.double().abs() @ B.double().abs()
    got = _gemm_modes(lambda: ops.gemm(A, B, trans_b=False))
    _assert_fp32_grade({m: float(((c.double() - ref).abs() / unit).max()) for m, c in got.items()}, f"[K,N] {M}x{N}x{K}")
    assert torch.equal(got[0], got[6])
    eye = torch.eye(M, K, device=dev)                                # A = I, asymmetric B: the row and column map, exactly
    for c in _gemm_modes(lambda: ops.gemm(eye, B, trans_b=False)).values():
        assert torch.equal(c[:K], B[:M]) and not bool(c[K:].any())   # rows of B below the M-th meet no 1


@pytest.mark.parametrize("N", [64, 128, 512])
def test_gemm_epilogue_on_the_split_kernels(dev, N):
    """alpha, scale, shift, residual, relu / bias only / a strided preallocated C, on full tiles: gemm_split_kernel<64|128, 6> and,
    with gemm_split 0, gemm_f32_kernel<64|128, true, false>."""
    from houv_amd import ops
    M, K = 256, 128
    gen = torch.Generator().manual_seed(N)
    A = torch.randn(M, K, generator=gen).to(dev); W = torch.randn(N, K, generator=gen).to(dev)
    sc = (torch.randn(N, generator=gen) * 2).to(dev); sh = torch.randn(N, generator=gen).to(dev)
    R = torch.randn(M, N, generator=gen).to(dev)
    prod = A.double() @ W.double().t()
    aprod = A.double().abs() @ W.double().abs().t()
    # the full epilogue
    pre = 0.37 * prod * sc.double() + sh.double() + R.double()
    assert bool((pre < 0).any()) and bool((pre > 0).any()) and bool((sc < 0).any())
    unit = 0.37 * aprod * sc.double().abs() + sh.double().abs() + R.double().abs()
    got = _gemm_modes(lambda: ops.gemm(A, W, scale=sc, shift=sh, residual=R, relu=True, alpha=0.37))
    _assert_fp32_grade({m: float(((c.double() - torch.relu(pre)).abs() / unit).max()) for m, c in got.items()}, f"epilogue N={N}")
    # bias only
    got = _gemm_modes(lambda: ops.gemm(A, W, shift=sh))
    _assert_fp32_grade({m: float(((c.double() - (prod + sh.double())).abs() / (aprod + sh.double().abs())).max())
                        for m, c in got.items()}, f"bias N={N}")
    # C = a column block of a wider buffer (ldc > N)
    def strided():
        buf = torch.full((M + 2, N + 96), SENTINEL, device=dev)
        ret = ops.gemm(A, W, buf[1:M + 1, 32:32 + N], alpha=-2.0)
        assert ret.data_ptr() == buf[1:M + 1, 32:32 + N].data_ptr()
        return buf
    got = _gemm_modes(strided)
    for buf in got.values():
        inside = torch.zeros_like(buf, dtype=torch.bool)
        inside[1:M + 1, 32:32 + N] = True
        assert bool((buf[~inside] == SENTINEL).all())
    _assert_fp32_grade({m: float(((buf[1:M + 1, 32:32 + N].double() + 2.0 * prod).abs() / (2.0 * aprod)).max())
                        for m, buf in got.items()}, f"strided C N={N}")
    # A = I with an asymmetric B, through the epilogue's identity settings
    eye = torch.eye(M, K, device=dev)
    for c in _gemm_modes(lambda: ops.gemm(eye, W)).values():
        assert torch.equal(c[:K], W.t()) and not bool(c[K:].any())


def test_gemm_batched_per_head_views_on_full_tiles(dev):
    """The model's attention products at Nq = Nk = 256, batch = P x H strided per-head views: Q K^T on gemm_split_kernel<128, 6>
    (gemm_f32_kernel<128, true, false> with gemm_split 0), P V on gemm_f32_kernel<128, false, false>."""
    from houv_amd import ops
    P, H, Nq, Nk, dk = 2, 4, 256, 256, 128
    gen = torch.Generator().manual_seed(21)
    Q = torch.randn(P, Nq, H, dk, generator=gen).to(dev); Kt = torch.randn(P, Nk, H, dk, generator=gen).to(dev)
    V = torch.randn(P, Nk, H, dk, generator=gen).to(dev)
    refS = 0.25 * torch.einsum("pqhd,pkhd->phqk", Q.double(), Kt.double())
    unitS = 0.25 * torch.einsum("pqhd,pkhd->phqk", Q.double().abs(), Kt.double().abs())
    got = _gemm_modes(lambda: ops.gemm(Q.permute(0, 2, 1, 3), Kt.permute(0, 2, 1, 3), trans_b=True, alpha=0.25))
    assert got[6].shape == (P, H, Nq, Nk)
    _assert_fp32_grade({m: float(((s.double() - refS).abs() / unitS).max()) for m, s in got.items()}, "Q K^T per head")
    S = got[6]

    def pv():
        ctx = torch.full((P, Nq, H, dk), SENTINEL, device=dev)
        ops.gemm(S, V.permute(0, 2, 1, 3), ctx.permute(0, 2, 1, 3), trans_b=False)
        return ctx
    refC = torch.einsum("phqk,pkhd->pqhd", S.double(), V.double())
    unitC = torch.einsum("phqk,pkhd->pqhd", S.double().abs(), V.double().abs())
    _assert_fp32_grade({m: float(((c.double() - refC).abs() / unitC).max()) for m, c in _gemm_modes(pv).items()}, "P V per head")
    # every head its own block: head h of pair p must see only its own operands
    Ksel = torch.zeros_like(Kt)
    Ksel[1, :, 2] = Kt[1, :, 2]
    only = ops.gemm(Q.permute(0, 2, 1, 3), Ksel.permute(0, 2, 1, 3), trans_b=True)
    mask = torch.zeros(P, H, dtype=torch.bool)
    mask[1, 2] = True
    assert not bool(only[~mask].any()) and bool(only[1, 2].any())


@pytest.mark.parametrize("M,N,K,tb,pad", [(128, 128, 40, True, 0), (128, 128, 40, False, 0), (128, 65, 64, True, 0), (129, 64, 64, True, 0),
                                         (128, 64, 64, False, 0), (128, 128, 64, True, 3), (128, 64, 64, True, 1)])
def test_gemm_guarded_edges(dev, M, N, K, tb, pad):
    """One guarded case each: K % 32 != 0; N = 65 (wide kernel, a tile of one column); N = 64 with M = 129; an lda that is no multiple
    of 4 (scalar loads), wide and narrow.  (128, 64, 64, False) is the unguarded narrow [K,N] kernel at another K."""
    from houv_amd import ops
    gen = torch.Generator().manual_seed(M * 7 + N + K + pad)
    A = torch.randn(M, K + pad, generator=gen).to(dev)[:, :K]
    assert A.stride(0) == K + pad
    B = (torch.randn(N, K, generator=gen) if tb else torch.randn(K, N, generator=gen)).to(dev)
    Bop = B.double().t() if tb else B.double()
    ref, unit = A.double() @ Bop, A.double().abs() @ Bop.abs()
    got = _gemm_modes(lambda: ops.gemm(A, B, trans_b=tb))
    assert got[6].shape == (M, N)
    _assert_fp32_grade({m: float(((c.double() - ref).abs() / unit).max()) for m, c in got.items()}, f"guarded {M}x{N}x{K} tb={tb} lda={K + pad}")
    eye = torch.zeros(M, K + pad, device=dev)
    eye[:, :K] = torch.eye(M, K)
    c = ops.gemm(eye[:, :K], B, trans_b=tb)
    want = B.t() if tb else B
    assert torch.equal(c[:min(M, K)], want[:min(M, K)]) and not bool(c[K:].any())


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _attention_ref(q, k, v, scale):
    """dcp.py:26-32 in float64 on [P, N, H, 128] operands."""
    qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    return (torch.softmax(qd @ kd.transpose(-1, -2) * scale, dim=-1) @ vd).permute(0, 2, 1, 3)


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("N", [256, 77, 128, 33])
def test_attention_on_q_k_v_sliced_from_one_packed_buffer(dev, N, H):
    """Token stride 3 * H * 128 > H * 128: Q, K and V are column blocks of one [P, N, 3 * H * 128] buffer.  N = 256, 128: full tiles
    (attention_split_kernel and its K / V split kernels; attention_f32_kernel<true> with attn_split 0); N = 77, 33: tails
    (attention_f32_kernel<false>).  The result must also equal, bit for bit, the one from contiguous copies of the operands."""
    from houv_amd import _lib, ops
    P, dk = 2, 128
    gen = torch.Generator().manual_seed(N * 10 + H)
    packed = torch.randn(P, N, 3 * H * dk, generator=gen).to(dev)
    q, k, v = (packed[..., i * H * dk:(i + 1) * H * dk].unflatten(-1, (H, dk)) for i in range(3))
    assert q.stride(1) == 3 * H * dk and q.stride(2) == dk and not q.is_contiguous()
    scale = 1.0 / np.sqrt(dk)
    ref = _attention_ref(q.cpu(), k.cpu(), v.cpu(), scale)
    before = packed.clone()
    try:
        for mode in (1, 0):
            _lib.debug_set("attn_split", mode)
            out = ops.attention(q, k, v, scale)
            assert out.shape == (P, N, H, dk) and torch.equal(packed, before)
            print(f"attention packed N={N} H={H} attn_split={mode}: max error {float((out.cpu().double() - ref).abs().max()):.3e}")
            np.testing.assert_allclose(out.cpu().numpy(), ref.float().numpy(), rtol=2e-5, atol=2e-5)
            assert torch.equal(out, ops.attention(q.contiguous(), k.contiguous(), v.contiguous(), scale))
    finally:
        _lib.debug_set("attn_split", 1)


def test_attention_of_no_pairs_is_empty(dev):
    from houv_amd import ops
    q = torch.empty(0, 128, 4, 128, device=dev)
    out = ops.attention(q, q, q, 0.1)
    assert out.shape == (0, 128, 4, 128) and out.numel() == 0


@pytest.mark.parametrize("Nq,Nk", [(128, 33), (129, 32), (1, 32), (128, 1)])
def test_attention_tails_do_not_depend_on_attn_split(dev, Nq, Nk):
    """A tail in either dimension falls from the split kernel back to attention_f32_kernel<false>: the same kernel with attn_split on
    and off, hence the same bits; and right against float64."""
    from houv_amd import _lib, ops
    P, H, dk = 2, 4, 128
    gen = torch.Generator().manual_seed(Nq * 100 + Nk)
    q = torch.randn(P, Nq, H, dk, generator=gen).to(dev)
    k = torch.randn(P, Nk, H, dk, generator=gen).to(dev)
    v = torch.randn(P, Nk, H, dk, generator=gen).to(dev)
    scale = 1.0 / np.sqrt(dk)
    out = {}
    try:
        for mode in (1, 0):
            _lib.debug_set("attn_split", mode)
            out[mode] = ops.attention(q, k, v, scale)
    finally:
        _lib.debug_set("attn_split", 1)
    assert torch.equal(_bits(out[1]), _bits(out[0]))
    np.testing.assert_allclose(out[1].cpu().numpy(), _attention_ref(q.cpu(), k.cpu(), v.cpu(), scale).float().numpy(), rtol=2e-5, atol=2e-5)
