"""GPU: the two ECG kernels.  houv_knn_feat: idx AND dist2 bit-equal to the host function hm_knn_feat
(tests/ecg_hostmath) at every size at which the kernel takes another path -- the wave of 64 queries, the register block of 32
candidates, the channel chunks 16 / 8 / 4 / 2 / 1, the three list sizes.  houv_dense_conv: against the float64 NumPy restatement
of ecg.py:58-65 in the reference's materialising form (tests/ecg_host.py) within 4x the float32 restatement's own maximum error
on the same inputs, computed and printed per case; where that error is 0 the results must be equal."""
import ctypes

import numpy as np
import pytest
import torch

import ecg_cases as cases
import ecg_host as host

pytestmark = pytest.mark.gpu
T = torch.tensor

# one below / above the wave (63, 65), the candidate block (31, 33) and the chunk (15, 17) besides the issue's sizes
KNN_N = (1, 16, 17, 31, 33, 63, 64, 65, 257)
KNN_C = (1, 3, 15, 17, 24, 48, 256)
KNN_K = (1, 4, 16, 20, 32)
DENSE_N = (1, 3, 5, 63, 64, 65, 130)
DENSE_K = (1, 4, 16, 20)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def test_block_constants():
    from houv_amd import ops
    assert (ops.KNN_FEAT_BLOCK, ops.KNN_FEAT_CHUNK, ops.DENSE_CONV_GROWTH) == (32, 16, host.G)
    assert {31, 33} <= set(KNN_N) and {15, 17} <= set(KNN_C)


# ---------------------------------------------------------------------------------------------------------------- knn_feat
@pytest.mark.parametrize("N", KNN_N)
@pytest.mark.parametrize("C", KNN_C)
def test_knn_feat_every_entry_exact(dev, C, N):
    """Three clouds per launch and one alone, rows wider than C (ldx > C), every k <= N of KNN_K, every input family."""
    from houv_amd import ops
    for family in cases.KNN_FAMILIES:
        for B in (3, 1):
            x = cases.knn_cloud(family, B, N, C, C + 3)
            want_i, want_d = cases.knn_expected(family, B, N, C, C + 3)
            xd = T(x).to(dev)
            for k in (KNN_K if B == 3 else (16,)):
                if k > N:
                    continue
                idx, d2 = ops.knn_feat(xd[:, :, :C], k, want_dist=True)
                assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, N, k)
                assert np.array_equal(idx.cpu().numpy(), want_i[..., :k]), (family, B, k)
                assert np.array_equal(_bits(d2), want_d[..., :k].view(np.int32)), (family, B, k)
                if family == "identical":
                    assert np.array_equal(idx.cpu().numpy(), np.broadcast_to(np.arange(k, dtype=np.int32), (B, N, k)))
            only = ops.knn_feat(xd[:, :, :C], min(N, 4))                      # dist2 == NULL
            assert np.array_equal(only.cpu().numpy(), want_i[..., :min(N, 4)])


@pytest.mark.parametrize("N,k", [(65, 20), (257, 8), (40, 32), (5, 3)])
def test_knn_feat_three_channels_equal_knn_cross(dev, N, k):
    from houv_amd import ops
    from houv_amd.mm3d_pn2 import knn_cross
    for family in cases.KNN_FAMILIES:
        x = T(cases.knn_cloud(family, 2, N, 3, 3)).to(dev)
        idx, d2 = ops.knn_feat(x, k, want_dist=True)
        d3, i3 = knn_cross(k, x, x)
        assert torch.equal(idx, i3) and np.array_equal(_bits(d2), _bits(d3))


def test_knn_feat_refusals(dev):
    from houv_amd import _lib
    lib = _lib.load()
    x = torch.zeros((2, 40, 300), device=dev)
    idx = torch.zeros((2, 40, 32), dtype=torch.int32, device=dev)
    d2 = torch.zeros((2, 40, 32), device=dev)

    def call(N=40, C=24, ldx=300, k=16, x=x, idx=idx, d2=d2):
        return lib.houv_knn_feat(_lib.ptr(x), 2, N, C, ldx, k, _lib.ptr(idx), _lib.ptr(d2), None)
    for kw, msg in ((dict(N=8, k=9), "k=9"), (dict(C=0), "C=0"), (dict(C=257), "C=257"), (dict(k=33), "k=33"), (dict(k=0), "k=0"),
                    (dict(C=24, ldx=23), "ldx=23"), (dict(N=16385), "N=16385"), (dict(x=None), "null pointer"),
                    (dict(idx=None), "null pointer")):
        assert call(**kw) == 0 and "houv_knn_feat" in _lib.last_error() and msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(d2=None) == 1 and call() == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- dense_conv
def _dense(dev, case, relu_out=False, out=None):
    from houv_amd import ops
    x, idx, *w = (T(a).to(dev) for a in case)
    return ops.dense_conv(x, idx, *w, relu_out=relu_out, out=out)


def _check(got, want64, err32, what):
    err = float(np.abs(got.astype(np.float64) - want64).max())
    print(what, "kernel vs float64", err, "float32 restatement vs float64", err32, "bound", 4 * err32)
    if err32 == 0:
        assert np.array_equal(got.astype(np.float64), want64), what
    assert err <= 4 * err32, what


@pytest.mark.parametrize("N", DENSE_N)
@pytest.mark.parametrize("C", (24, 48))
def test_dense_conv_vs_float64(dev, C, N):
    for B in (1, 3):
        for k in DENSE_K:
            want, err32 = cases.dense_expected(B, N, C, k)
            got = _dense(dev, cases.dense_case(B, N, C, k)).cpu().numpy()
            assert got.shape == (B, N, C + 72)
            _check(got, want, err32, f"C={C} N={N} B={B} k={k}")


@pytest.mark.parametrize("kind", ["self", "repeat", "last", "negative"])
@pytest.mark.parametrize("C", (24, 48))
def test_dense_conv_neighbour_patterns(dev, C, kind):
    B, N, k = 2, 65, 16
    case = cases.dense_case(B, N, C, k, kind)
    want, err32 = cases.dense_expected(B, N, C, k, kind)
    got = _dense(dev, case).cpu().numpy()
    _check(got, want, err32, f"{kind} C={C}")
    if kind == "negative":
        assert (want[..., C + 48:] < 0).all() and (got[..., C + 48:] < 0).all()      # a pool that starts at 0 returns 0 here
    if kind == "last":
        # the far neighbour, listed last, alone attains the maximum in a good share of the channels
        x, idx, *w = case
        first = host.dense_conv(np.swapaxes(x, 1, 2), idx[..., :-1].astype(np.int64), *w, dtype=np.float64)
        assert (np.swapaxes(first, 1, 2) < want).mean() > 0.2
    relu = _dense(dev, case, relu_out=True).cpu().numpy()
    assert np.array_equal(relu, np.maximum(got, 0))


@pytest.mark.parametrize("C", (24, 48))
def test_dense_conv_on_knn_feat_lists_into_a_wider_buffer(dev, C):
    """The model's call: lists from houv_knn_feat, x a column slice of the buffer the result is written into (ldx, ldo > width),
    the caller's relu; the columns beyond C + 72 keep their contents."""
    from houv_amd import ops
    B, N, k = 3, 130, 16
    x, _, *w = cases.dense_case(B, N, C, k)
    wide = torch.full((B, N, C + 72 + C + 5), -7.0, device=dev)
    wide[..., C + 72:2 * C + 72] = T(x).to(dev)
    xs = wide[..., C + 72:2 * C + 72]
    idx = ops.knn_feat(xs, k)
    ops.dense_conv(xs, idx, *(T(a).to(dev) for a in w), relu_out=True, out=wide[..., :C + 72])
    got = wide.cpu().numpy()
    assert np.array_equal(got[..., C + 72:2 * C + 72], x) and (got[..., 2 * C + 72:] == -7.0).all()
    xc = np.ascontiguousarray(np.swapaxes(x, 1, 2))
    i64 = idx.cpu().numpy().astype(np.int64)
    f64 = np.swapaxes(host.dense_conv(xc, i64, *w, dtype=np.float64), 1, 2)
    f32 = np.swapaxes(host.dense_conv(xc, i64, *w, dtype=np.float32), 1, 2)
    _check(got[..., :C + 72], np.maximum(f64, 0), float(np.abs(np.maximum(f32, 0).astype(np.float64) - np.maximum(f64, 0)).max()),
           f"knn_feat lists C={C}")


@pytest.mark.parametrize("C", (24, 48))
def test_dense_conv_zero_weights_exact(dev, C):
    B, N, k = 2, 70, 4
    case = cases.dense_case(B, N, C, k, "zero")
    x, _, _, b0, _, b1, _, b2 = case
    got = _dense(dev, case).cpu().numpy()
    want = np.concatenate([np.broadcast_to(np.maximum(b0, 0), (B, N, 24)), x, np.broadcast_to(np.maximum(b1, 0), (B, N, 24)),
                           np.broadcast_to(b2, (B, N, 24))], axis=2)
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32))
    assert (b2 < 0).any()


def test_dense_conv_out_of_range_indices_are_clamped(dev):
    B, N, C, k = 1, 40, 24, 4
    x, idx, *w = cases.dense_case(B, N, C, k)
    wild = idx.copy()
    wild[0, ::3, 1], wild[0, 1::3, 2] = -5, N + 1000
    got = _dense(dev, (x, wild, *w)).cpu().numpy()
    want = _dense(dev, (x, np.clip(wild, 0, N - 1), *w)).cpu().numpy()
    assert np.array_equal(got, want)


def test_dense_conv_refusals(dev):
    from houv_amd import _lib
    lib = _lib.load()
    x = torch.zeros((2, 40, 48), device=dev)
    idx = torch.zeros((2, 40, 33), dtype=torch.int32, device=dev)
    w = torch.zeros(24 * 96, device=dev)
    out = torch.zeros((2, 40, 130), device=dev)

    def call(C=48, k=16, ldx=48, ldo=130, x=x, W1=w, out=out):
        p = _lib.ptr
        return lib.houv_dense_conv(p(x), ldx, p(idx), 2, 40, C, k, p(w), p(w), p(W1), p(w), p(w), p(w), 0, p(out), ldo, None)
    for kw, msg in ((dict(C=32), "C=32"), (dict(k=33), "k=33"), (dict(k=0), "k=0"), (dict(ldo=119), "ldo=119"),
                    (dict(ldx=47), "ldx=47"), (dict(x=None), "x is a null pointer"), (dict(W1=None), "W1 is a null pointer"),
                    (dict(out=None), "out is a null pointer")):
        assert call(**kw) == 0 and "houv_dense_conv" in _lib.last_error() and msg in _lib.last_error(), (kw, _lib.last_error())
    assert call() == 1
    torch.cuda.synchronize()


def test_torch_ops_are_registered(dev):
    from houv_amd import ops
    ops.register_torch_ops()
    x = T(cases.knn_cloud("random", 1, 40, 24, 24)).to(dev)
    idx, d2 = torch.ops.houv.knn_feat(x, 4)
    assert torch.equal(idx, ops.knn_feat(x, 4))
    case = [T(a).to(dev) for a in cases.dense_case(1, 5, 24, 4)]
    assert torch.equal(torch.ops.houv.dense_conv(*case, False), ops.dense_conv(*case))
