"""GPU: houv_sa_attn through ops.gemm + ops.sa_attn, against the float64 NumPy restatement of
vrcnet.py:49-67 in the reference's materialising form (tests/vrcnet_host.py) within 4x the float32 restatement's own maximum
error on the same inputs, computed and printed per case; where that error is 0 the results must be equal (the rule of
test_gpu_ecg_ops._check).  Then the layer goldens of the real reference through SA_module and SK_SA_module on the device."""
import numpy as np
import pytest
import torch

import vrcnet_cases as cases
from test_gpu_ecg_ops import _check

pytestmark = pytest.mark.gpu
T = torch.tensor
# the issue's sizes, and one below / above the 128 points of a workgroup
SA_N = (1, 5, 63, 64, 65, 127, 129, 130)
SA_K = (1, 10, 16, 20, 32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_block_constant():
    from houv_amd import ops
    assert ops.SA_ATTN_BLOCK == 128 and {127, 129} <= set(SA_N)


def _weights(dev, st, prefix=""):
    m = lambda n: T(st[prefix + n]).to(dev).reshape(st[prefix + n].shape[0], -1).contiguous()
    v = lambda n: T(st[prefix + n]).to(dev)
    Wp = torch.cat((m("conv1.weight"), m("conv2.weight"), m("conv3.weight")), 0)
    bp = torch.cat((v("conv1.bias"), v("conv2.bias"), v("conv3.bias")), 0)
    return Wp, bp, (m("conv_w.1.weight"), m("conv_w.3.weight"), v("conv_w.3.bias"), m("conv_out.weight"), v("conv_out.bias"))


def _project(x, Wp, bp):
    from houv_amd import ops
    B, N, C = x.shape
    return ops.gemm(torch.relu(x).reshape(-1, C), Wp, shift=bp).view(B, N, -1)


def _sa(dev, C, k, x, idx, relu_out=False, out=None, st=None):
    from houv_amd import ops
    Wp, bp, w = _weights(dev, cases.sa_state(C, k) if st is None else st)
    xd = x if torch.is_tensor(x) else T(x).to(dev)
    return ops.sa_attn(_project(xd, Wp, bp), xd, T(idx).to(dev), *w, relu_out=relu_out, out=out)


@pytest.mark.parametrize("N", SA_N)
@pytest.mark.parametrize("C", cases.SA_C)
def test_sa_attn_vs_float64(dev, C, N):
    for B in (1, 3):
        for k in (SA_K if B == 3 else (16,)):
            if k > N:
                continue
            want, err32 = cases.sa_expected(B, N, C, k)
            got = _sa(dev, C, k, *cases.sa_case(B, N, C, k)).cpu().numpy()
            assert got.shape == (B, N, C)
            _check(got, want, err32, f"C={C} N={N} B={B} k={k}")


@pytest.mark.parametrize("kind", ["self", "repeat", "last"])
@pytest.mark.parametrize("C", cases.SA_C)
def test_sa_attn_neighbour_patterns(dev, C, kind):
    B, N, k = 2, 65, 16
    x, idx = cases.sa_case(B, N, C, k, kind)
    want, err32 = cases.sa_expected(B, N, C, k, kind)
    got = _sa(dev, C, k, x, idx).cpu().numpy()
    _check(got, want, err32, f"{kind} C={C}")
    if kind == "last":
        # the far point, listed last, carries the attention branch: without it the result is another one
        near = cases.sa_host(cases.sa_state(C, k), x, np.where(np.arange(k) == k - 1, np.arange(N)[None, :, None], idx), np.float64)
        assert np.abs(near - want).max() > 1000 * max(err32, 1e-7)
    relu = _sa(dev, C, k, x, idx, relu_out=True).cpu().numpy()
    assert (got < 0).any() and np.array_equal(relu, np.maximum(got, 0))


@pytest.mark.parametrize("C", cases.SA_C)
def test_sa_attn_out_of_range_indices_are_clamped(dev, C):
    B, N, k = 2, 40, 10
    x, wild = cases.sa_case(B, N, C, k, "wild")
    assert (wild < 0).any() and (wild >= N).any()
    got = _sa(dev, C, k, x, wild).cpu().numpy()
    want = _sa(dev, C, k, x, np.clip(wild, 0, N - 1)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    _check(got, *cases.sa_expected(B, N, C, k, "wild"), f"wild C={C}")


@pytest.mark.parametrize("C", cases.SA_C)
def test_sa_attn_on_slices_of_wider_buffers_and_in_place(dev, C):
    """P, x and out as column slices (ldp, ldx, ldo wider than their widths) of buffers filled with a sentinel: the result is
    the contiguous call's bit for bit and every other column keeps the sentinel.  Then out = x itself."""
    from houv_amd import ops
    B, N, k = 3, 130, 16
    x, idx = cases.sa_case(B, N, C, k)
    Wp, bp, w = _weights(dev, cases.sa_state(C, k))
    xd, idxd = T(x).to(dev), T(idx).to(dev)
    P = _project(xd, Wp, bp)
    plain = ops.sa_attn(P, xd, idxd, *w)
    wp = P.shape[2]
    Pw = torch.full((B, N, wp + 8), -7.0, device=dev)
    Pw[..., 4:4 + wp] = P
    xo = torch.full((B, N, 2 * C + 7), -7.0, device=dev)
    xo[..., 3:3 + C] = xd
    got = ops.sa_attn(Pw[..., 4:4 + wp], xo[..., 3:3 + C], idxd, *w, out=xo[..., C + 5:2 * C + 5])
    assert got.data_ptr() == xo[..., C + 5:].data_ptr()
    full = xo.cpu().numpy()
    assert np.array_equal(full[..., C + 5:2 * C + 5].view(np.int32), plain.cpu().numpy().view(np.int32))
    assert np.array_equal(full[..., 3:3 + C], x)
    assert (full[..., :3] == -7).all() and (full[..., 3 + C:C + 5] == -7).all() and (full[..., 2 * C + 5:] == -7).all()
    assert (Pw[..., :4] == -7).all() and (Pw[..., 4 + wp:] == -7).all()
    same = xd.clone()
    ops.sa_attn(P, same, idxd, *w, out=same)
    assert torch.equal(same, plain)


@pytest.mark.parametrize("C", cases.SA_C)
def test_sa_attn_zero_conv_out_is_x_plus_bias_exactly(dev, C):
    B, N, k = 2, 70, 10
    x, idx = cases.sa_case(B, N, C, k)
    st = dict(cases.sa_state(C, k))
    st["conv_out.weight"] = np.zeros_like(st["conv_out.weight"])
    got = _sa(dev, C, k, x, idx, st=st).cpu().numpy()
    want = x + st["conv_out.bias"][None, None, :]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_sa_attn_refusals(dev):
    from houv_amd import _lib
    lib = _lib.load()
    C, N, k = 64, 40, 16
    P = torch.zeros((2, N, 32), device=dev)
    x = torch.zeros((2, N, 80), device=dev)
    idx = torch.zeros((2, N, 32), dtype=torch.int32, device=dev)
    w = torch.zeros(512 * 128, device=dev)
    out = torch.zeros((2, N, 80), device=dev)

    def call(C=C, N=N, k=k, B=2, ldp=32, ldx=80, ldo=80, P=P, x=x, idx=idx, Ww1=w, bout=w, out=out):
        p = _lib.ptr
        return lib.houv_sa_attn(p(P), ldp, p(x), ldx, p(idx), B, N, C, k, p(Ww1), p(w), p(w), p(w), p(bout), 0, p(out), ldo, None)
    for kw, msg in ((dict(C=32), "C=32"), (dict(C=96), "C=96"), (dict(C=1024), "C=1024"), (dict(k=33), "k=33"), (dict(k=0), "k=0"),
                    (dict(N=8, k=9), "N=8"), (dict(N=16385), "N=16385"), (dict(B=65536), "B=65536"), (dict(ldp=23), "ldp=23"),
                    (dict(ldp=26), "ldp=26"), (dict(ldx=63), "ldx=63"), (dict(ldo=63), "ldo=63"), (dict(P=None), "P is a null pointer"),
                    (dict(x=None), "x is a null pointer"), (dict(idx=None), "idx is a null pointer"),
                    (dict(Ww1=None), "Ww1 is a null pointer"), (dict(bout=None), "bout is a null pointer"),
                    (dict(out=None), "out is a null pointer"), (dict(P=P.view(-1)[1:]), "P is not aligned"),
                    (dict(out=x, ldo=64), "out is x but ldo=64")):
        assert call(**kw) == 0 and "houv_sa_attn" in _lib.last_error() and msg in _lib.last_error(), (kw, _lib.last_error())
    assert call() == 1 and call(out=x) == 1 and call(B=0, P=None) == 1
    torch.cuda.synchronize()


def test_torch_op_is_registered(dev):
    from houv_amd import ops
    ops.register_torch_ops()
    C, k = 64, 10
    x, idx = cases.sa_case(1, 40, C, k)
    Wp, bp, w = _weights(dev, cases.sa_state(C, k))
    xd, idxd = T(x).to(dev), T(idx).to(dev)
    P = _project(xd, Wp, bp)
    assert torch.equal(torch.ops.houv.sa_attn(P, xd, idxd, *w, True), ops.sa_attn(P, xd, idxd, *w, relu_out=True))


# ------------------------------------------------------------------------------------------- the reference's layers, on the device
def _load(module, st, dev):
    module.load_state_dict({k: T(v) for k, v in st.items()}, strict=True)
    return module.to(dev).eval()


@pytest.mark.parametrize("k", cases.LAYER_K)
@pytest.mark.parametrize("C", cases.SA_C)
def test_sa_module_reproduces_the_reference_layer(dev, golden, C, k):
    from houv_amd.models.vrcnet import SA_module
    g = golden("g27_vrcnet.npz")
    key = f"sa{C}_{k}"
    net = _load(SA_module(C, C // 16, C // 4, C, 8, k), cases.sa_state(C, k), dev)
    x, idx = T(g[key + "_x"]).to(dev), T(g[key + "_idx"].astype(np.int32)).to(dev)
    got = net.forward_rows(x, idx).cpu().numpy()
    f64 = cases.sa_host(cases.sa_state(C, k), g[key + "_x"], g[key + "_idx"], np.float64)
    assert np.abs(f64 - g[key]).max() <= 4 * float(g["spread_" + key])    # the restatement is the reference's (test_vrcnet_host.py)
    _check(got, f64, float(g["spread_" + key]), key)
    ref_err = float(np.abs(got - g[key]).max())
    print(key, "device vs the reference's float32 forward", ref_err)
    assert ref_err <= 8 * float(g["spread_" + key])                       # both sides within 4x of float64
    # the reference's layout: [x (B,C,1,N), idx] -> [out (B,C,1,N), idx]
    out4, _ = net([x.transpose(1, 2).unsqueeze(2).contiguous(), idx.long()])
    assert np.array_equal(out4.squeeze(2).transpose(1, 2).cpu().numpy(), got)


def test_sk_sa_module_reproduces_the_reference_layer(dev, golden):
    from houv_amd.models.vrcnet import SK_SA_module
    g = golden("g27_vrcnet.npz")
    C = 64
    net = _load(SK_SA_module(C, C // 16, C // 4, C, 8, list(cases.SK_KS)), cases.sk_state(), dev)
    x = T(g["sk_x"]).to(dev)
    idxs = [T(g[f"sk_idx{i}"].astype(np.int32)).to(dev) for i in range(len(cases.SK_KS))]
    got = net.forward_rows(x, idxs).cpu().numpy()
    cols = np.ascontiguousarray(np.swapaxes(g["sk_x"], 1, 2))[:, :, None, :]
    f64 = cases.host.sk_sa_module(cases.sk_state(), "", cols, [g[f"sk_idx{i}"].astype(np.int64) for i in range(len(idxs))], np.float64)
    f64 = np.ascontiguousarray(np.swapaxes(f64[:, :, 0], 1, 2))
    assert np.abs(f64 - g["sk"]).max() <= 4 * float(g["spread_sk"])
    _check(got, f64, float(g["spread_sk"]), "SK_SA_module [10, 20]")
    assert (got >= 0).all()
    # one list: relu(SA_module(x)), fc / fcs not evaluated
    W = cases.vrcnet_weights
    one = _load(SK_SA_module(C, C // 16, C // 4, C, 8, [10]), W.make_state(W.sk_spec("", C, (10,)), 5), dev)
    alone = one.sams[0].forward_rows(x, idxs[0])
    assert torch.equal(one.forward_rows(x, idxs[:1]), torch.relu(alone))
