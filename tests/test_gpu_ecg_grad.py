"""GPU: houv_dense_conv_arg and houv_dense_conv_backward.  `out` must carry houv_dense_conv's bits and
every arg must be a maximum of its column in float64 to within the float32 spread.  Each of the seven gradients is compared with
the float64 NumPy restatement in the reference's materialising form (tests/ecg_grad_host.py) GIVEN the kernel's arg, within 4x
the float32 restatement's own maximum error on the same inputs (printed per case); where that error is 0 the results must be
equal.  Random inputs keep the float64 ReLU inputs >= 1e-5 from 0 (asserted), so no mask can differ between the precisions."""
import ctypes

import numpy as np
import pytest
import torch

import ecg_grad_host as gh

pytestmark = pytest.mark.gpu
T = torch.tensor
G = gh.G
SIZES = (1, 3, 5, 63, 64, 65, 127, 128, 129, 130)      # the workgroup of 128 points and the wave of 64, one below and above
KB = ((1, 1), (4, 3), (16, 1), (20, 3), (32, 1))        # (k, B)
WNAMES = ("W0", "b0", "W1", "b1", "W2", "b2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _run(dev, c, relu_out=False, pad=0):
    """-> (out, arg, dict of gradients) as NumPy arrays; pad > 0: x, out, gout and gx are column slices of wider buffers whose
    other columns must come back untouched."""
    from houv_amd import ops
    B, N, C = c["x"].shape
    w = [T(c[n]).to(dev) for n in WNAMES]
    idx = T(c["idx"]).to(dev)

    def wide(a, width):
        buf = torch.full((B, N, width + pad), -77.0, dtype=torch.float32, device=dev)
        view = buf[:, :, pad // 2:pad // 2 + width]
        if a is not None:
            view.copy_(T(a))
        return buf, view
    xb, x = wide(c["x"], C)
    ob, out = wide(None, C + 3 * G)
    gb, gout = wide(c["gout"], C + 3 * G)
    gxb, gx = wide(None, C)
    plain = ops.dense_conv(x, idx, *w, relu_out=relu_out)
    out2, arg = ops.dense_conv_arg(x, idx, *w, relu_out=relu_out, out=out)
    assert out2 is out and np.array_equal(_bits(out.contiguous()), _bits(plain)), "out differs from houv_dense_conv's bits"
    res = ops.dense_conv_backward(x, idx, *w, arg, gout, out=out if relu_out else None, relu_out=relu_out, gx=gx)
    if pad:
        for buf, width in ((xb, C), (ob, C + 3 * G), (gb, C + 3 * G), (gxb, C)):
            keep = torch.ones(width + pad, dtype=torch.bool)
            keep[pad // 2:pad // 2 + width] = False
            assert bool((buf[:, :, keep.to(dev)] == -77.0).all()), "a column outside the slice was written"
    return out.contiguous().cpu().numpy(), arg.cpu().numpy(), {n: res[n].contiguous().cpu().numpy() for n in gh.GRADS}


def _check(c, out, arg, grads, relu_out=False, label=""):
    """arg valid in float64; every gradient within 4x the float32 restatement's error of the float64 one, given arg."""
    B, N, C = c["x"].shape
    k = c["idx"].shape[2]
    r64 = gh.dense_conv_backward(**c, relu_out=relu_out, arg=arg)
    r32 = gh.dense_conv_backward(**c, relu_out=relu_out, arg=arg, dtype=np.float32)
    assert min(np.abs(r64["z0"]).min(), np.abs(r64["z1"]).min()) >= 1e-5, "a float64 ReLU input is within 1e-5 of 0"
    spread = np.abs(r32["full"] - r64["full"]).max()
    cols = gh.pooled_columns(C)
    full = r64["full"][..., cols]
    assert arg.dtype == np.int8 and arg.min() >= 0 and arg.max() < k
    at = np.take_along_axis(full, arg.astype(np.int64)[:, :, None, :], axis=2)[:, :, 0]
    assert (at >= full.max(2) - 2 * spread).all(), "an arg is not a maximum of its column"
    assert np.abs(out - r64["out"]).max() <= 4 * np.abs(r32["out"] - r64["out"]).max()
    ratios = {}
    for n in gh.GRADS:
        own = np.abs(r32[n] - r64[n]).max()
        err = np.abs(grads[n] - r64[n]).max()
        ratios[n] = err / own if own > 0 else (0.0 if err == 0 else np.inf)
        print(f"{label} {n}: kernel error {err:.3e}, float32 restatement {own:.3e}, ratio {ratios[n]:.2f}")
    for n in gh.GRADS:
        assert ratios[n] <= 4, (label, n, ratios)
    return ratios


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("C", (24, 48))
def test_arg_and_backward_parity_at_every_size(dev, C, N):
    for k, B in KB:
        c = gh.random_case(1000 + N, B, N, C, k)
        relu_out = (k in (4, 20))
        out, arg, grads = _run(dev, c, relu_out=relu_out)
        _check(c, out, arg, grads, relu_out, label=f"C={C} N={N} k={k} B={B}")


@pytest.mark.parametrize("C", (24, 48))
def test_all_self_lists_give_arg_zero_and_last_neighbour_gives_k_minus_one(dev, C):
    N, k = 65, 16
    c = gh.random_case(7, 2, N, C, k, idx=np.broadcast_to(np.arange(N, dtype=np.int32)[None, :, None], (2, N, k)).copy())
    out, arg, grads = _run(dev, c)
    assert (arg == 0).all()                                                       # every candidate ties: the lowest slot
    _check(c, out, arg, grads, label=f"self C={C}")
    # the maximum at the last neighbour only: the first k - 1 slots list the point itself (y0 = s1 = s2 = 0 under these weights),
    # the last slot lists the one point that differs, which makes all three positive
    from houv_amd import ops
    x = np.zeros((1, N, C), np.float32)
    x[0, N - 1] = 1.0
    idx = np.broadcast_to(np.arange(N, dtype=np.int32)[None, :, None], (1, N, k)).copy()
    idx[0, :N - 1, k - 1] = N - 1
    W0 = np.zeros((G, 2 * C), np.float32); W0[:, C:] = 1.0
    eye = lambda n: np.concatenate([np.eye(G, dtype=np.float32), np.zeros((G, n - G), np.float32)], 1)
    W1, W2 = eye(G + C), eye(2 * G + C)
    zero = np.zeros(G, np.float32)
    args = [T(a).to(dev) for a in (W0, zero, W1, zero, W2, zero)]
    _, a = ops.dense_conv_arg(T(x).to(dev), T(idx).to(dev), *args)
    assert (a.cpu().numpy()[0, :N - 1] == k - 1).all() and (a.cpu().numpy()[0, N - 1] == 0).all()


def _knn_lists(dev, x, k):
    from houv_amd import ops
    return ops.knn_feat(T(x).to(dev), k).cpu().numpy()


@pytest.mark.parametrize("C", (24, 48))
def test_edge_lists(dev, C):
    """Lists from knn_feat, repeats, out-of-range indices (the gradient lands on the clamped row), a hub every point lists and a
    point nobody lists, each with rows wider than the tensors and sentinels around them."""
    N, k, B = 130, 16, 2
    lists = {"knn_feat": lambda x: _knn_lists(dev, x, k),
             "repeats": np.repeat(np.random.default_rng(1).integers(0, N, (B, N, 1)), k, axis=2).astype(np.int32),
             "out_of_range": np.random.default_rng(2).integers(-N, 2 * N, (B, N, k)).astype(np.int32),
             "hub": np.concatenate([np.full((B, N, 1), 7, np.int32), np.random.default_rng(3).integers(0, N - 1, (B, N, k - 1)).astype(np.int32)], 2)}
    assert not (lists["hub"] == N - 1).any() and (lists["out_of_range"] < 0).any() and (lists["out_of_range"] >= N).any()
    for name, idx in lists.items():
        c = gh.random_case(21, B, N, C, k, idx=idx)
        idx = c["idx"]
        if name == "knn_feat":
            assert np.array_equal(idx, _knn_lists(dev, c["x"], k)) and (idx[:, :, 0] == np.arange(N)).all()
        relu_out = name in ("knn_feat", "hub")
        out, arg, grads = _run(dev, c, relu_out=relu_out, pad=6)
        _check(c, out, arg, grads, relu_out, label=f"{name} C={C}")
        if name == "out_of_range":
            clamped = dict(c, idx=np.clip(idx, 0, N - 1))
            out2, arg2, grads2 = _run(dev, clamped)
            assert np.array_equal(arg, arg2) and all(np.array_equal(_bits(T(grads[n])), _bits(T(grads2[n]))) for n in gh.GRADS)


@pytest.mark.parametrize("C", (24, 48))
def test_zero_gout_gives_exact_zeros_and_two_calls_give_the_same_bits(dev, C):
    c = gh.random_case(31, 3, 129, C, 20)
    a = _run(dev, c, relu_out=True)
    b = _run(dev, c, relu_out=True)
    assert np.array_equal(a[1], b[1]) and all(np.array_equal(_bits(T(a[2][n])), _bits(T(b[2][n]))) for n in gh.GRADS)
    c["gout"][:] = 0
    _, _, grads = _run(dev, c, relu_out=True)
    assert all(not grads[n].any() for n in gh.GRADS)


def test_all_nan_column_reports_minus_one_and_sends_no_gradient(dev):
    C, o = 24, 5
    c = gh.random_case(41, 2, 65, C, 4)
    nan = dict(c, b2=c["b2"].copy())
    nan["b2"][o] = np.nan                                                         # s2[:, o] is NaN for every neighbour
    from houv_amd import ops
    args = [T(nan[n]).to(dev) for n in WNAMES]
    x, idx, gout = (T(nan[n]).to(dev) for n in ("x", "idx", "gout"))
    out, arg = ops.dense_conv_arg(x, idx, *args)
    arg_h = arg.cpu().numpy()
    assert (arg_h[:, :, 2 * G + o] == -1).all() and np.isneginf(out.cpu().numpy()[:, :, 2 * G + C + o]).all()
    assert (np.delete(arg_h, 2 * G + o, axis=2) >= 0).all()
    res = ops.dense_conv_backward(x, idx, *args, arg, gout)
    grads = {n: res[n].cpu().numpy() for n in gh.GRADS}
    assert all(np.isfinite(grads[n]).all() for n in gh.GRADS) and grads["gb2"][o] == 0 and not grads["gW2"][o].any()
    r64 = gh.dense_conv_backward(**c, arg=arg_h)                                  # nothing else depends on s2: b2[o] = its old value
    r32 = gh.dense_conv_backward(**c, arg=arg_h, dtype=np.float32)
    for n in gh.GRADS:
        assert np.abs(grads[n] - r64[n]).max() <= 4 * np.abs(r32[n] - r64[n]).max(), n


def test_workspace_and_argument_refusals(dev):
    from houv_amd import _lib, ops
    lib = _lib.load()
    C, N, k, B = 24, 40, 4, 2
    c = gh.random_case(51, B, N, C, k)
    t = {n: T(c[n]).to(dev) for n in c}
    out, arg = ops.dense_conv_arg(t["x"], t["idx"], *(t[n] for n in WNAMES))
    nbytes = lib.houv_dense_conv_backward_workspace_bytes(B, N, C, k)
    assert nbytes >= 4 * B * N * k * G and nbytes % 16 == 0
    assert lib.houv_dense_conv_backward_workspace_bytes(B, N, 25, k) == 0 and lib.houv_dense_conv_backward_workspace_bytes(B, N, C, 33) == 0
    # the one [B, N, k, .] tensor is 24 floats wide: the rest of the workspace is small next to it at the network's shape
    big = lib.houv_dense_conv_backward_workspace_bytes(32, 3072, 24, 16)
    assert big < 1.5 * 4 * 32 * 3072 * 16 * G
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    g = {n: torch.empty_like(t[n]) for n in WNAMES}
    gx = torch.empty_like(t["x"])
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())

    def call(fn="backward", **kw):
        a = dict(x=t["x"], ldx=C, idx=t["idx"], B=B, N=N, C=C, k=k, relu_out=0, arg=arg, out=None, ldo=0, gout=t["gout"], ldg=C + 72,
                 gx=gx, ldgx=C, ws=ws, nbytes=nbytes, W0=t["W0"])
        a.update(kw)
        w = [p(a["W0"])] + [p(t[n]) for n in WNAMES[1:]]
        if fn == "arg":
            return lib.houv_dense_conv_arg(p(a["x"]), a["ldx"], p(a["idx"]), a["B"], a["N"], a["C"], a["k"], *w, a["relu_out"], p(out),
                                           C + 72 if a["ldo"] == 0 else a["ldo"], p(a["arg"]), None)
        return lib.houv_dense_conv_backward(p(a["x"]), a["ldx"], p(a["idx"]), a["B"], a["N"], a["C"], a["k"], *w, a["relu_out"],
                                            p(a["arg"]), p(a["out"]), a["ldo"], p(a["gout"]), a["ldg"], p(a["gx"]), a["ldgx"],
                                            *(p(g[n]) for n in WNAMES), p(a["ws"]), a["nbytes"], None)
    assert call() == 1
    refusals = [(dict(C=25), "C=25 has no kernel: 24 and 48 are served"), (dict(k=0), "k=0 neighbours per point: 1..32 are served"),
                (dict(k=33), "k=33 neighbours per point"), (dict(B=65536), "bad argument"), (dict(N=0), "bad argument"),
                (dict(ldx=C - 1), "bad argument"), (dict(x=None), "x is a null pointer"), (dict(W0=None), "W0 is a null pointer")]
    for fn, name in (("backward", "houv_dense_conv_backward: "), ("arg", "houv_dense_conv_arg: ")):
        for kw, msg in refusals:
            assert call(fn, **kw) == 0 and _lib.last_error().startswith(name) and msg in _lib.last_error(), (fn, kw, _lib.last_error())
    for kw, msg in [(dict(ws=None), "workspace of"), (dict(nbytes=nbytes - 16), "workspace of"), (dict(ldg=C + 71), "bad argument"),
                    (dict(ldgx=C - 1), "bad argument"), (dict(relu_out=1, ldo=C + 72), "relu_out is set but out is a null pointer"), (dict(relu_out=1, ldo=C + 71, out=out), "bad argument"),
                    (dict(arg=None), "arg is a null pointer"), (dict(gout=None), "gout is a null pointer")]:
        assert call(**kw) == 0 and _lib.last_error().startswith("houv_dense_conv_backward: ") and msg in _lib.last_error(), (kw, _lib.last_error())
    assert call("arg", arg=None) == 0 and "arg is a null pointer" in _lib.last_error()
    # B = 0 writes zero weight gradients and needs no workspace
    for n in WNAMES:
        g[n].fill_(3.0)
    assert call(B=0, ws=None, nbytes=0) == 1
    torch.cuda.synchronize()
    assert all(not g[n].any() for n in WNAMES)
    with pytest.raises(_lib.HouvHipError, match="arg must be int8"):
        ops.dense_conv_backward(t["x"], t["idx"], *(t[n] for n in WNAMES), arg.int(), t["gout"])


CASES_A = [f"c{C}n{N}r{r}" for C in (24, 48) for N in (17, 33) for r in (0, 1)]


@pytest.mark.parametrize("name", CASES_A)
def test_reference_dense_conv_gradients_through_the_function(dev, golden, name):
    """Fixture (a) of g29_ecg_grad.npz: the REFERENCE's Dense_conv (its own k-NN lists, float32 autograd) through
    models.ecg._DenseConvFunction, each gradient within 4x the stored float32-vs-float64 spread of the float64 restatement; the
    reference's own gradients lie within the same bound of it (asserted here on the CPU side as well)."""
    from houv_amd.models.ecg import _DenseConvFunction
    g = golden("g29_ecg_grad.npz")
    shape, relu_out = name[:-2], bool(int(name[-1]))
    leaf = lambda a: T(np.ascontiguousarray(a)).to(dev).requires_grad_(True)
    x = leaf(np.swapaxes(g[f"{name}_x"], 1, 2))
    w = [leaf(g[f"{shape}_{n}"]) for n in WNAMES]
    out, arg = _DenseConvFunction.apply(x, T(g[f"{name}_idx"]).to(dev), *w, relu_out)
    assert not arg.requires_grad and out.requires_grad
    (out * T(np.ascontiguousarray(np.swapaxes(g[f"{name}_G"], 1, 2))).to(dev)).sum().backward()
    got = dict(zip(gh.GRADS, [np.swapaxes(x.grad.cpu().numpy(), 1, 2)] + [t.grad.cpu().numpy() for t in w]))
    for n in gh.GRADS:
        bound = 4 * float(g[f"{name}_spread_{n}"])
        assert np.abs(g[f"{name}_ref_{n}"] - g[f"{name}_f64_{n}"]).max() <= bound, (n, "the reference itself")
        err = np.abs(got[n] - g[f"{name}_f64_{n}"]).max()
        print(f"{name} {n}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, n, err, bound)
