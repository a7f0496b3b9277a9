"""GPU: houv_sa_attn_backward through ops.sa_attn_backward.  Each of gP, gWw1, gWw2, gbw2 and ro is
compared with the float64 NumPy restatement in the reference's materialising form (tests/vrcnet_grad_host.py), within 4x the
float32 restatement's own maximum error on the same inputs (printed per case); where that error is 0 the results must be equal.
Random inputs keep the float64 ReLU inputs >= 1e-5 from 0 (asserted), so no mask can differ between the precisions.  Fixture (a)
of g30_vrcnet_grad_a*.npz, the REAL reference's SA_module gradients, goes through models.vrcnet._SAAttnFunction."""
import ctypes

import numpy as np
import pytest
import torch

import vrcnet_grad_cases as gc
import vrcnet_grad_host as gh

pytestmark = pytest.mark.gpu
T = torch.tensor
SIZES = (1, 5, 63, 64, 65, 127, 128, 129, 130)          # the workgroup of 128 points and the wave of 64, one below and above
KB = ((1, 1), (4, 3), (16, 1), (20, 3), (32, 1))        # (k, B); at C = 512, k = 20 and 32 take conv_w[1] in two chunks of slots
WNAMES = ("Ww1", "Ww2", "bw2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _run(dev, c, pad=0):
    """-> dict of the five results as NumPy arrays; pad > 0 (a multiple of 8): P, G and gP are column slices of wider buffers whose
    other columns must come back untouched."""
    from houv_amd import ops
    B, N, wp = c["P"].shape
    mid = c["G"].shape[2]

    def wide(a, width):
        buf = torch.full((B, N, width + pad), -77.0, dtype=torch.float32, device=dev)
        view = buf[:, :, pad // 2:pad // 2 + width]
        if a is not None:
            view.copy_(T(a))
        return buf, view
    Pb, P = wide(c["P"], wp)
    Gb, G = wide(c["G"], mid)
    gPb, gP = wide(None, wp)
    res = ops.sa_attn_backward(P, T(c["idx"]).to(dev), *(T(c[n]).to(dev) for n in WNAMES), G, gP=gP)
    assert res["gP"] is gP
    if pad:
        for buf, width in ((Pb, wp), (Gb, mid), (gPb, wp)):
            keep = torch.ones(width + pad, dtype=torch.bool)
            keep[pad // 2:pad // 2 + width] = False
            assert bool((buf[:, :, keep.to(dev)] == -77.0).all()), "a column outside the slice was written"
    return {n: res[n].contiguous().cpu().numpy() for n in gh.OP_GRADS}


def _check(c, got, label=""):
    r64 = gh.sa_attn_backward(**c)
    r32 = gh.sa_attn_backward(**c, dtype=np.float32)
    assert min(np.abs(r64[n]).min() for n in ("t", "pre", "o")) >= 1e-5, "a float64 ReLU input is within 1e-5 of 0"
    ratios = {}
    for n in gh.OP_GRADS:
        own = np.abs(r32[n] - r64[n]).max()
        err = np.abs(got[n] - r64[n]).max()
        ratios[n] = err / own if own > 0 else (0.0 if err == 0 else np.inf)
        print(f"{label} {n}: kernel error {err:.3e}, float32 restatement {own:.3e}, ratio {ratios[n]:.2f}")
    for n in gh.OP_GRADS:
        assert ratios[n] <= 4, (label, n, ratios)
    return ratios


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("C", (64, 128, 256, 512))
def test_backward_parity_at_every_size(dev, C, N):
    for k, B in KB:
        if k > N:
            continue
        c = gh.op_case(1000 + N, B, N, C, k)
        _check(c, _run(dev, c), label=f"C={C} N={N} k={k} B={B}")


@pytest.mark.parametrize("C", (64, 128, 256, 512))
def test_ro_carries_the_forward_chain_bits(dev, C):
    """With Wout = [I; 0], bout = 0 and x = 0 houv_sa_attn's output columns 0 .. mid-1 are relu(o) exactly (the other products of
    the chain are 0 * finite), so ro must equal the forward kernel's own relu(o), not merely lie close to it."""
    from houv_amd import ops
    N, k, B = 130, 20, 2
    mid = C // 4
    c = gh.op_case(61, B, N, C, k)
    Wout = torch.zeros((C, mid), dtype=torch.float32, device=dev)
    Wout[:mid] = torch.eye(mid, device=dev)
    zero = torch.zeros((B, N, C), dtype=torch.float32, device=dev)
    out = ops.sa_attn(T(c["P"]).to(dev), zero, T(c["idx"]).to(dev), *(T(c[n]).to(dev) for n in WNAMES), Wout, zero[0, 0].clone())
    got = _run(dev, c)
    assert np.array_equal(out[:, :, :mid].cpu().numpy(), got["ro"])              # as values: -0 == +0


def _knn_lists(dev, x, k):
    from houv_amd import ops
    return ops.knn_feat(T(x).to(dev), k).cpu().numpy()


@pytest.mark.parametrize("C", (64, 512))
def test_edge_lists(dev, C):
    """Lists from knn_feat, repeats, out-of-range indices (the gradient lands on the clamped row), a hub every point lists and a
    point nobody lists, each with rows wider than the tensors and sentinels around them."""
    N, k, B = 130, 16, 2
    rel = C // 16
    P0 = gh.op_case(21, B, N, C, k)["P"]
    lists = {"knn_feat": _knn_lists(dev, P0[:, :, :rel], k),
             "repeats": np.repeat(np.random.default_rng(1).integers(0, N, (B, N, 1)), k, axis=2).astype(np.int32),
             "out_of_range": np.random.default_rng(2).integers(-N, 2 * N, (B, N, k)).astype(np.int32),
             "hub": np.concatenate([np.full((B, N, 1), 7, np.int32), np.random.default_rng(3).integers(0, N - 1, (B, N, k - 1)).astype(np.int32)], 2)}
    assert not (lists["hub"] == N - 1).any() and (lists["out_of_range"] < 0).any() and (lists["out_of_range"] >= N).any()
    assert (lists["knn_feat"][:, :, 0] == np.arange(N)).all()
    for name, idx in lists.items():
        c = gh.op_case(21, B, N, C, k, idx=idx)
        got = _run(dev, c, pad=8)
        _check(c, got, label=f"{name} C={C}")
        if name == "hub":                                                         # nobody lists the last point: no x2 / x3 gradient
            assert not got["gP"][:, N - 1, rel:].any() and got["gP"][:, 7, rel:].any()
        if name == "out_of_range":
            got2 = _run(dev, dict(c, idx=np.clip(idx, 0, N - 1)))
            assert all(np.array_equal(_bits(got[n]), _bits(got2[n])) for n in gh.OP_GRADS)


@pytest.mark.parametrize("C", (64, 128, 256, 512))
def test_zero_G_gives_exact_zeros_and_two_calls_give_the_same_bits(dev, C):
    c = gh.op_case(31, 3, 129, C, 20)
    a, b = _run(dev, c), _run(dev, c)
    assert all(np.array_equal(_bits(a[n]), _bits(b[n])) for n in gh.OP_GRADS)
    c["G"][:] = 0
    z = _run(dev, c)
    assert all(not z[n].any() for n in ("gP", "gWw1", "gWw2", "gbw2")) and np.array_equal(_bits(z["ro"]), _bits(a["ro"]))


def test_workspace_and_argument_refusals(dev):
    from houv_amd import _lib, ops
    lib = _lib.load()
    C, N, k, B = 64, 40, 4, 2
    rel, mid, m = C // 16, C // 4, C // 32
    wp = 2 * rel + mid
    c = gh.op_case(51, B, N, C, k)
    t = {n: T(c[n]).to(dev) for n in c}
    nbytes = lib.houv_sa_attn_backward_workspace_bytes(B, N, C, k)
    assert nbytes > 0 and nbytes % 16 == 0
    for bad in ((B, N, 65, k), (B, N, C, 33), (B, N, C, 0), (B, 3, C, k), (B, 16385, C, k), (65536, N, C, k), (0, N, C, k)):
        assert lib.houv_sa_attn_backward_workspace_bytes(*bad) == 0, bad
    # the memory rule at the first level of the shipped cfg: a handful of per-point rows and three int32 arrays per edge, nothing
    # of extent N k C, and every single buffer far below N k mid
    B1, N1, k1 = 24, 3072, 16
    big = lib.houv_sa_attn_backward_workspace_bytes(B1, N1, 64, k1)
    assert big < 4 * B1 * N1 * (6 * (rel * (k1 + 1) + k1 * m + 2 * mid) + 3 * k1 + 2) and big < 4 * B1 * N1 * k1 * C
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    g = dict(gWw1=torch.empty_like(t["Ww1"]), gWw2=torch.empty_like(t["Ww2"]), gbw2=torch.empty_like(t["bw2"]))
    gP, ro = torch.empty_like(t["P"]), torch.empty_like(t["G"])
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())

    def call(**kw):
        a = dict(P=t["P"], ldp=wp, idx=t["idx"], B=B, N=N, C=C, k=k, Ww1=t["Ww1"], Ww2=t["Ww2"], bw2=t["bw2"], G=t["G"], ldg=mid,
                 gP=gP, ldgp=wp, ro=ro, ldro=mid, gWw1=g["gWw1"], ws=ws, nbytes=nbytes)
        a.update(kw)
        return lib.houv_sa_attn_backward(p(a["P"]), a["ldp"], p(a["idx"]), a["B"], a["N"], a["C"], a["k"], p(a["Ww1"]), p(a["Ww2"]),
                                         p(a["bw2"]), p(a["G"]), a["ldg"], p(a["gP"]), a["ldgp"], p(a["ro"]), a["ldro"],
                                         p(a["gWw1"]), p(g["gWw2"]), p(g["gbw2"]), p(a["ws"]), a["nbytes"], None)
    assert call() == 1
    for kw, msg in [(dict(C=65), "C=65 has no kernel: 64, 128, 256 and 512 are served"), (dict(k=0), "k=0 neighbours per point: 1..32"),
                    (dict(k=33), "k=33 neighbours per point"), (dict(N=3), "N=3 points with k=4"), (dict(N=16385), "N=16385 points"),
                    (dict(B=65536), "B=65536 clouds"), (dict(ldp=wp - 4), "ldp="), (dict(ldp=wp + 2), "ldp="), (dict(ldg=mid - 1), "ldg="),
                    (dict(ldgp=wp - 1), "ldgp="), (dict(ldro=mid - 1), "ldro="), (dict(P=None), "P is a null pointer"),
                    (dict(idx=None), "idx is a null pointer"), (dict(Ww1=None), "Ww1 is a null pointer"), (dict(G=None), "G is a null pointer"),
                    (dict(gP=None), "gP is a null pointer"), (dict(ro=None), "ro is a null pointer"),
                    (dict(gWw1=None), "gWw1 is a null pointer"), (dict(ws=None), "workspace of"), (dict(nbytes=nbytes - 16), "workspace of")]:
        assert call(**kw) == 0 and _lib.last_error().startswith("houv_sa_attn_backward: ") and msg in _lib.last_error(), (kw, _lib.last_error())
    # B = 0 writes zero weight gradients and needs no workspace
    for n in g:
        g[n].fill_(3.0)
    assert call(B=0, ws=None, nbytes=0, P=None, G=None, gP=None, ro=None) == 1
    torch.cuda.synchronize()
    assert all(not g[n].any() for n in g)
    with pytest.raises(_lib.HouvHipError, match="G must be"):
        ops.sa_attn_backward(t["P"], t["idx"], t["Ww1"], t["Ww2"], t["bw2"], t["G"][:, :, :mid - 1])


def _module_grads(dev, state, x, idx, G, relu_out):
    """models.vrcnet._SAAttnFunction behind the projection GEMM, as SA_module(trainable=True) calls it -> {name: gradient}."""
    from houv_amd.model_utils_completion import _LinearRowsFunction
    from houv_amd.models.vrcnet import _SAAttnFunction
    leaf = lambda a: T(np.ascontiguousarray(a)).to(dev).requires_grad_(True)
    B, C, _, N = x.shape
    p = {n: leaf(v.reshape(v.shape[0], -1) if v.ndim == 4 else v) for n, v in state.items()}
    rows = leaf(np.swapaxes(x[:, :, 0], 1, 2))
    W = torch.cat((p["conv1.weight"], p["conv2.weight"], p["conv3.weight"]), 0)
    b = torch.cat((p["conv1.bias"], p["conv2.bias"], p["conv3.bias"]), 0)
    P = _LinearRowsFunction.apply(torch.relu(rows).reshape(-1, C), W, b, False).view(B, N, -1)
    out = _SAAttnFunction.apply(P, rows, T(idx).int().to(dev), p["conv_w.1.weight"], p["conv_w.3.weight"], p["conv_w.3.bias"],
                                p["conv_out.weight"], p["conv_out.bias"], relu_out)
    (out * T(np.ascontiguousarray(np.swapaxes(G[:, :, 0], 1, 2))).to(dev)).sum().backward()
    grads = {n: t.grad.cpu().numpy().reshape(state[n].shape) for n, t in p.items()}
    grads["x"] = np.swapaxes(rows.grad.cpu().numpy(), 1, 2)[:, :, None, :]
    return out.detach().cpu().numpy(), grads


@pytest.mark.parametrize("k", gc.A_K)
@pytest.mark.parametrize("C", gc.A_C)
def test_reference_sa_module_gradients_through_the_function(dev, golden, C, k):
    """Fixture (a): the REFERENCE's SA_module (float32 autograd) through _SAAttnFunction: every stored entry of every parameter
    gradient and of gx within 4x the stored float32-vs-float64 spread of the float64 restatement."""
    g = golden(gc.file_a(C))
    key = f"sa{C}_{k}"
    state, x, idx, G = gc.load_a(g, key)
    _, grads = _module_grads(dev, state, x, idx, G, False)
    worst = 0.0
    for n in list(state) + ["x"]:
        at = g[f"{key}_at_{n}"].astype(np.int64)
        spread = float(g[f"{key}_spread_{n}"])
        err = float(np.abs(grads[n].reshape(-1)[at] - g[f"{key}_f64_{n}"]).max())
        print(f"{key} {n}: error {err:.3e}, spread {spread:.3e}")
        worst = max(worst, err / spread)
        assert err <= 4 * spread, (key, n, err, spread)
    print(f"{key}: largest error {worst:.2f}x the spread")


@pytest.mark.parametrize("C", (64, 256))
def test_function_with_relu_out_against_the_restatement(dev, C):
    """SK_SA_module's branch: relu_out = True.  Output bit-equal to ops.sa_attn's, gradients within 4x the float32 restatement's
    own error against float64."""
    k = 10
    for seed in range(16):
        state, x, idx, G = gc.inputs_a(C, k, 100 + seed)
        kinks = []
        st64 = {n: np.asarray(v, np.float64) for n, v in state.items()}
        out64, bw64 = gh.sa_module(st64, "", x, idx, True, np.float64, kinks)
        if gh.margin(kinks) >= 1e-5:
            break
    assert gh.margin(kinks) >= 1e-5
    gx64, g64 = bw64(G)
    gx32, g32 = gh.sa_module(state, "", x, idx, True, np.float32)[1](G)
    out, grads = _module_grads(dev, state, x, idx, G, True)
    assert (out >= 0).all() and (out == 0).any()
    r64, r32 = dict(g64, x=gx64), dict(g32, x=gx32)
    for n in r64:
        own = np.abs(r32[n] - r64[n]).max()
        err = np.abs(grads[n] - r64[n]).max()
        print(f"relu_out C={C} {n}: kernel error {err:.3e}, float32 restatement {own:.3e}, ratio {err / own:.2f}")
        assert err <= 4 * own, (n, err, own)
