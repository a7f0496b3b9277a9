"""GPU: the IDAM head -- houv_edge_diff bit for bit against NumPy, houv_idam_simmat against the float64
NumPy restatement of its contract (tests/idam_host.py) on the same fp32 inputs, and models.idam.Model against golden vectors from
the reference's idam.py (tests/golden/g24_idam.npz; seeded weights from tests/golden/idam_weights.py) and against the
restatement of the model.  Inputs and the bounds TOL_ROWMAX / TOL_SCORE (4x the
float32 restatement's own error against float64 on these inputs: rowmax 1.26e-06 -> 5.0e-06, scores 1.35e-05 -> 5.4e-05) live
in tests/idam_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

import idam_cases as cases
import idam_host as host

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import idam_weights  # noqa: E402

T = torch.tensor


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _np(t):
    return None if t is None else t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- edge_diff
@pytest.mark.parametrize("B,N,k,C,ldo", cases.EDGE_SHAPES)
def test_edge_diff_bit_for_bit(dev, B, N, k, C, ldo):
    from houv_amd import ops
    x, idx = cases.edge_case(B, N, k, C)
    assert (idx[..., :k] < 0).any() and (idx[..., :k] >= N).any()
    want = host.edge_diff(x, idx, k, ldo)
    got = ops.edge_diff(T(x).to(dev), T(idx).to(dev), k, ldo)
    torch.cuda.synchronize()
    assert got.shape == (B * N * k, ldo)
    assert np.array_equal(_bits(got), want.view(np.int32))
    assert (got[:, C:] == 0).all() and (got.view(B, N, k, ldo)[:, :, 0, :C] == 0).all()     # padding; the point itself
    # the same values from a buffer that is only 4-byte aligned: the element-wise path
    buf = torch.empty(x.size + 1, device=dev)
    xo = buf[1:].view(B, N, C)
    xo.copy_(T(x))
    assert xo.data_ptr() % 16 != 0
    lib_out = ops.edge_diff(xo, T(idx).to(dev), k, ldo)
    assert np.array_equal(_bits(lib_out), want.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- similarity matrix
def _run(dev, case, **want):
    from houv_amd import ops
    src, tgt, es, et, par = case
    return ops.idam_simmat(*(T(a).to(dev) for a in (src, tgt, es, et)), *(T(a).to(dev) for a in par), **want)


@pytest.mark.parametrize("B,Ms,Mt,E", cases.SIM_SHAPES)
def test_idam_simmat_vs_float64(dev, B, Ms, Mt, E):
    case = cases.sim_case(B, Ms, Mt, E)
    y, flagged = cases.sim_yardstick(case)
    a = _run(dev, case, want_scores=True)
    torch.cuda.synchronize()
    rowmax, cidx, corr, scores = (_np(t) for t in a)
    assert rowmax.shape == (B, Ms, 32) and cidx.shape == (B, Ms) and corr.shape == (B, 3, Ms) and scores.shape == (B, Ms, Mt)
    assert np.isfinite(scores).all() and np.isfinite(rowmax).all()             # d = 0 (source 0 == target Mt-1): u = 0, no NaN
    cases.check_sim(rowmax, scores, cidx, corr, case, y, flagged, f"idam_simmat {(B, Ms, Mt, E)}")
    if Mt >= 4:                                                                 # targets 1, 2 and Mt-2 are one point: never the later copies
        assert not np.isin(cidx, [2, Mt - 2]).any()
        assert np.array_equal(scores[..., 1], scores[..., 2]) and np.array_equal(scores[..., 1], scores[..., Mt - 2])
    b = _run(dev, case, want_scores=True)                                       # two calls: identical bits
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


@pytest.mark.parametrize("B,Ms,Mt,E", cases.CLAMP_SHAPES)
@pytest.mark.parametrize("sign", [1, -1])
def test_idam_simmat_whole_rows_at_the_clamp(dev, B, Ms, Mt, E, sign):
    case = cases.sim_case(B, Ms, Mt, E, b4=sign * 1000.0)
    y, flagged = cases.sim_yardstick(case)
    assert (y["scores"] == sign * 20).all() and not flagged.any()
    rowmax, cidx, corr, scores = (_np(t) for t in _run(dev, case, want_scores=True))
    assert (scores == sign * 20).all() and (cidx == 0).all()
    cases.check_sim(rowmax, scores, cidx, corr, case, y, flagged, f"clamp {sign:+d} {(B, Ms, Mt, E)}")


def test_idam_simmat_null_outputs_in_every_combination(dev):
    case = cases.sim_case(2, 33, 31, 64)
    full = _run(dev, case, want_scores=True)
    for mask in range(16):
        w = [bool(mask >> i & 1) for i in range(4)]
        got = _run(dev, case, want_rowmax=w[0], want_idx=w[1], want_corr=w[2], want_scores=w[3])
        for g, f, on in zip(got, full, w):
            assert (g is not None) == on
            if on:
                assert np.array_equal(_bits(g), _bits(f))
    torch.cuda.synchronize()


def test_error_paths(dev):
    from houv_amd import _lib, ops
    lib = _lib.load()
    src, tgt, es, et, par = cases.sim_case(2, 5, 7, 64)
    d = [T(a).to(dev) for a in (src, tgt, es, et)] + [T(a).to(dev) for a in par]
    out = torch.empty(2, 5, 32, device=dev)
    ptrs = [_lib.ptr(t) for t in d]

    def call(Ms=5, Mt=7, E=64, p=ptrs):
        return lib.houv_idam_simmat(*p[:4], 2, Ms, Mt, E, *p[4:], _lib.ptr(out), None, None, None, None)
    assert call() == 1
    for kw, msg in ((dict(Ms=0), "Ms=0"), (dict(Mt=0), "Mt=0"), (dict(E=6), "E=6"), (dict(E=132), "E=132")):
        assert call(**kw) == 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    import ctypes
    off = list(ptrs)
    off[2] = ctypes.c_void_p(d[2].data_ptr() + 4)                               # es on a 4-byte boundary only
    assert call(p=off) == 0 and "16-byte aligned" in _lib.last_error()
    nul = list(ptrs)
    nul[6] = None
    assert call(p=nul) == 0 and "null" in _lib.last_error()
    x, idx = cases.edge_case(1, 12, 12, 3)
    xd, idd = T(x).to(dev), T(idx).to(dev)
    eo = torch.empty(1 * 12 * 12, 4, device=dev)
    assert lib.houv_edge_diff(_lib.ptr(xd), _lib.ptr(idd), 1, 12, 12, 3, 14, 2, _lib.ptr(eo), None) == 0 and "ldo=2" in _lib.last_error()
    assert lib.houv_edge_diff(_lib.ptr(xd), _lib.ptr(idd), 1, 12, 15, 3, 14, 4, _lib.ptr(eo), None) == 0 and "idx_ld=14" in _lib.last_error()
    assert lib.houv_edge_diff(_lib.ptr(xd), _lib.ptr(idd), 1, 0, 12, 3, 14, 4, _lib.ptr(eo), None) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.HouvHipError, match="CPU tensor"):                  # CPU tensors are refused by the ops
        ops.edge_diff(T(x), T(idx))
    with pytest.raises(_lib.HouvHipError, match="CPU tensor"):
        ops.idam_simmat(*(T(a) for a in (src, tgt, es, et)), *(T(a) for a in par))


def test_torch_ops_registration(dev):
    from houv_amd import ops
    ops.register_torch_ops()
    src, tgt, es, et, par = cases.sim_case(2, 16, 16, 64)
    d = [T(a).to(dev) for a in (src, tgt, es, et)] + [T(a).to(dev) for a in par]
    a = torch.ops.houv.idam_simmat(*d)
    b = ops.idam_simmat(*d, want_scores=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    x, idx = cases.edge_case(2, 13, 12, 64)
    assert torch.equal(torch.ops.houv.edge_diff(T(x).to(dev), T(idx).to(dev), 12, 64), ops.edge_diff(T(x).to(dev), T(idx).to(dev), 12, 64))


# ---------------------------------------------------------------------------------------------------------------- the model
def _model(dev):
    from houv_amd.models.idam import Model
    net = Model(idam_weights.Args)
    state = {k: T(v) for k, v in idam_weights.make_state().items()}
    missing, unexpected = net.load_state_dict(state, strict=False)
    assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing), (missing, unexpected)
    return net.to(dev)


def _clouds(N):
    rng = np.random.default_rng(5)
    src = rng.uniform(-0.5, 0.5, (2, N, 3)).astype(np.float32)
    return src, (src[:, ::-1] + np.float32(0.01)).copy()


def test_embedding_vs_float64(dev):
    """GNN and the significance head against the float64 restatement on the model's own neighbour lists; the bound is 8x the
    float32 restatement's own error on these inputs (the factor section 9.7 uses at model level: the GEMMs run as bf16 x 3 splits
    in another summation order)."""
    from houv_amd.models import idam
    net = _model(dev)
    state = idam_weights.make_state()
    src, _ = _clouds(96)
    x = T(src).to(dev)
    idx = idam.knn_idx(x)
    assert idx.shape == (2, 96, 12) and (idx[..., 0].cpu() == torch.arange(96)).all()
    emb = net.emb_nn(x, idx)
    sig = net.significance_fc(emb.view(2 * 96, -1)).view(2, 96)
    e64 = host.embed(state, src, idx.cpu().numpy(), np.float64)
    e32 = host.embed(state, src, idx.cpu().numpy(), np.float32)
    s64, s32 = host.significance(state, e64, np.float64), host.significance(state, e32, np.float32)
    be, bs = 8 * float(np.abs(e32 - e64).max()), 8 * float(np.abs(s32 - s64).max())
    ee, es = float(np.abs(emb.cpu().numpy() - e64).max()), float(np.abs(sig.cpu().numpy() - s64).max())
    print("embedding error", ee, "bound", be, "significance error", es, "bound", bs, "|emb| up to", float(np.abs(e64).max()))
    assert ee <= be and es <= bs


def _check_iterations(net, state, what, spread_w, spread_R, spread_t):
    """Every iteration of the model's last forward against the float64 restatement stepped from the MODEL's own inputs of that
    iteration (so that one flipped median mask cannot make the two drift apart): corr_idx exact on unflagged rows, the median
    mask exact, weights, R and t within 8x the float32-vs-float64 spreads given.  Returns the float64 iterations."""
    ks, kt, es, et = (a.cpu().numpy() for a in net.kept)
    y64, _ = host.stepwise(state, [it["src"].cpu().numpy() for it in net.iters], kt, es, et, np.float64)
    f32, _ = host.stepwise(state, [it["src"].cpu().numpy() for it in net.iters], kt, es, et, np.float32)
    assert np.array_equal(net.iters[0]["src"].cpu().numpy(), ks)
    for i, (it, y, f) in enumerate(zip(net.iters, y64, f32)):
        flagged = host.flagged_rows(y["scores"], 4 * float(np.abs(f["scores"] - y["scores"]).max()))
        got = it["corr_idx"].cpu().numpy()
        w = it["weights"].cpu().numpy()
        ew = float(np.abs(w - y["weights"]).max())
        eR, et_ = float(np.abs(it["R"].cpu().numpy() - y["R"]).max()), float(np.abs(it["t"].cpu().numpy() - y["t"]).max())
        print(what, "iteration", i, "flagged", int(flagged.sum()), "of", flagged.size, "weights", ew, "bound", 8 * spread_w, "R", eR,
              "bound", 8 * spread_R, "t", et_, "bound", 8 * spread_t)
        assert flagged.mean() <= 0.02
        assert np.array_equal(got[~flagged], y["corr_idx"][~flagged]), (what, i)
        if not flagged.any():
            assert np.array_equal(w > 0, y["weights"] > 0), (what, i)              # w >= the LOWER median, on the same rows
            assert ew <= 8 * spread_w and eR <= 8 * spread_R and et_ <= 8 * spread_t, (what, i)
        if i + 1 < len(net.iters):                                                 # the next iteration starts from R src + t
            moved = it["src"].cpu().numpy().astype(np.float64) @ np.swapaxes(it["R"].cpu().numpy().astype(np.float64), 1, 2) \
                + it["t"].cpu().numpy().astype(np.float64)[:, None]
            assert np.abs(net.iters[i + 1]["src"].cpu().numpy() - moved).max() <= 1e-5
    return y64


@pytest.mark.parametrize("name", ["n96", "n192", "n768"])
def test_model_vs_reference_golden(golden, dev, monkeypatch, name):
    """models.idam.Model on the clouds of tests/golden/g24_idam.npz (a float32 forward of the real registration/models/idam.py
    under the same weights).  The k-NN ranking differs from the reference's in near-ties and one moved neighbour moves an
    embedding by O(1): for THIS comparison the reference's own neighbour lists are fed to the model, and the model's own k-NN path
    is held to neighbour-SET agreement > 0.999, as the DeepGMR test does.  Then: the kept sets equal the reference's (the lists in
    order too wherever the reference's order is also the float64 restatement's); every iteration against the float64
    restatement stepped from the model's own inputs (`_check_iterations`, R and t against the case's own spread); per iteration
    the correspondences, as (source point, target point) pairs, equal the reference's on rows the reference's float64 restatement
    does not flag (rows tied at the clamp only when both lists are in the reference's order: the lowest j is a matter of order);
    the final T within 8x the case's float32-vs-float64 spread of T of the float64 pose composed from the reference's
    iterations."""
    from houv_amd.models import idam
    g = golden("g24_idam.npz")
    state = idam_weights.make_state()
    net = _model(dev)
    src, tgt = T(g[f"{name}_src"]).to(dev), T(g[f"{name}_tgt"]).to(dev)
    B, N, _ = src.shape
    lists = {}
    for cloud, c in ((src, "src"), (tgt, "tgt")):
        ref_idx = T(g[f"{name}_knn_{c}"]).to(dev)
        same = (idam.knn_idx(cloud).sort(-1)[0] == ref_idx.sort(-1)[0]).all(-1).float().mean()
        assert same > 0.999, float(same)
        lists[cloud.data_ptr()] = ref_idx.contiguous()
    monkeypatch.setattr(idam, "knn_idx", lambda cloud: lists[cloud.data_ptr()])
    Tm = net(src, tgt, prefix="test").cpu().numpy()
    ordered = {}
    for c, own in (("src", net.src_idx), ("tgt", net.tgt_idx)):
        own, ref = own.cpu().numpy(), g[f"{name}_{c}_idx"]
        assert np.array_equal(np.sort(own, -1), np.sort(ref, -1)), (name, c)
        ordered[c] = np.array_equal(own, ref)
        print(name, c, "kept list in the reference's order:", ordered[c])
    assert ordered["src"] or name == "n768"
    _check_iterations(net, state, name, float(g["spread_weights"]), float(g[f"{name}_spread_R"]), float(g[f"{name}_spread_t"]))
    bi = np.arange(B)[:, None]
    r64, _ = host.stepwise(state, [g[f"{name}_src_at{i}"] for i in range(3)], g[f"{name}_tgt"][bi, g[f"{name}_tgt_idx"]],
                           g[f"{name}_es"], g[f"{name}_et"], np.float64)
    own_s, own_t = net.src_idx.cpu().numpy(), net.tgt_idx.cpu().numpy()
    for i, it in enumerate(net.iters):
        flagged = host.flagged_rows(r64[i]["scores"], 4 * float(g["spread_scores"]))
        top = r64[i]["scores"].max(-1)
        tied = (r64[i]["scores"] == top[..., None]).sum(-1) >= 2
        skip = flagged if all(ordered.values()) else flagged | tied
        ref_pair = np.full((B, N), -1)
        ref_pair[bi, g[f"{name}_src_idx"]] = np.where(skip, -2, g[f"{name}_tgt_idx"][bi, g[f"{name}_corr_idx{i}"]])
        own_pair = own_t[bi, it["corr_idx"].cpu().numpy()]
        want = ref_pair[bi, own_s]
        print(name, "iteration", i, "rows compared with the reference", int((want >= 0).sum()), "of", want.size, "differing",
              int(((want >= 0) & (want != own_pair)).sum()))
        assert (want != -1).all() and np.array_equal(own_pair[want >= 0], want[want >= 0]), (name, i)
    err = float(np.abs(Tm - g[f"{name}_T_f64"]).max())
    print(name, "T error", err, "bound", 8 * float(g[f"{name}_spread_T"]), "against the reference's float32 T", float(np.abs(Tm - g[f"{name}_T"]).max()))
    assert err <= 8 * float(g[f"{name}_spread_T"])
    assert np.array_equal(Tm[:, 3], np.broadcast_to(np.float32([0, 0, 0, 1]), (B, 4)))


def test_model_forward(dev):
    """The model on its own k-NN path, M = 32 (even: the lower median leaves 17 rows, an upper one 16): the kept lists equal
    topk of the float64 restatement's significance on the model's own neighbour lists; every iteration against the float64
    restatement stepped from the model's inputs; T is the float64 composition of the per-iteration poses; bit-identical from call
    to call; the train prefix returns the reference's tuple with loss 0."""
    from houv_amd.models import idam
    from houv_amd.train_utils import rotation_error, translation_error
    net = _model(dev)
    state = idam_weights.make_state()
    src, tgt = _clouds(192)
    s, t = T(src).to(dev), T(tgt).to(dev)
    Tm = net(s, t, prefix="test")
    assert Tm.shape == (2, 4, 4) and np.array_equal(Tm[:, 3].cpu().numpy(), np.broadcast_to(np.float32([0, 0, 0, 1]), (2, 4)))
    assert net.src_idx.shape == (2, 32) and len(net.iters) == 3
    for cloud, x, own in ((src, s, net.src_idx), (tgt, t, net.tgt_idx)):
        idx = idam.knn_idx(x).cpu().numpy()
        s64 = host.significance(state, host.embed(state, cloud, idx, np.float64), np.float64)
        s32 = host.significance(state, host.embed(state, cloud, idx, np.float32), np.float32)
        srt = -np.sort(-s64, -1)
        gap, err = float((srt[:, 31] - srt[:, 32]).min()), float(np.abs(s32 - s64).max())
        print("significance gap at place M", gap, "float32-vs-float64", err)
        if gap >= 100 * err:                                                       # the precondition under which the set is pinned
            assert np.array_equal(np.sort(own.cpu().numpy(), -1), np.sort(host.keep(s64, 32), -1))
        sig_own = np.take_along_axis(s64, own.cpu().numpy().astype(np.int64), -1)
        assert (np.diff(sig_own, axis=-1) <= 8 * err).all()                        # topk order: descending significance
    f = [host.stepwise(state, [it["src"].cpu().numpy() for it in net.iters], net.kept[1].cpu().numpy(), net.kept[2].cpu().numpy(),
                       net.kept[3].cpu().numpy(), d)[0] for d in (np.float32, np.float64)]
    sp = {q: max(float(np.abs(a[q] - b[q]).max()) for a, b in zip(*f)) for q in ("weights", "R", "t")}
    _check_iterations(net, state, "own k-NN", sp["weights"], sp["R"], sp["t"])
    assert all(int((it["weights"] > 0).sum(-1).min()) >= 17 for it in net.iters)   # M = 32: w >= the 16th smallest keeps 17
    Tc = host.compose([it["R"].cpu().numpy() for it in net.iters], [it["t"].cpu().numpy() for it in net.iters], np.float64)
    print("T against the float64 composition of the model's iterations", float(np.abs(Tm.cpu().numpy() - Tc).max()))
    assert np.abs(Tm.cpu().numpy() - Tc).max() <= 1e-5
    assert torch.equal(Tm, net(s, t, prefix="test"))                            # bit-identical from call to call
    T_gt = torch.eye(4, device=dev).repeat(2, 1, 1)
    out = net(s, t, T_gt)
    assert len(out) == 5 and float(out[0]) == 0 and all(o.shape == (2,) for o in out[1:])
    assert torch.equal(out[1], rotation_error(net.T[:, :3, :3], T_gt[:, :3, :3]))
    assert torch.equal(out[2], translation_error(net.T[:, :3, 3], T_gt[:, :3, 3]))


def test_fpfh_is_refused():
    from houv_amd.models.idam import Model

    class A(idam_weights.Args):
        use_fpfh = True
    with pytest.raises(NotImplementedError, match="FPFH"):
        Model(A)
