"""GPU: the DeepGMR head -- houv_rri_features, houv_gmm_params and houv_gmm_register against the float64
NumPy restatements of their contracts (tests/deepgmr_host.py) on the same fp32 inputs, and models.deepgmr.Model against golden
vectors from the reference's deepgmr.py (tests/golden/g23_deepgmr.npz; seeded random weights from
tests/golden/deepgmr_weights.py).  Inputs and the bounds TOL_DOT / TOL_PHI / TOL_REG (4x the float32 restatement's own error
against float64 on these inputs: theta 2.50e-07 -> 1.0e-06, phi 9.70e-06 -> 3.9e-05, T 2.14e-07 -> 8.6e-07) live in
tests/deepgmr_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

import deepgmr_cases as cases
import deepgmr_host as host

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import deepgmr_weights  # noqa: E402

T = torch.tensor
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- RRI
@pytest.mark.parametrize("B,N,k", cases.RRI_SHAPES)
def test_rri_features_vs_float64(dev, B, N, k):
    from houv_amd import ops
    xyz, idx = cases.rri_case(B, N, k)                         # idx[B,N,k+1], the point itself first
    nbr = idx[..., 1:]
    feat64, psi64, flagged = cases.rri_yardstick(xyz, nbr, k)
    x = T(xyz).to(dev)
    a = ops.rri_features(x, T(idx).to(dev), k, skip=1)         # idx_skip = 1 on the k+1 list
    assert a.shape == (B, N, 4 * k)
    cases.check_rri(a.cpu().numpy(), feat64, psi64, flagged, k, f"rri {(B, N, k)} skip=1")
    wide = np.concatenate([nbr, idx[..., :1], idx[..., :1], idx[..., :1]], axis=-1)    # idx_skip = 0, idx_ld = k + 3
    b = ops.rri_features(x, T(np.ascontiguousarray(wide)).to(dev), k, skip=0)
    assert np.array_equal(_bits(a), _bits(b))                  # the same neighbours at another offset and row pitch: same bits
    assert np.array_equal(_bits(a), _bits(ops.rri_features(x, T(idx).to(dev), k, skip=1)))     # determinism


def test_rri_zero_norm_point_follows_ieee(dev):
    from houv_amd import ops
    B, N, k = 3, 64, 20
    xyz, idx = cases.rri_case(B, N, k)
    base = ops.rri_features(T(xyz).to(dev), T(idx).to(dev), k, skip=1).cpu().numpy().reshape(B, N, k, 4)
    z = xyz.copy()
    z[:, 7] = 0.0
    got = ops.rri_features(T(z).to(dev), T(idx).to(dev), k, skip=1).cpu().numpy().reshape(B, N, k, 4)
    torch.cuda.synchronize()                                   # no fault
    nbr = idx[..., 1:]
    lists_it = (nbr == 7).any(-1)
    lists_it[:, 7] = True
    assert lists_it.sum() > B and (~lists_it).sum() > 0
    assert np.array_equal(got[~lists_it].view(np.int32), base[~lists_it].view(np.int32))       # untouched rows: same bits
    assert (got[:, 7, :, 0] == 0).all() and np.isnan(got[:, 7, :, 2]).all() and np.isnan(got[:, 7, :, 3]).all()
    want = host.rri_features(z, nbr, k, np.float64).reshape(B, N, k, 4)
    assert np.array_equal(np.isnan(got), np.isnan(want))       # NaN exactly where the restatement has it (NaNs rank last)
    rows = lists_it.copy()
    rows[:, 7] = False
    is7 = (nbr == 7)[rows]                                     # in rows listing point 7: its own slot is NaN theta / phi, rq = 0
    g, w = got[rows], want[rows]
    assert (g[..., 1][is7] == 0).all() and np.isnan(g[..., 2][is7]).all() and np.isnan(g[..., 3][is7]).all()
    _, psi64, flagged = cases.rri_yardstick(z, nbr, k)
    ok = ~is7
    assert np.abs(g[..., :2][ok] - w[..., :2][ok]).max() <= 4 * EPS32 * np.abs(w[..., :2]).max()
    assert (np.abs(g[..., 2][ok] - w[..., 2][ok]) * np.maximum(np.sin(w[..., 2][ok]), 1e-3)).max() <= cases.TOL_DOT
    fl = flagged[rows]
    d = np.abs(g[..., 3] - w[..., 3])
    assert np.where(fl | is7, 0, d).max() <= cases.TOL_PHI     # the other slots' phi skip the NaN and stay on the yardstick


def test_rri_features_rejects_bad_arguments(dev):
    from houv_amd import _lib, ops
    xyz, idx = cases.rri_case(3, 64, 20)
    x, i = T(xyz).to(dev), T(idx).to(dev)                      # idx_ld = 21
    for k, skip, msg in ((1, 0, "k=1"), (32, 0, "k=32"), (20, 2, "exceeds idx_ld=21"), (21, 1, "exceeds idx_ld=21")):
        with pytest.raises(_lib.HouvHipError, match="houv_rri_features"):
            ops.rri_features(x, i, k, skip=skip)
        assert msg in _lib.last_error()
    lib = _lib.load()
    out = torch.empty(3, 64, 80, device=dev)
    for args in ((None, _lib.ptr(i), _lib.ptr(out)), (_lib.ptr(x), None, _lib.ptr(out)), (_lib.ptr(x), _lib.ptr(i), None)):
        assert lib.houv_rri_features(args[0], args[1], 3, 64, 20, 21, 1, args[2], None) == 0
        assert "null pointer" in _lib.last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- GMM parameters
@pytest.mark.parametrize("B,N,J", cases.GMM_SHAPES)
def test_gmm_params_vs_float64(dev, B, N, J):
    """Bound of each output = 16 eps32 sum|terms| of its own sum (a tree of depth <= 14 plus the products), divided through as the
    formula divides; derived, not measured."""
    from houv_amd import ops
    gamma, pts = cases.gmm_case(B, N, J)
    g64, p64 = gamma.astype(np.float64), pts.astype(np.float64)
    pi64, mu64, sg64 = host.gmm_params(gamma, pts, np.float64)
    npi = pi64 * N
    b_pi = 16 * EPS32 * np.abs(g64).sum(1) / N
    b_mu = 16 * EPS32 * np.einsum("bnj,bnc->bjc", np.abs(g64), np.abs(p64)) / npi[..., None]
    d2 = ((p64[:, :, None, :] - mu64[:, None]) ** 2).sum(-1)
    b_sg = 16 * EPS32 * (g64 * d2).sum(1) / npi
    a = ops.gmm_params(T(gamma).to(dev), T(pts).to(dev))
    pi, mu, sg = (t.cpu().numpy().astype(np.float64) for t in a)
    print((B, N, J), "pi", float((np.abs(pi - pi64) / b_pi).max()), "mu", float((np.abs(mu - mu64) / b_mu).max()),
          "sigma", float((np.abs(sg - sg64) / np.maximum(b_sg, 1e-300)).max()), "(fractions of the bound)")
    assert (np.abs(pi - pi64) <= b_pi).all()
    assert (np.abs(mu - mu64) <= b_mu).all()
    assert (np.abs(sg - sg64) <= b_sg).all()
    b = ops.gmm_params(T(gamma).to(dev), T(pts).to(dev))
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- GMM registration
def _check_register(dev, cols):
    from houv_amd import ops
    w, ms, mt, sg, T_gt = cols
    got = ops.gmm_register(T(w).to(dev), T(ms).to(dev), T(mt).to(dev), T(sg).to(dev)).cpu().numpy()
    want = host.gmm_register(w, ms, mt, sg, np.float64)
    R = got[:, :3, :3].astype(np.float64)
    print("register", w.shape, "vs float64", float(np.abs(got - want).max()), "orthogonality",
          float(np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max()))
    assert np.abs(got - want).max() <= cases.TOL_REG
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-5 and np.abs(np.linalg.det(R) - 1).max() <= 1e-5
    assert np.array_equal(got[:, 3], np.broadcast_to(np.float32([0, 0, 0, 1]), (len(w), 4)))
    return got, want, T_gt


@pytest.mark.parametrize("B,J", cases.REG_SHAPES)
def test_gmm_register_recovers_the_pose(dev, B, J):
    got, want, T_gt = _check_register(dev, cases.reg_case(B, J))
    assert np.abs(got - T_gt).max() <= cases.TOL_REG + np.abs(want - T_gt).max()


def test_gmm_register_mirrored_targets_give_a_proper_rotation(dev):
    cols = cases.reg_case(8, 16, mirrored=True)
    _, _, _, d = host.gmm_register(*cols[:4], np.float64, return_svd=True)
    assert (d < -0.999).all()                                  # det(V U^T) = -1: the correction is what makes det R = +1
    _check_register(dev, cols)


# ---------------------------------------------------------------------------------------------------------------- whole model
def _model(dev):
    from houv_amd.models.deepgmr import Model
    net = Model(deepgmr_weights.Args)
    state = {k: T(v) for k, v in deepgmr_weights.make_state(2024).items()}
    missing, unexpected = net.load_state_dict(state, strict=False)
    assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing), (missing, unexpected)
    return net.to(dev)


@pytest.mark.parametrize("name", ["n64", "n256"])
def test_model_vs_reference_golden(golden, dev, monkeypatch, name):
    """gamma and T_12 against the reference run in float64, within 8x the fixture's own float32-vs-float64 spread (the GEMMs run as
    bf16 x 3 splits in another summation order).  The k-NN ranking differs from the reference's in near-ties, and one moved
    neighbour moves 4 of a point's 80 input features by O(1): for THIS comparison the reference's own neighbour lists go through
    ops.rri_features, and the model's own k-NN path is held to neighbour-SET agreement > 0.999, as tests/test_gpu_dcp.py does."""
    from houv_amd import ops
    from houv_amd.mm3d_pn2 import knn_cross
    from houv_amd.models import deepgmr
    g = golden("g23_deepgmr.npz")
    net = _model(dev)
    assert sorted(k for k in net.state_dict() if not k.endswith("num_batches_tracked")) == [str(k) for k in g["state_keys"]]
    src, tgt = T(g[f"{name}_src"]).to(dev), T(g[f"{name}_tgt"]).to(dev)
    feats = {}
    for cloud, c in ((src, "1"), (tgt, "2")):
        ref_idx = T(g[f"{name}_knn{c}_f32"]).to(dev)
        own = knn_cross(21, cloud, cloud)[1][..., 1:]
        same = (own.sort(-1)[0] == ref_idx.sort(-1)[0]).all(-1).float().mean()
        assert same > 0.999, float(same)
        feats[cloud.data_ptr()] = ops.rri_features(cloud, ref_idx.contiguous(), 20)
    monkeypatch.setattr(deepgmr, "rri_rows", lambda pts, k: feats[pts.data_ptr()])
    T12 = net(src, tgt, prefix="test")
    for c in ("1", "2"):
        spread = float(np.abs(g[f"{name}_gamma{c}_f32"].astype(np.float64) - g[f"{name}_gamma{c}_f64"]).max())
        err = float(np.abs(getattr(net, "gamma" + c).cpu().numpy() - g[f"{name}_gamma{c}_f64"]).max())
        print(name, "gamma" + c, "error", err, "fixture spread", spread)
        assert err <= 8 * spread
    err = float(np.abs(T12.cpu().numpy() - g[f"{name}_T12_f64"]).max())
    print(name, "T_12 error", err, "t12_spread", float(g["t12_spread"]))
    assert err <= 8 * float(g["t12_spread"])
    assert np.array_equal(T12[:, 3].cpu().numpy(), np.broadcast_to(np.float32([0, 0, 0, 1]), (2, 4)))


def test_train_prefix_returns_the_reference_tuple(golden, dev):
    from houv_amd.train_utils import rotation_error, translation_error
    g = golden("g23_deepgmr.npz")
    net = _model(dev)
    src, tgt, T_gt = (T(g[f"n64_{n}"]).to(dev) for n in ("src", "tgt", "T_gt"))
    out = net(src, tgt, T_gt)
    assert len(out) == 5 and out[0].ndim == 0 and all(o.shape == (2,) for o in out[1:])
    assert torch.equal(out[1], rotation_error(net.T_12[:, :3, :3], T_gt[:, :3, :3]))
    assert torch.equal(out[2], translation_error(net.T_12[:, :3, 3], T_gt[:, :3, 3]))
    assert torch.equal(net.T_12, net(src, tgt, prefix="test"))


def test_get_rri_cluster_layout_and_torch_ops(dev):
    """get_rri_cluster folds clusters into the batch and returns [B,4k,S,M]; the ops are reachable as torch.ops.houv.*."""
    from houv_amd import model_utils, ops
    from houv_amd.mm3d_pn2 import knn_cross
    xyz, _ = cases.rri_case(2, 65, 20)
    x = T(xyz).to(dev)                                         # two clouds as M = 2 clusters of one batch entry
    cl = x.permute(2, 1, 0).unsqueeze(0).contiguous()          # [1,3,S,M]
    f = model_utils.get_rri_cluster(cl, 20)
    assert f.shape == (1, 80, 65, 2)
    idx = knn_cross(21, x, x)[1]
    assert (idx[..., 0].cpu() == torch.arange(65)).all()
    ops.register_torch_ops()
    rows = torch.ops.houv.rri_features(x, idx, 20, 1)
    assert torch.equal(f[0].permute(2, 1, 0), rows)
    gamma, pts = cases.gmm_case(2, 64, 16)
    pi, mu, sg = torch.ops.houv.gmm_params(T(gamma).to(dev), T(pts).to(dev))
    assert torch.equal(torch.ops.houv.gmm_register(pi, mu, mu, sg), ops.gmm_register(pi, mu, mu, sg))
