"""GPU: the PCN completion network -- houv_mlp2_max and houv_pcn_fold against the float64 NumPy
restatement of their contracts (tests/pcn_host.py, written in the reference's concatenating formulation) on the same fp32
inputs, and models.pcn.Model against golden vectors from the reference's pcn.py (tests/golden/g25_pcn.npz; seeded weights from
tests/golden/pcn_weights.py).  Kernel-level bound: 4x the float32 restatement's own maximum error against float64 on the same
inputs, computed and printed per case.  Model-level bound: 8x the fixture's float32-vs-float64 spread (section 9.7's factor) of the restatement's float64 forward."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pcn_cases as cases
import pcn_host as host

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pcn_weights  # noqa: E402

T = torch.tensor
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _mlp_yardstick(key, case):
    """(pooled64, y64, bound_pooled, bound_y): computed once per case and shared."""
    if key not in _CACHE:
        p64, y64 = host.mlp2_max(*case, dtype=np.float64)
        p32, y32 = host.mlp2_max(*case, dtype=np.float32)
        assert y32.dtype == np.float32
        _CACHE[key] = (p64, y64, 4 * float(np.abs(p32 - p64).max()), 4 * float(np.abs(y32 - y64).max()))
    return _CACHE[key]


def _run_mlp(dev, case, want_y):
    from houv_amd import ops
    return ops.mlp2_max(*(T(a).to(dev) for a in case), want_y=want_y)


def test_row_tile_constant():
    from houv_amd import ops
    assert ops.PCN_ROW_TILE == cases.T


# ---------------------------------------------------------------------------------------------------------------- mlp2_max
@pytest.mark.parametrize("N", cases.MLP_N)
@pytest.mark.parametrize("B", cases.MLP_B)
@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_vs_float64(dev, Cin, H, Cout, B, N):
    case = cases.mlp_case(B, N, Cin, H, Cout)
    p64, y64, bp, by = _mlp_yardstick((B, N, Cin), case)
    pooled, y = _run_mlp(dev, case, True)
    torch.cuda.synchronize()
    assert pooled.shape == (B, Cout) and y.shape == (B, N, Cout)
    ep, ey = float(np.abs(pooled.cpu().numpy() - p64).max()), float(np.abs(y.cpu().numpy() - y64).max())
    print((Cin, H, Cout), "B", B, "N", N, "pooled error", ep, "bound", bp, "y error", ey, "bound", by)
    assert ep <= bp and ey <= by
    assert np.array_equal(_bits(y.max(1)[0]), _bits(pooled))                      # the pool is the maximum of what was stored
    pooled_only, none = _run_mlp(dev, case, False)
    assert none is None and np.array_equal(_bits(pooled_only), _bits(pooled))     # y stored or not: identical pooled bits
    again, y_again = _run_mlp(dev, case, True)
    assert np.array_equal(_bits(again), _bits(pooled)) and np.array_equal(_bits(y_again), _bits(y))   # two calls: identical bits


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_all_negative_columns(dev, Cin, H, Cout):
    """b2 far below anything W2 . h reaches: every pooled value is negative, and still the true maximum."""
    x, W1, s1, W2, b2 = cases.mlp_case(3, cases.T + 1, Cin, H, Cout, seed=1)
    case = (x, W1, s1, (W2 * np.float32(0.25)).astype(np.float32), (b2 - np.float32(50)).astype(np.float32))
    p64, y64 = host.mlp2_max(*case, dtype=np.float64)
    p32, _ = host.mlp2_max(*case, dtype=np.float32)
    assert (p64 < -10).all()
    bound = 4 * float(np.abs(p32 - p64).max())
    pooled, y = _run_mlp(dev, case, True)
    err = float(np.abs(pooled.cpu().numpy() - p64).max())
    print((Cin, H, Cout), "all-negative pooled error", err, "bound", bound)
    assert (pooled < -10).all() and err <= bound and np.array_equal(_bits(y.max(1)[0]), _bits(pooled))


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_largest_row_is_the_last_of_a_partial_tile(dev, Cin, H, Cout):
    """N = T + 3: the last valid row (the third of the second tile) carries an input 8x larger than any other, so it owns the
    maximum of every column in which its value is positive and beyond the other rows' (about 0.38 of them: P(z > 2.5 / 8) for a
    unit normal against the ~2.5 sigma maximum of 66 others); it has to be seen, and the rows past it must not."""
    N = cases.T + 3
    x, W1, s1, W2, b2 = cases.mlp_case(2, N, Cin, H, Cout, seed=2)
    x[:, N - 1] *= np.float32(8)
    case = (x, W1, s1, W2, b2)
    p64, y64 = host.mlp2_max(*case, dtype=np.float64)
    p32, _ = host.mlp2_max(*case, dtype=np.float32)
    owner = y64.argmax(1)
    assert (owner == N - 1).mean() > 0.3
    bound = 4 * float(np.abs(p32 - p64).max())
    pooled, _ = _run_mlp(dev, case, False)
    err = float(np.abs(pooled.cpu().numpy() - p64).max())
    print((Cin, H, Cout), "last-row pooled error", err, "bound", bound, "columns owned by the last row", float((owner == N - 1).mean()))
    assert err <= bound


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_shared_against_per_cloud_shift(dev, Cin, H, Cout):
    x, W1, s1, W2, b2 = cases.mlp_case(3, cases.T + 1, Cin, H, Cout, per_cloud=False, seed=3)
    assert s1.shape == (H,)
    shared = _run_mlp(dev, (x, W1, s1, W2, b2), True)
    tiled = _run_mlp(dev, (x, W1, np.tile(s1, (3, 1)), W2, b2), True)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(shared, tiled))
    other = np.tile(s1, (3, 1))
    other[1] += np.float32(0.5)                                                   # only cloud 1 may move
    moved = _run_mlp(dev, (x, W1, other, W2, b2), True)
    assert np.array_equal(_bits(moved[0][0]), _bits(shared[0][0])) and np.array_equal(_bits(moved[0][2]), _bits(shared[0][2]))
    assert not np.array_equal(_bits(moved[0][1]), _bits(shared[0][1]))
    p64, _ = host.mlp2_max(x, W1, other, W2, b2, dtype=np.float64)
    p32, _ = host.mlp2_max(x, W1, other, W2, b2, dtype=np.float32)
    assert np.abs(moved[0].cpu().numpy() - p64).max() <= 4 * np.abs(p32 - p64).max()


# ---------------------------------------------------------------------------------------------------------------- pcn_fold
def _run_fold(dev, case):
    from houv_amd import ops
    return ops.pcn_fold(*(T(a).to(dev) for a in case))


@pytest.mark.parametrize("scale", cases.FOLD_SCALES)
@pytest.mark.parametrize("nc", cases.FOLD_NC)
@pytest.mark.parametrize("B", cases.FOLD_B)
def test_pcn_fold_vs_float64(dev, B, nc, scale):
    case = cases.fold_case(B, nc, scale)
    f64 = host.fold_rows(*case, dtype=np.float64)
    f32 = host.fold_rows(*case, dtype=np.float32)
    assert f32.dtype == np.float32
    bound = 4 * float(np.abs(f32 - f64).max())
    fine = _run_fold(dev, case)
    torch.cuda.synchronize()
    assert fine.shape == (B, nc * scale, 3)
    err = float(np.abs(fine.cpu().numpy() - f64).max())
    print("fold B", B, "nc", nc, "scale", scale, "error", err, "bound", bound, "|fine| up to", float(np.abs(f64).max()))
    assert err <= bound
    assert np.array_equal(_bits(_run_fold(dev, case)), _bits(fine))               # two calls: identical bits


@pytest.mark.parametrize("scale", [1, 3, 16])
def test_pcn_fold_zero_weights_replicate_the_centres(dev, scale):
    """W2 = W3 = 0: fine[b, c*scale + s] = b3 + coarse[b, c] exactly, for every s: the f -> (c, s) map and the centre add."""
    coarse, cvec, grid, Wgp, W2, b2, W3, b3 = cases.fold_case(3, cases.T + 1, scale, seed=1)
    fine = _run_fold(dev, (coarse, cvec, grid, Wgp, np.zeros_like(W2), b2, np.zeros_like(W3), b3)).cpu().numpy()
    want = np.repeat((b3[None, None, :] + coarse)[:, :, None, :], scale, axis=2).reshape(3, -1, 3)
    assert want.dtype == np.float32 and np.array_equal(fine.view(np.int32), want.view(np.int32))


def test_pcn_fold_clouds_differ_where_cvec_differs(dev):
    coarse, cvec, grid, Wgp, W2, b2, W3, b3 = cases.fold_case(2, cases.T + 1, 4, seed=2)
    coarse[1], cvec[1] = coarse[0], cvec[0]
    same = _run_fold(dev, (coarse, cvec, grid, Wgp, W2, b2, W3, b3))
    assert np.array_equal(_bits(same[0]), _bits(same[1]))
    cvec[1, 100:] += np.float32(0.25)
    diff = _run_fold(dev, (coarse, cvec, grid, Wgp, W2, b2, W3, b3))
    assert np.array_equal(_bits(diff[0]), _bits(same[0])) and (diff[1] != same[1]).float().mean() > 0.9
    f64 = host.fold_rows(coarse, cvec, grid, Wgp, W2, b2, W3, b3, dtype=np.float64)
    f32 = host.fold_rows(coarse, cvec, grid, Wgp, W2, b2, W3, b3, dtype=np.float32)
    assert np.abs(diff.cpu().numpy() - f64).max() <= 4 * np.abs(f32 - f64).max()


# ---------------------------------------------------------------------------------------------------------------- errors, torch.ops
def test_error_paths(dev):
    from houv_amd import _lib, ops
    lib = _lib.load()
    d = [T(a).to(dev) for a in cases.mlp_case(2, 5, 3, 128, 256)]
    x, W1, s1, W2, b2 = (_lib.ptr(t) for t in d)
    pooled = torch.empty(2, 256, device=dev)

    def mlp(N=5, Cin=3, H=128, Cout=256, stride=128, x=x, pooled=_lib.ptr(pooled), ws=None):
        return lib.houv_mlp2_max(x, 2, N, Cin, W1, H, s1, stride, W2, b2, Cout, pooled, None, ws, None)
    assert mlp() == 1
    for kw, msg in ((dict(N=0), "N=0"), (dict(Cin=4), "(4, 128, 256)"), (dict(H=256), "(3, 256, 256)"), (dict(Cout=512), "(3, 128, 512)"),
                    (dict(stride=64), "shift1_stride=64"), (dict(x=None), "x is a null pointer"), (dict(pooled=None), "pooled is a null pointer"),
                    (dict(N=cases.T + 1), "workspace is a null pointer: N=65")):
        assert mlp(**kw) == 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    assert lib.houv_mlp2_max_workspace_bytes(2, cases.T, 256) == 0
    assert lib.houv_mlp2_max_workspace_bytes(2, cases.T + 1, 256) == 2 * 2 * 256 * 4
    f = [T(a).to(dev) for a in cases.fold_case(2, 3, 2)]
    fp = [_lib.ptr(t) for t in f]
    fine = torch.empty(2, 6, 3, device=dev)

    def fold(nc=3, scale=2, p=fp, out=_lib.ptr(fine)):
        return lib.houv_pcn_fold(p[0], p[1], p[2], 2, nc, scale, *p[3:], out, None)
    assert fold() == 1
    for kw, msg in ((dict(nc=0), "nc=0"), (dict(scale=0), "scale=0"), (dict(out=None), "fine is a null pointer"),
                    (dict(p=fp[:4] + [None] + fp[5:]), "W2 is a null pointer")):
        assert fold(**kw) == 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    with pytest.raises(_lib.HouvHipError, match="CPU tensor"):
        ops.mlp2_max(*(T(a) for a in cases.mlp_case(2, 5, 3, 128, 256)))
    with pytest.raises(_lib.HouvHipError, match="CPU tensor"):
        ops.pcn_fold(*(T(a) for a in cases.fold_case(2, 3, 2)))
    with pytest.raises(_lib.HouvHipError, match=r"\(4, 128, 256\)"):                # through the op: the library's message
        ops.mlp2_max(torch.zeros(1, 5, 4, device=dev), torch.zeros(128, 4, device=dev), d[2][0].contiguous(), d[3], d[4])
    with pytest.raises(_lib.HouvHipError, match="shift1 must be"):
        ops.mlp2_max(d[0], d[1], torch.zeros(3, 128, device=dev), d[3], d[4])
    with pytest.raises(_lib.HouvHipError, match="expected torch.float32"):
        ops.pcn_fold(f[0].double(), *f[1:])


def test_torch_ops_registration(dev):
    from houv_amd import ops
    ops.register_torch_ops()
    d = [T(a).to(dev) for a in cases.mlp_case(3, cases.T + 1, 256, 512, 1024)]
    a, b = torch.ops.houv.mlp2_max(*d), ops.mlp2_max(*d, want_y=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    f = [T(a).to(dev) for a in cases.fold_case(3, cases.T + 1, 4)]
    assert torch.equal(torch.ops.houv.pcn_fold(*f), ops.pcn_fold(*f))


# ---------------------------------------------------------------------------------------------------------------- the model
def _model(dev, num_points, num_coarse):
    from houv_amd.models.pcn import Model
    net = Model(pcn_weights.args(num_points), num_coarse=num_coarse)
    net.load_state_dict({k: T(v) for k, v in pcn_weights.make_state(num_coarse).items()}, strict=True)
    return net.to(dev)


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_model_vs_reference_golden(golden, dev, name):
    """models.pcn.Model on the clouds of tests/golden/g25_pcn.npz under the same weights: feat, out1 and out2 within 8x the case's
    stored float32-vs-float64 spread of the stored float64 forward (the NumPy restatement's under the same weights, which the CPU
    tests tie to the reference's float32 forward); "val" returns the reference's five keys with the metrics
    of calc_cd on out2; bit-identical from call to call."""
    from houv_amd.model_utils_completion import calc_cd
    g = golden("g25_pcn.npz")
    num_points, num_coarse = cases.GOLDEN_CASES[name]
    net = _model(dev, num_points, num_coarse)
    x = T(g[f"{name}_x"]).to(dev)
    seen = {}
    hook = net.encoder.register_forward_hook(lambda m, i, o: seen.__setitem__("feat", o))
    res = net(x, prefix="test")
    hook.remove()
    assert list(res) == ["result"] and res["result"].shape == (2, num_points, 3)
    gt = (torch.rand(2, num_points, 3, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev)
    val = net(x, gt, prefix="val")
    assert sorted(val) == ["cd_p", "cd_t", "f1", "out1", "out2"] and val["out1"].shape == (2, num_coarse, 3)
    assert torch.equal(val["out2"], res["result"])                               # bit-identical from call to call
    got = dict(feat=seen["feat"], out1=val["out1"], out2=val["out2"])
    for q in ("feat", "out1", "out2"):
        keep = g[f"{name}_{q}_idx"].astype(np.int64)
        own = got[q].cpu().numpy()[:, keep]
        err, bound = float(np.abs(own - g[f"{name}_{q}_f64"]).max()), 8 * float(g[f"{name}_spread_{q}"])
        print(name, q, "error", err, "bound", bound, "against the reference's float32", float(np.abs(own - g[f"{name}_{q}"]).max()))
        assert err <= bound, (name, q)
    for k, v in zip(("cd_p", "cd_t", "f1"), calc_cd(val["out2"], gt, calc_f1=True)):
        assert torch.equal(val[k], v) and v.shape == (2,)


def test_model_train_prefix_and_refusals(dev):
    from houv_amd.model_utils_completion import calc_cd
    from houv_amd.models.pcn import Model
    net = _model(dev, 96, 24)
    g = torch.Generator().manual_seed(2)
    x, gt = (torch.rand(2, 3, 100, generator=g) - 0.5).to(dev), (torch.rand(2, 96, 3, generator=g) - 0.5).to(dev)
    out2, loss2, total = net(x, gt, prefix="train", alpha=0.5)
    assert out2.shape == (2, 96, 3) and loss2.shape == (2,) and total.dim() == 0 and not total.requires_grad
    assert torch.equal(loss2, calc_cd(out2, gt)[0])
    with pytest.raises(ValueError, match="power of two"):
        Model(pcn_weights.args(96), num_coarse=32)
