"""CPU: the host-side refusals of houv_amd.ops and houv_amd.mm3d_pn2, message by message.  _lib.require_gpu and
_lib.require_gpu_any are replaced by no-ops (as in tests/test_run_stage_launches.py), each wrapper is called with small CPU
tensors that trip one check, and the full text of the message is stated literally.  The checks that a family of wrappers shares
are tripped through every member: the wrapper's own name at the front of the message is what a shared check can get wrong.
No library and no device: every call is refused before it would launch."""
import pytest
import torch

from houv_amd import _lib, mm3d_pn2, ops

I8, I64, F64 = torch.int8, torch.int64, torch.float64
ROWS = "expected [B,N,C] rows with unit channel stride and one row stride, got shape"


def F(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def I(*shape, dtype=torch.int32):
    return torch.zeros(shape, dtype=dtype)


def E(*shape):
    """A float32 tensor of the shape that holds one element (weights whose values no check reads)."""
    return torch.zeros(1).expand(shape)


def wide(*shape):
    """A [.., C] view with channel stride 2: refused by every row check."""
    return torch.zeros(shape + (2,))[..., 0]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "require_gpu_any", lambda *a, **k: None)


def refused(msg, fn, *args, **kw):
    with pytest.raises(_lib.HouvHipError) as e:
        fn(*args, **kw)
    assert str(e.value) == msg


def wants(name, dtype, got):
    return f"{name}: expected {dtype}, got {got}"


def swap(args, i, new):
    """args with entry i (a position or a keyword) replaced."""
    if isinstance(args, dict):
        return {**args, i: new}
    return args[:i] + (new,) + args[i + 1:]


# ---- Chamfer, Kabsch, pose ------------------------------------------------------------------------------------------------
def test_chamfer():
    fw = (F(1, 2, 3), F(1, 4, 3), F(1, 2), F(1, 4), I(1, 2), I(1, 4))
    refused(wants("xyz1", "torch.float32", "torch.float64"), ops.chamfer_forward, *swap(fw, 0, F(1, 2, 3, dtype=F64)))
    refused(wants("idx2", "torch.int32", "torch.int64"), ops.chamfer_forward, *swap(fw, 5, I(1, 4, dtype=I64)))
    refused("chamfer_forward: expected xyz1[B,N,3], xyz2[B,M,3]", ops.chamfer_forward, *swap(fw, 1, F(1, 4, 2)))
    refused("chamfer_forward: expected xyz1[B,N,3], xyz2[B,M,3]", ops.chamfer_forward, *swap(fw, 1, F(2, 4, 3)))
    refused("chamfer_forward: output shapes do not match [B,N] / [B,M]", ops.chamfer_forward, *swap(fw, 2, F(1, 3)))
    refused("chamfer_forward: output shapes do not match [B,N] / [B,M]", ops.chamfer_forward, *swap(fw, 5, I(1, 3)))
    bw = (F(1, 2, 3), F(1, 4, 3), F(1, 2, 3), F(1, 4, 3), F(1, 2), F(1, 4), I(1, 2), I(1, 4))
    refused(wants("graddist1", "torch.float32", "torch.float64"), ops.chamfer_backward, *swap(bw, 4, F(1, 2, dtype=F64)))
    refused(wants("idx1", "torch.int32", "torch.int64"), ops.chamfer_backward, *swap(bw, 6, I(1, 2, dtype=I64)))
    refused("chamfer_backward: shape mismatch", ops.chamfer_backward, *swap(bw, 2, F(1, 2, 2)))
    refused("chamfer_backward: shape mismatch", ops.chamfer_backward, *swap(bw, 7, I(1, 3)))


def test_kabsch_and_pose():
    refused("kabsch: expected src, corr [B,3,N]", ops.kabsch, F(1, 2, 4), F(1, 2, 4))
    refused("kabsch: expected src, corr [B,3,N]", ops.kabsch, F(1, 3, 4), F(1, 3, 5))
    refused(wants("corr", "torch.float32", "torch.float64"), ops.kabsch, F(1, 3, 4), F(1, 3, 4, dtype=F64))
    refused("kabsch: expected weights [B,1,N]", ops.kabsch, F(1, 3, 4), F(1, 3, 4), F(1, 1, 3))
    refused(wants("weights", "torch.float32", "torch.float64"), ops.kabsch, F(1, 3, 4), F(1, 3, 4), F(1, 1, 4, dtype=F64))
    refused(wants("params", "torch.float32", "torch.float64"), ops.pose_forward, F(2, 8, dtype=F64), 0)
    refused(wants("src", "torch.float32", "torch.float64"), ops.pose_forward, F(2, 8), 0, 0, F(2, 4, 3, dtype=F64))


# ---- the fused solve: entry and seed share the src / tgt / state / nn_ws checks ----------------------------------------------
def _solve(**over):
    a = dict(src=F(1, 4, 3), tgt=F(1, 4, 3), state=F(2, 24, dtype=F64), K=2, steps_done=0, n_iters=1, angle_base=0, trans_mode=0,
             use_views=True, f64_params=False, k_full=2, k_view=4, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, loss_scale=1.0,
             out_score=F(2), out_loss=F(2), out_R=F(2, 3, 3), out_T=F(2, 3))
    a.update(over)
    return a


def _seed(**over):
    a = dict(src=F(1, 4, 3), tgt=F(1, 4, 3), state=F(2, 24, dtype=F64), K=2, angle_base=0, trans_mode=0, use_views=True,
             nn_ws=I(2, 16, 8, dtype=torch.int16))
    a.update(over)
    return a


NN_WS = "nn_ws must be a contiguous int16 [P*K,16,stride] tensor (ops.solve_workspace)"


@pytest.mark.parametrize("who, fn, base", [("solve_iterate", ops.solve_iterate_out, _solve), ("solve_seed", ops.solve_seed, _seed)])
def test_solve_shared_checks(who, fn, base):
    refused(wants("src", "torch.float32", "torch.float64"), fn, **base(src=F(1, 4, 3, dtype=F64)))
    refused(wants("tgt", "torch.float32", "torch.float64"), fn, **base(tgt=F(1, 4, 3, dtype=F64)))
    refused(wants("state", "torch.float64", "torch.float32"), fn, **base(state=F(2, 24)))
    refused(f"{who}: expected src[P,N,3], tgt[P,M,3]", fn, **base(tgt=F(2, 4, 3)))
    refused(f"{who}: expected src[P,N,3], tgt[P,M,3]", fn, **base(src=F(1, 4, 2)))
    refused(f"{who}: expected src[P,N,3], tgt[P,M,3]", fn, **base(tgt=F(1, 5, 2)))
    refused(f"{who}: state must be [2,24], got (3, 24)", fn, **base(state=F(3, 24, dtype=F64)))
    refused(f"{who}: state must be [6,24], got (2, 24)", fn, **base(K=6))
    refused(f"{who}: {NN_WS}", fn, **base(nn_ws=I(2, 16, 8)))                                   # int32
    refused(f"{who}: {NN_WS}", fn, **base(nn_ws=I(3, 16, 8, dtype=torch.int16)))
    refused(f"{who}: {NN_WS}", fn, **base(nn_ws=I(2, 16, dtype=torch.int16)))
    refused(f"{who}: {NN_WS}", fn, **base(nn_ws=I(2, 16, 8, 2, dtype=torch.int16)[..., 0]))     # not contiguous
    refused(f"{who}: state must be [2,24], got (2, 23)", fn, **base(state=F(2, 23, dtype=F64), nn_ws=I(2, 16, 8)))  # state first


def test_solve_seed_needs_a_workspace():
    refused(f"solve_seed: {NN_WS}", ops.solve_seed, **_seed(nn_ws=None))


def test_solve_iterate_out():
    fn = ops.solve_iterate_out
    refused("solve_iterate: out_score must hold 2 floats, got 3", fn, **_solve(out_score=F(3)))
    refused("solve_iterate: out_loss must hold 2 floats, got 1", fn, **_solve(out_loss=F(1)))
    refused("solve_iterate: out_R must hold 18 floats, got 6", fn, **_solve(out_R=F(2, 3)))
    refused("solve_iterate: out_T must hold 6 floats, got 4", fn, **_solve(out_T=F(2, 2)))
    refused("solve_iterate: out_grad must hold 16 floats, got 14", fn, **_solve(out_grad=F(2, 7)))
    refused("solve_iterate: out_cd must hold 16 floats, got 8", fn, **_solve(out_cd=F(1, 8)))
    refused(wants("out_cd", "torch.float32", "torch.float64"), fn, **_solve(out_cd=F(2, 8, dtype=F64)))
    ws = I(2, 16, 8, dtype=torch.int16)
    refused("solve_iterate: the large-cloud kernel is a brute-force sweep and takes no workspace", fn, **_solve(large=True, nn_ws=ws))
    refused("solve_iterate: the large-cloud kernel has no stage form", fn, **_solve(large=True, chunk_iters=1, sched_ws=I(6)))
    refused("solve_iterate: sched_ws must hold 6 int32 (ops.solve_sched_workspace)", fn, **_solve(chunk_iters=1, sched_ws=I(5)))
    refused("solve_iterate: sched_ws must hold 6 int32 (ops.solve_sched_workspace)", fn,
            **_solve(chunk_iters=1, sched_ws=I(6, dtype=I64)))
    refused("solve_iterate: sched_ws must hold 6 int32 (ops.solve_sched_workspace)", fn,
            **_solve(chunk_iters=1, sched_ws=I(5), nn_ws=I(2, 16, 8)))                          # the schedule before the workspace
    refused(f"solve_iterate: {NN_WS}", fn, **_solve(chunk_iters=1, sched_ws=I(6), nn_ws=I(2, 16, 8)))


def test_solve_iterate_forms():
    a = _solve(tgt=F(2, 4, 3))
    a = {k: v for k, v in a.items() if k not in ("large",)}
    refused("solve_iterate: expected src[P,N,3], tgt[P,M,3]", ops.solve_iterate_large_out, **a)
    refused("solve_iterate: out_R must hold 18 floats, got 6", ops.solve_iterate_large_out, **_solve(out_R=F(2, 3)))
    kw = dict(steps_done=0, n_iters=1, angle_base=0, trans_mode=0, use_views=True, f64_params=False, k_full=2, k_view=4, lr=0.01,
              loss_scale=1.0)
    refused("solve_iterate: state must be [2,24], got (3, 24)", ops.solve_iterate, F(1, 4, 3), F(1, 4, 3), F(3, 24, dtype=F64), 2, **kw)
    refused(f"solve_iterate: {NN_WS}", ops.solve_iterate, F(1, 4, 3), F(1, 4, 3), F(2, 24, dtype=F64), 2, nn_ws=I(2, 16, 8), **kw)
    refused("solve_iterate: the large-cloud kernel has no stage form", ops.solve_iterate, F(1, 4, 3), F(1, 4, 3), F(2, 24, dtype=F64),
            2, large=True, chunk_iters=1, sched_ws=I(6), want_grad=True, want_cd=True, **kw)


# ---- k-d sort, ICP, EMD ---------------------------------------------------------------------------------------------------------
def test_kd_sort_icp_emd():
    refused(wants("cloud", "torch.float32", "torch.float64"), ops.kd_sort, F(1, 4, 3, dtype=F64))
    refused("kd_sort: expected cloud[P,N,3]", ops.kd_sort, F(1, 4, 2))
    refused("kd_sort: expected cloud[P,N,3]", ops.kd_sort, F(4, 3))
    refused("kd_sort: rule must be one of ['area', 'extent'], got 'volume'", ops.kd_sort, F(1, 4, 3), rule="volume")
    refused(wants("tgt", "torch.float32", "torch.float64"), ops.icp_refine, F(1, 4, 3), F(1, 4, 3, dtype=F64))
    refused("icp_refine: expected src[P,N,3], tgt[P,M,3]", ops.icp_refine, F(1, 4, 3), F(2, 4, 3))
    refused("icp_refine: expected src[P,N,3], tgt[P,M,3]", ops.icp_refine, F(1, 4, 3), F(1, 5, 2))
    refused("icp_refine: init must be [P,4,4]", ops.icp_refine, F(1, 4, 3), F(1, 5, 3), F(1, 3, 4))
    refused(wants("init", "torch.float32", "torch.float64"), ops.icp_refine, F(1, 4, 3), F(1, 5, 3), F(1, 4, 4, dtype=F64))
    refused("emd_forward: expected xyz1[B,N,3], xyz2[B,N,3]", ops.emd_forward, F(1, 4, 3), F(1, 4, 2), 0.01, 10)
    refused("emd_forward: expected xyz1[B,N,3], xyz2[B,N,3]", ops.emd_forward, F(1, 4, 3, dtype=F64), F(2, 4, 3), 0.01, 10)
    # the clouds and the gradient are converted to fp32 before anything is checked: a float64 cloud is not what is refused
    refused(wants("assignment", "torch.int32", "torch.int64"), ops.emd_backward, F(1, 4, 3, dtype=F64), F(1, 4, 3), F(1, 4, dtype=F64),
            I(1, 4, dtype=I64))
    refused("emd_backward: shape mismatch", ops.emd_backward, F(1, 4, 3), F(1, 5, 3), F(1, 4), I(1, 4))
    refused("emd_backward: shape mismatch", ops.emd_backward, F(1, 4, 3), F(1, 4, 3), F(1, 4), I(1, 3))


# ---- DeepGMR head -----------------------------------------------------------------------------------------------------------------
def test_rri_features():
    refused(wants("idx", "torch.int32", "torch.int64"), ops.rri_features, F(1, 4, 3), I(1, 4, 2, dtype=I64), 2)
    refused("rri_features: expected xyz[B,N,3], idx[B,N,L]", ops.rri_features, F(1, 4, 3), I(1, 5, 2), 2)
    refused("rri_features: expected xyz[B,N,3], idx[B,N,L]", ops.rri_features, F(1, 4, 2), I(1, 4, 2), 2)


def _gmm_params_bw(**over):
    a = dict(gamma=F(1, 4, 2), pts=F(1, 4, 3), pi=F(1, 2), mu=F(1, 2, 3), sigma=F(1, 2), g_pi=F(1, 2), g_mu=F(1, 2, 3), g_sigma=F(1, 2))
    a.update(over)
    return a


def test_gmm_params_family():
    for who, fn, base in (("gmm_params", ops.gmm_params, lambda **o: {**dict(gamma=F(1, 4, 2), pts=F(1, 4, 3)), **o}),
                          ("gmm_params_backward", ops.gmm_params_backward, _gmm_params_bw)):
        refused(wants("gamma", "torch.float32", "torch.float64"), fn, **base(gamma=F(1, 4, 2, dtype=F64)))
        refused(wants("pts", "torch.float32", "torch.float64"), fn, **base(pts=F(1, 4, 3, dtype=F64)))
        refused(f"{who}: expected gamma[B,N,J], pts[B,N,3]", fn, **base(pts=F(1, 5, 3)))
        refused(f"{who}: expected gamma[B,N,J], pts[B,N,3]", fn, **base(pts=F(1, 4, 2)))
        refused(f"{who}: expected gamma[B,N,J], pts[B,N,3]", fn, **base(gamma=F(4, 2)))
    fn, shapes = ops.gmm_params_backward, "gmm_params_backward: expected pi / sigma and their gradients [B,J], mu / g_mu [B,J,3]"
    refused(wants("g_sigma", "torch.float32", "torch.float64"), fn, **_gmm_params_bw(g_sigma=F(1, 2, dtype=F64)))
    refused(shapes, fn, **_gmm_params_bw(mu=F(1, 2)))
    refused(shapes, fn, **_gmm_params_bw(g_pi=F(1, 3)))
    refused(shapes, fn, **_gmm_params_bw(g_mu=F(1, 2, 2)))
    refused("gmm_params_backward: expected gamma[B,N,J], pts[B,N,3]", fn, **_gmm_params_bw(pts=F(1, 5, 3), mu=F(1, 2)))   # the order


def test_gmm_register_family():
    fw = "gmm_register: expected pi_s[B,J], mu_s[B,J,3], mu_t[B,J,3], sigma_t[B,J]"
    bw = "gmm_register_backward: expected pi_s[B,J], mu_s[B,J,3], mu_t[B,J,3], sigma_t[B,J], g_T[B,4,4]"
    ok = (F(1, 2), F(1, 2, 3), F(1, 2, 3), F(1, 2))
    for msg, fn, args in ((fw, ops.gmm_register, ok), (bw, ops.gmm_register_backward, ok + (F(1, 4, 4),))):
        refused(wants("pi_s", "torch.float32", "torch.float64"), fn, *swap(args, 0, F(1, 2, dtype=F64)))
        refused(wants("sigma_t", "torch.float32", "torch.float64"), fn, *swap(args, 3, F(1, 2, dtype=F64)))
        refused(msg, fn, *swap(args, 0, F(2)))
        refused(msg, fn, *swap(args, 1, F(1, 2, 2)))
        refused(msg, fn, *swap(args, 2, F(1, 3, 3)))
        refused(msg, fn, *swap(args, 3, F(1, 3)))
    refused(wants("g_T", "torch.float32", "torch.float64"), ops.gmm_register_backward, *ok, F(1, 4, 4, dtype=F64))
    refused(bw, ops.gmm_register_backward, *ok, F(1, 3, 4))
    refused(bw, ops.gmm_register_backward, *ok, F(2, 4, 4))


def test_bn_rows():
    rows = "expected rows [R,C] with contiguous columns and a row stride >= C"
    v = (F(2), F(2), F(2), F(2))
    refused(f"bn_rows_stats: {rows}", ops.bn_rows_stats, F(4))
    refused(f"bn_rows_stats: {rows}", ops.bn_rows_stats, F(0, 2))
    refused(f"bn_relu_rows: {rows}", ops.bn_relu_rows, F(2, 4).t(), *v)
    refused(f"bn_relu_rows_backward: {rows}", ops.bn_relu_rows_backward, F(4, 2), F(4), *v)
    refused(f"bn_relu_rows_backward: {rows}", ops.bn_relu_rows_backward, F(2, 4).t(), F(4, 2), *v)
    refused("bn_relu_rows_backward: gy and z differ in shape", ops.bn_relu_rows_backward, F(3, 2), F(4, 2), *v)
    for fn, lead in ((ops.bn_relu_rows, (F(4, 2),)), (ops.bn_relu_rows_backward, (F(4, 2), F(4, 2)))):
        refused("bn_rows: expected per-channel vectors of 2 elements", fn, *lead, *swap(v, 0, F(3)))
        refused("bn_rows: expected per-channel vectors of 2 elements", fn, *lead, *swap(v, 3, F(1, 2)))
        refused(wants("per-channel vector", "torch.float32", "torch.float64"), fn, *lead, *swap(v, 2, F(2, dtype=F64)))
    refused("bn_relu_rows: n_group = 3 does not divide the 4 rows", ops.bn_relu_rows, F(4, 2), *v, n_group=3)
    refused("bn_relu_rows: n_group = -1 does not divide the 4 rows", ops.bn_relu_rows, F(4, 2), *v, n_group=-1)


# ---- IDAM head --------------------------------------------------------------------------------------------------------------------
def test_idam():
    a = (F(1, 2, 3), F(1, 3, 3), F(1, 2, 4), F(1, 3, 4), F(32, 12), F(32), F(32), E(32, 32), F(32), E(32, 32), F(32), F(32), F(32), F(1))
    clouds = "idam_simmat: expected src[B,Ms,3], tgt[B,Mt,3], es[B,Ms,E], et[B,Mt,E]"
    pars = "idam_simmat: expected W1[32,2E+4], W2[32,32], W3[32,32], b4[1] and 32-element s1, t1, b2, s3, t3, w4"
    refused(wants("idam_simmat", "torch.float32", "torch.float64"), ops.idam_simmat, *swap(a, 12, F(32, dtype=F64)))
    refused(clouds, ops.idam_simmat, *swap(a, 3, F(1, 3, 5)))
    refused(clouds, ops.idam_simmat, *swap(a, 2, F(1, 3, 4)))
    refused(clouds, ops.idam_simmat, *swap(a, 1, F(2, 3, 3)))
    refused(pars, ops.idam_simmat, *swap(a, 4, F(32, 11)))
    refused(pars, ops.idam_simmat, *swap(a, 13, F(2)))
    refused(pars, ops.idam_simmat, *swap(a, 8, F(31)))
    refused(wants("x", "torch.float32", "torch.float64"), ops.edge_diff, F(1, 4, 2, dtype=F64), I(1, 4, 3))
    refused(wants("idx", "torch.int32", "torch.int64"), ops.edge_diff, F(1, 4, 2), I(1, 4, 3, dtype=I64))
    refused("edge_diff: expected x[B,N,C], idx[B,N,L]", ops.edge_diff, F(1, 4, 2), I(1, 5, 3))
    refused("edge_diff: expected x[B,N,C], idx[B,N,L]", ops.edge_diff, F(4, 2), I(1, 4, 3))


# ---- PCN: the three mlp2_max entries share the x / W1 / W2 / shift1 checks, the two fold entries theirs ----------------------------
MLP2 = dict(x=F(1, 2, 3), W1=F(4, 3), shift1=F(4), W2=F(5, 4))


def _mlp2_fw(**over):
    return {**MLP2, "b2": F(5), **over}


def _mlp2_bw(**over):
    return {**MLP2, "arg": I(1, 5), "gpooled": F(1, 5), **over}


@pytest.mark.parametrize("who, fn, base, tail", [("mlp2_max", ops.mlp2_max, _mlp2_fw, ", b2[Cout]"),
                                                 ("mlp2_max_arg", ops.mlp2_max_arg, _mlp2_fw, ", b2[Cout]"),
                                                 ("mlp2_max_backward", ops.mlp2_max_backward, _mlp2_bw, "")])
def test_mlp2_max_shared_checks(who, fn, base, tail):
    for name in ("x", "W1", "shift1", "W2"):
        refused(wants(f"{who}: {name}", "torch.float32", "torch.float64"), fn, **base(**{name: MLP2[name].double()}))
    got_b2 = ", (5,)" if tail else ""
    shapes = f"{who}: expected x[B,N,Cin], W1[H,Cin], W2[Cout,H]{tail}, got "
    refused(shapes + "(1, 2, 3), (4, 2), (5, 4)" + got_b2, fn, **base(W1=F(4, 2)))
    refused(shapes + "(1, 2, 3), (4, 3), (5, 3)" + got_b2, fn, **base(W2=F(5, 3)))
    refused(shapes + "(2, 3), (4, 3), (5, 4)" + got_b2, fn, **base(x=F(2, 3)))
    refused(f"{who}: shift1 must be [4] or [1,4], got (2, 4)", fn, **base(shift1=F(2, 4)))
    refused(f"{who}: shift1 must be [4] or [1,4], got (5,)", fn, **base(shift1=F(5)))
    refused(f"{who}: shift1 must be [4] or [2,4], got (1, 4)", fn, **base(x=F(2, 2, 3), shift1=F(1, 4), **(
        {} if tail else dict(arg=I(2, 5), gpooled=F(2, 5)))))
    refused(shapes + "(1, 2, 3), (4, 2), (5, 4)" + got_b2, fn, **base(W1=F(4, 2), shift1=F(5)))          # shapes before shift1


def test_mlp2_max_own_checks():
    for fn, who in ((ops.mlp2_max, "mlp2_max"), (ops.mlp2_max_arg, "mlp2_max_arg")):
        refused(wants(f"{who}: b2", "torch.float32", "torch.float64"), fn, **_mlp2_fw(b2=F(5, dtype=F64)))
        refused(f"{who}: expected x[B,N,Cin], W1[H,Cin], W2[Cout,H], b2[Cout], got (1, 2, 3), (4, 3), (5, 4), (4,)", fn, **_mlp2_fw(b2=F(4)))
    fn = ops.mlp2_max_backward
    refused(wants("mlp2_max_backward: gpooled", "torch.float32", "torch.float64"), fn, **_mlp2_bw(gpooled=F(1, 5, dtype=F64)))
    refused(wants("mlp2_max_backward: arg", "torch.int32", "torch.int64"), fn, **_mlp2_bw(arg=I(1, 5, dtype=I64)))
    refused("mlp2_max_backward: arg and gpooled must be [1,5], got (1, 4), (1, 5)", fn, **_mlp2_bw(arg=I(1, 4)))
    refused("mlp2_max_backward: arg and gpooled must be [1,5], got (1, 5), (5,)", fn, **_mlp2_bw(gpooled=F(5)))
    refused("mlp2_max_backward: arg and gpooled must be [1,5], got (1, 4), (1, 5)", fn, **_mlp2_bw(arg=I(1, 4), shift1=F(5)))   # before shift1
    refused("mlp2_max_backward: rows, nrows and gy_rows come together", fn, **_mlp2_bw(rows=I(1, 2)))
    refused("mlp2_max_backward: rows, nrows and gy_rows come together", fn, **_mlp2_bw(nrows=I(1), gy_rows=F(1, 2, 5)))
    rows = dict(rows=I(1, 2), nrows=I(1), gy_rows=F(1, 2, 5))
    refused(wants("mlp2_max_backward: rows", "torch.int32", "torch.int64"), fn, **_mlp2_bw(**{**rows, "rows": I(1, 2, dtype=I64)}))
    refused(wants("mlp2_max_backward: nrows", "torch.int32", "torch.int64"), fn, **_mlp2_bw(**{**rows, "nrows": I(1, dtype=I64)}))
    refused(wants("mlp2_max_backward: gy_rows", "torch.float32", "torch.float64"), fn, **_mlp2_bw(**{**rows, "gy_rows": F(1, 2, 5, dtype=F64)}))
    refused("mlp2_max_backward: expected rows[1,R], nrows[1], gy_rows[1,R,5], got (1, 2), (2,), (1, 2, 5)", fn,
            **_mlp2_bw(**{**rows, "nrows": I(2)}))
    refused("mlp2_max_backward: expected rows[1,R], nrows[1], gy_rows[1,R,5], got (1, 2), (1,), (1, 3, 5)", fn,
            **_mlp2_bw(**{**rows, "gy_rows": F(1, 3, 5)}))
    refused("mlp2_max_backward: shift1 must be [4] or [1,4], got (5,)", fn, **_mlp2_bw(**{**rows, "nrows": I(2)}, shift1=F(5)))  # shift1 first


def _fold(**over):
    a = dict(coarse=F(1, 2, 3), cvec=E(1, 512), grid=F(2, 2), Wgp=E(512, 5), W2=E(512, 512), b2=E(512), W3=E(3, 512), b3=F(3))
    a.update(over)
    return a


@pytest.mark.parametrize("who, fn, more", [("pcn_fold", ops.pcn_fold, {}), ("pcn_fold_backward", ops.pcn_fold_backward, dict(gfine=F(1, 4, 3)))])
def test_pcn_fold_shared_checks(who, fn, more):
    base = lambda **over: _fold(**more, **over)
    refused(wants(who, "torch.float32", "torch.float64"), fn, **base(b3=F(3, dtype=F64)))
    refused(wants(who, "torch.float32", "torch.float64"), fn, **base(coarse=F(1, 2, 3, dtype=F64)))
    clouds = f"{who}: expected coarse[B,nc,3], cvec[B,512], grid[2,scale], got "
    refused(clouds + "(1, 2, 3), (1, 5), (2, 2)", fn, **base(cvec=F(1, 5)))
    refused(clouds + "(1, 2, 2), (1, 512), (2, 2)", fn, **base(coarse=F(1, 2, 2)))
    refused(clouds + "(1, 2, 3), (1, 512), (3, 2)", fn, **base(grid=F(3, 2)))
    refused(clouds + "(2, 2, 3), (1, 512), (2, 2)", fn, **base(coarse=F(2, 2, 3)))
    weights = f"{who}: expected Wgp[512,5], W2[512,512], b2[512], W3[3,512], b3[3]"
    refused(weights, fn, **base(Wgp=E(512, 4)))
    refused(weights, fn, **base(W2=E(512, 511)))
    refused(weights, fn, **base(b2=E(511)))
    refused(weights, fn, **base(W3=E(512, 3)))
    refused(weights, fn, **base(b3=F(4)))
    refused(clouds + "(1, 2, 3), (1, 5), (2, 2)", fn, **base(cvec=F(1, 5), b3=F(4)))           # the clouds before the weights


def test_pcn_fold_backward_own_checks():
    refused(wants("pcn_fold_backward", "torch.float32", "torch.float64"), ops.pcn_fold_backward, **_fold(gfine=F(1, 4, 3, dtype=F64)))
    refused("pcn_fold_backward: gfine must be [1,4,3], got (1, 4, 2)", ops.pcn_fold_backward, **_fold(gfine=F(1, 4, 2)))
    refused("pcn_fold_backward: gfine must be [1,6,3], got (1, 4, 3)", ops.pcn_fold_backward, **_fold(grid=F(2, 3), gfine=F(1, 4, 3)))
    refused("pcn_fold_backward: expected Wgp[512,5], W2[512,512], b2[512], W3[3,512], b3[3]", ops.pcn_fold_backward,
            **_fold(b3=F(4), gfine=F(1, 4, 2)))                                                 # the weights before gfine


# ---- ECG: the three dense_conv entries share the x / idx / weight checks --------------------------------------------------------------
def test_knn_feat():
    refused(f"knn_feat: x: {ROWS} (4, 2) strides (2, 1)", ops.knn_feat, F(4, 2), 2)
    refused(f"knn_feat: x: {ROWS} (1, 4, 2) strides (16, 4, 2)", ops.knn_feat, wide(1, 4, 2), 2)
    refused(f"knn_feat: x: {ROWS} (2, 2, 2) strides (8, 2, 1)", ops.knn_feat, F(2, 4, 2)[:, :2], 2)     # two row strides


def _dense(**over):
    a = dict(x=F(1, 2, 24), idx=I(1, 2, 3), W0=E(24, 48), b0=E(24), W1=E(24, 48), b1=E(24), W2=E(24, 72), b2=E(24))
    a.update(over)
    return a


def _dense_bw(**over):
    return _dense(**{**dict(arg=I(1, 2, 72, dtype=I8), gout=F(1, 2, 96)), **over})


@pytest.mark.parametrize("who, fn, base", [("dense_conv", ops.dense_conv, _dense), ("dense_conv_arg", ops.dense_conv_arg, _dense),
                                           ("dense_conv_backward", ops.dense_conv_backward, _dense_bw)])
def test_dense_conv_shared_checks(who, fn, base):
    refused(wants(f"{who}: idx", "torch.int32", "torch.int64"), fn, **base(idx=I(1, 2, 3, dtype=I64)))
    refused(f"{who}: x: {ROWS} (2, 24) strides (24, 1)", fn, **base(x=F(2, 24)))
    refused(f"{who}: x: {ROWS} (1, 2, 24) strides (96, 48, 2)", fn, **base(x=wide(1, 2, 24)))
    refused(f"{who}: expected idx[1,2,k], got (1, 3, 3)", fn, **base(idx=I(1, 3, 3)))
    refused(f"{who}: expected idx[1,2,k], got (2, 3)", fn, **base(idx=I(2, 3)))
    weights = f"{who}: expected W0[24,48], W1[24,48], W2[24,72] and biases [24], got "
    refused(weights + "(24, 47), (24, 48), (24, 72)", fn, **base(W0=E(24, 47)))
    refused(weights + "(24, 48), (24, 47), (24, 72)", fn, **base(W1=E(24, 47)))
    refused(weights + "(24, 48), (24, 48), (23, 72)", fn, **base(W2=E(23, 72)))
    refused(weights + "(24, 48), (24, 48), (24, 72)", fn, **base(b1=E(23)))
    refused(f"{who}: expected W0[24,96], W1[24,72], W2[24,96] and biases [24], got (24, 48), (24, 48), (24, 72)", fn,
            **base(x=F(1, 2, 48), **({} if who != "dense_conv_backward" else dict(gout=F(1, 2, 120)))))
    refused(f"{who}: expected idx[1,2,k], got (1, 3, 3)", fn, **base(idx=I(1, 3, 3), W0=E(24, 47)))      # idx before the weights


@pytest.mark.parametrize("who, fn", [("dense_conv", ops.dense_conv), ("dense_conv_arg", ops.dense_conv_arg)])
def test_dense_conv_out(who, fn):
    refused(f"{who}: out must be [1,2,96], got (1, 2, 95)", fn, **_dense(out=F(1, 2, 95)))
    refused(f"{who}: out must be [1,2,96], got (2, 96)", fn, **_dense(out=F(2, 96)))
    refused(f"{who}: out: {ROWS} (1, 2, 96) strides (384, 192, 2)", fn, **_dense(out=wide(1, 2, 96)))
    refused(f"{who}: expected W0[24,48], W1[24,48], W2[24,72] and biases [24], got (24, 47), (24, 48), (24, 72)", fn,
            **_dense(W0=E(24, 47), out=F(1, 2, 95)))                                            # the weights before out


def test_dense_conv_backward_own_checks():
    fn, who = ops.dense_conv_backward, "dense_conv_backward"
    refused(f"{who}: arg must be int8 [1,2,72], got torch.int32 (1, 2, 72)", fn, **_dense_bw(arg=I(1, 2, 72)))
    refused(f"{who}: arg must be int8 [1,2,72], got torch.int8 (1, 2, 71)", fn, **_dense_bw(arg=I(1, 2, 71, dtype=I8)))
    refused(f"{who}: gout must be [1,2,96], got (1, 2, 95)", fn, **_dense_bw(gout=F(1, 2, 95)))
    refused(f"{who}: gout: {ROWS} (1, 2, 96) strides (384, 192, 2)", fn, **_dense_bw(gout=wide(1, 2, 96)))
    refused(f"{who}: relu_out needs the forward's out [1,2,96]", fn, **_dense_bw(relu_out=True))
    refused(f"{who}: relu_out needs the forward's out [1,2,96]", fn, **_dense_bw(relu_out=True, out=F(1, 2, 95)))
    refused(f"{who}: out: {ROWS} (1, 2, 96) strides (384, 192, 2)", fn, **_dense_bw(relu_out=True, out=wide(1, 2, 96)))
    refused(f"{who}: gx must be [1,2,24], got (1, 2, 23)", fn, **_dense_bw(gx=F(1, 2, 23)))
    refused(f"{who}: gx must be [1,2,24], got (1, 2, 23)", fn, **_dense_bw(gx=F(1, 2, 23), out=F(1, 2, 95)))   # out unread without relu_out
    refused(f"{who}: gx: {ROWS} (1, 2, 24) strides (96, 48, 2)", fn, **_dense_bw(gx=wide(1, 2, 24)))
    refused(f"{who}: arg must be int8 [1,2,72], got torch.int32 (1, 2, 72)", fn, **_dense_bw(arg=I(1, 2, 72), gout=F(1, 2, 95), gx=F(1, 2, 23)))
    refused(f"{who}: gout must be [1,2,96], got (1, 2, 95)", fn, **_dense_bw(gout=F(1, 2, 95), gx=F(1, 2, 23)))


# ---- VRCNet: attention, edge pool, EF expansion, the loss node --------------------------------------------------------------------
def _sa(**over):       # C = 64: rel 4, mid 16, m 2; k = 3
    a = dict(P=F(1, 2, 24), x=F(1, 2, 64), idx=I(1, 2, 3), Ww1=F(2, 16), Ww2=F(6, 2), bw2=F(6), Wout=E(64, 16), bout=E(64))
    a.update(over)
    return a


def _sa_bw(**over):
    a = {k: v for k, v in _sa().items() if k in ("P", "idx", "Ww1", "Ww2", "bw2")}
    return {**a, "G": F(1, 2, 16), **over}


def test_sa_attn():
    fn = ops.sa_attn
    refused(wants("sa_attn: idx", "torch.int32", "torch.int64"), fn, **_sa(idx=I(1, 2, 3, dtype=I64)))
    refused(f"sa_attn: x: {ROWS} (2, 64) strides (64, 1)", fn, **_sa(x=F(2, 64)))
    refused("sa_attn: expected idx[1,2,k], got (1, 3, 3)", fn, **_sa(idx=I(1, 3, 3)))
    refused("sa_attn: expected P[1,2,24], got (1, 2, 23)", fn, **_sa(P=F(1, 2, 23)))
    refused(f"sa_attn: P: {ROWS} (1, 2, 24) strides (96, 48, 2)", fn, **_sa(P=wide(1, 2, 24)))
    weights = "sa_attn: expected Ww1[2,16], Ww2[6,2], bw2[6], Wout[64,16], bout[64], got "
    refused(weights + "(2, 15), (6, 2), (6,), (64, 16), (64,)", fn, **_sa(Ww1=F(2, 15)))
    refused(weights + "(2, 16), (6, 2), (5,), (64, 16), (64,)", fn, **_sa(bw2=F(5)))
    refused(weights + "(2, 16), (6, 2), (6,), (64, 15), (64,)", fn, **_sa(Wout=E(64, 15)))
    refused("sa_attn: out must be [1,2,64], got (1, 2, 63)", fn, **_sa(out=F(1, 2, 63)))
    refused(f"sa_attn: out: {ROWS} (1, 2, 64) strides (256, 128, 2)", fn, **_sa(out=wide(1, 2, 64)))
    refused(weights + "(2, 15), (6, 2), (6,), (64, 16), (64,)", fn, **_sa(Ww1=F(2, 15), out=F(1, 2, 63)))


def test_sa_attn_backward():
    fn, who = ops.sa_attn_backward, "sa_attn_backward"
    refused(wants(f"{who}: idx", "torch.int32", "torch.int64"), fn, **_sa_bw(idx=I(1, 2, 3, dtype=I64)))
    refused(f"{who}: P: {ROWS} (2, 24) strides (24, 1)", fn, **_sa_bw(P=F(2, 24)))
    refused(f"{who}: expected idx[1,2,k], got (1, 3, 3)", fn, **_sa_bw(idx=I(1, 3, 3)))
    refused(f"{who}: P has 23 columns; 2 rel + mid = 24, 48, 96 or 192 (C = 64 .. 512) are served", fn, **_sa_bw(P=F(1, 2, 23)))
    refused(f"{who}: P has 30 columns; 2 rel + mid = 24, 48, 96 or 192 (C = 64 .. 512) are served", fn, **_sa_bw(P=F(1, 2, 30)))
    refused(f"{who}: expected Ww1[2,16], Ww2[6,2], bw2[6], got (2, 15), (6, 2), (6,)", fn, **_sa_bw(Ww1=F(2, 15)))
    refused(f"{who}: expected Ww1[2,16], Ww2[6,2], bw2[6], got (2, 16), (6, 3), (6,)", fn, **_sa_bw(Ww2=F(6, 3)))
    refused(f"{who}: G must be [1,2,16], got (1, 2, 15)", fn, **_sa_bw(G=F(1, 2, 15)))
    refused(f"{who}: G: {ROWS} (1, 2, 16) strides (64, 32, 2)", fn, **_sa_bw(G=wide(1, 2, 16)))
    refused(f"{who}: gP must be [1,2,24], got (1, 2, 23)", fn, **_sa_bw(gP=F(1, 2, 23)))
    refused(f"{who}: gP: {ROWS} (1, 2, 24) strides (96, 48, 2)", fn, **_sa_bw(gP=wide(1, 2, 24)))
    refused(f"{who}: G must be [1,2,16], got (1, 2, 15)", fn, **_sa_bw(G=F(1, 2, 15), gP=F(1, 2, 23)))


def test_edge_pool():
    lists = "expected p_idx[1,S] and pn_idx[1,S,pk], got"
    fw = dict(feat=F(1, 4, 2), p_idx=I(1, 3), pn_idx=I(1, 3, 2))
    bw = dict(g=F(1, 3, 4), p_idx=I(1, 3), pn_idx=I(1, 3, 2), arg=I(1, 3, 2, dtype=I8), N=4)
    for who, fn, a in (("edge_pool", ops.edge_pool, fw), ("edge_pool_backward", ops.edge_pool_backward, bw)):
        refused(wants(f"{who}: p_idx", "torch.int32", "torch.int64"), fn, **swap(a, "p_idx", I(1, 3, dtype=I64)))
        refused(wants(f"{who}: pn_idx", "torch.int32", "torch.int64"), fn, **swap(a, "pn_idx", I(1, 3, 2, dtype=I64)))
        refused(f"{who}: {lists} (1, 3) and (1, 2, 2)", fn, **swap(a, "pn_idx", I(1, 2, 2)))
        refused(f"{who}: {lists} (2, 3) and (1, 3, 2)", fn, **swap(a, "p_idx", I(2, 3)))
    refused(f"edge_pool: feat: {ROWS} (4, 2) strides (2, 1)", ops.edge_pool, **swap(fw, "feat", F(4, 2)))
    refused("edge_pool: out must be [1,3,4], got (1, 3, 3)", ops.edge_pool, **fw, out=F(1, 3, 3))
    refused(f"edge_pool: out: {ROWS} (1, 3, 4) strides (24, 8, 2)", ops.edge_pool, **fw, out=wide(1, 3, 4))
    refused(f"edge_pool: {lists} (1, 3) and (1, 2, 2)", ops.edge_pool, **swap(fw, "pn_idx", I(1, 2, 2)), out=F(1, 3, 3))
    refused(f"edge_pool_backward: g: {ROWS} (3, 4) strides (4, 1)", ops.edge_pool_backward, **swap(bw, "g", F(3, 4)))
    both = "edge_pool_backward: expected g[1,3,2C] and int8 arg[1,3,C], got"
    refused(f"{both} (1, 3, 4) and torch.int32 (1, 3, 2)", ops.edge_pool_backward, **swap(bw, "arg", I(1, 3, 2)))
    refused(f"{both} (1, 3, 4) and torch.int8 (1, 3, 3)", ops.edge_pool_backward, **swap(bw, "arg", I(1, 3, 3, dtype=I8)))
    refused(f"{both} (1, 3, 5) and torch.int8 (1, 3, 2)", ops.edge_pool_backward, **swap(bw, "g", F(1, 3, 5)))
    refused(f"{both} (1, 2, 4) and torch.int8 (1, 3, 2)", ops.edge_pool_backward, **swap(bw, "g", F(1, 2, 4)))


def test_cd_loss_backward():
    fn, who = ops.cd_loss_backward, "cd_loss_backward"
    a = dict(output=F(1, 3, 3), gt=F(1, 2, 3), dist1=F(1, 2), dist2=F(1, 3), idx1=I(1, 2), idx2=I(1, 3), g_p=F(1), g_t=F(1))
    refused(wants(f"{who}: idx1", "torch.int32", "torch.int64"), fn, **swap(a, "idx1", I(1, 2, dtype=I64)))
    refused(wants(f"{who}: g_t", "torch.float32", "torch.float64"), fn, **swap(a, "g_t", F(1, dtype=F64)))
    refused(f"{who}: expected output[B,M,3] and gt[B,N,3], got (1, 3, 3) and (2, 2, 3)", fn, **swap(a, "gt", F(2, 2, 3)))
    refused(f"{who}: expected output[B,M,3] and gt[B,N,3], got (1, 3, 2) and (1, 2, 3)", fn, **swap(a, "output", F(1, 3, 2)))
    lists = f"{who}: expected dist1, idx1 [1,2], dist2, idx2 [1,3] and g_p, g_t [1], got "
    refused(lists + "(1, 3), (1, 2), (1, 3), (1, 3), (1,), (1,)", fn, **swap(a, "dist1", F(1, 3)))
    refused(lists + "(1, 2), (1, 2), (1, 3), (1, 2), (1,), (1,)", fn, **swap(a, "idx2", I(1, 2)))
    refused(lists + "(1, 2), (1, 2), (1, 3), (1, 3), (2,), (1,)", fn, **swap(a, "g_p", F(2)))
    refused(wants(f"{who}: gout", "torch.float32", "torch.float64"), fn, **a, gout=F(1, 3, 3, dtype=F64))
    refused(f"{who}: gout must be [1,3,3], got (1, 3, 2)", fn, **a, gout=F(1, 3, 2))
    refused(f"{who}: gout must be [1,3,3], got (1, 2, 3)", fn, **a, gout=F(1, 2, 3))


def _ef(**over):       # O = 2, r = 1: proj has 2 O + 2 O r = 8 columns
    a = dict(proj=F(1, 2, 8), idx=I(1, 2, 3), W2a=F(2, 2), W3=F(2, 2), r=1)
    a.update(over)
    return a


def _ef_fw(**over):
    return _ef(**{"b3": F(2), **over})


def _ef_bw(**over):
    return _ef(**{"arg": I(1, 2, 2, dtype=I8), "g": F(1, 2, 2), **over})


@pytest.mark.parametrize("who, fn, base", [("ef_expand", ops.ef_expand, _ef_fw), ("ef_expand_backward", ops.ef_expand_backward, _ef_bw)])
def test_ef_expand_shared_checks(who, fn, base):
    refused(f"{who}: proj: {ROWS} (2, 8) strides (8, 1)", fn, **base(proj=F(2, 8)))
    dense = f"{who}: expected dense W3[O,O] and proj[B,N,2O+2Or], got W3 "
    refused(dense + "(2, 3), proj (1, 2, 8), r=1", fn, **base(W3=F(2, 3)))
    refused(dense + "(2, 2), proj (1, 2, 8), r=1", fn, **base(W3=F(2, 4)[:, :2]))
    refused(dense + "(2, 2), proj (1, 2, 8), r=2", fn, **base(r=2))
    refused(dense + "(2, 2), proj (1, 2, 8), r=0", fn, **base(r=0))
    refused(dense + "(2, 2), proj (1, 2, 7), r=1", fn, **base(proj=F(1, 2, 7)))
    refused(f"{who}: expected W2a[2,2] rows with unit column stride, got (3, 2) strides (2, 1)", fn, **base(W2a=F(3, 2)))
    refused(f"{who}: expected W2a[2,2] rows with unit column stride, got (2, 2) strides (1, 2)", fn, **base(W2a=F(2, 2).t()))
    refused(wants(f"{who}: idx", "torch.int32", "torch.int64"), fn, **base(idx=I(1, 2, 3, dtype=I64)))
    refused(f"{who}: expected idx[1,2,k], got (1, 3, 3)", fn, **base(idx=I(1, 3, 3)))
    refused(dense + "(2, 3), proj (1, 2, 8), r=1", fn, **base(W3=F(2, 3), idx=I(1, 3, 3)))               # W3 before idx


def test_ef_expand_own_checks():
    refused(wants("ef_expand: b3", "torch.float32", "torch.float64"), ops.ef_expand, **_ef_fw(b3=F(2, dtype=F64)))
    refused("ef_expand: b3 must be [2], got (3,)", ops.ef_expand, **_ef_fw(b3=F(3)))
    refused("ef_expand: out must be [1,2,2], got (1, 2, 3)", ops.ef_expand, **_ef_fw(out=F(1, 2, 3)))
    refused(f"ef_expand: out: {ROWS} (1, 2, 2) strides (8, 4, 2)", ops.ef_expand, **_ef_fw(out=wide(1, 2, 2)))
    refused("ef_expand: b3 must be [2], got (3,)", ops.ef_expand, **_ef_fw(b3=F(3), out=F(1, 2, 3)))
    fn, who = ops.ef_expand_backward, "ef_expand_backward"
    refused(f"{who}: expected g[1,2,2] and int8 arg of that shape, got (1, 2, 3) and torch.int8 (1, 2, 2)", fn, **_ef_bw(g=F(1, 2, 3)))
    refused(f"{who}: expected g[1,2,2] and int8 arg of that shape, got (1, 2, 2) and torch.int32 (1, 2, 2)", fn, **_ef_bw(arg=I(1, 2, 2)))
    refused(f"{who}: g: {ROWS} (1, 2, 2) strides (8, 4, 2)", fn, **_ef_bw(g=wide(1, 2, 2)))
    refused(f"{who}: gproj must be [1,2,8], got (1, 2, 7)", fn, **_ef_bw(gproj=F(1, 2, 7)))
    refused(f"{who}: gproj: {ROWS} (1, 2, 8) strides (32, 16, 2)", fn, **_ef_bw(gproj=wide(1, 2, 8)))
    refused(f"{who}: g: {ROWS} (1, 2, 2) strides (8, 4, 2)", fn, **_ef_bw(g=wide(1, 2, 2), gproj=F(1, 2, 7)))


# ---- DCP feature head -----------------------------------------------------------------------------------------------------------------
def test_dcp_blocks():
    refused(wants("xyz", "torch.float32", "torch.float64"), ops.knn, F(1, 4, 3, dtype=F64), 2)
    refused("knn: expected xyz[B,N,3]", ops.knn, F(1, 4, 2), 2)
    refused("knn: expected xyz[B,N,3]", ops.knn, F(4, 3), 2)
    ec = (F(1, 4, 3), I(1, 4, 2), F(64, 6), F(64), F(64))
    refused(wants("idx", "torch.int32", "torch.int64"), ops.edgeconv1, *swap(ec, 1, I(1, 4, 2, dtype=I64)))
    refused("edgeconv1: expected xyz[B,N,3], idx[B,N,k]", ops.edgeconv1, *swap(ec, 1, I(1, 3, 2)))
    refused("edgeconv1: expected W[64,6], scale[64], shift[64]", ops.edgeconv1, *swap(ec, 2, F(64, 5)))
    refused("edgeconv1: expected W[64,6], scale[64], shift[64]", ops.edgeconv1, *swap(ec, 4, F(63)))
    shape = "max_over_k: expected act[npts*k,C], out[npts, >= col0+C]"
    refused(wants("out", "torch.float32", "torch.float64"), ops.max_over_k, F(4, 4), 2, F(2, 8, dtype=F64), 0)
    refused(shape, ops.max_over_k, F(4, 4), 0, F(2, 8), 0)
    refused(shape, ops.max_over_k, F(4, 4), 2, F(2, 8), -4)
    refused(shape, ops.max_over_k, F(16), 2, F(2, 8), 0)
    refused(shape + " (C and the row stride multiples of 4)", ops.max_over_k, F(3, 4), 2, F(2, 8), 0)
    refused(shape + " (C and the row stride multiples of 4)", ops.max_over_k, F(4, 3), 2, F(2, 8), 0)
    refused(shape + " (C and the row stride multiples of 4)", ops.max_over_k, F(4, 4), 2, F(2, 6), 0)
    refused(shape + " (C and the row stride multiples of 4)", ops.max_over_k, F(4, 4), 2, F(2, 8), 8)
    refused("max_over_k: act and out[:, col0:] must start on 16-byte boundaries (col0 a multiple of 4 in a 16-byte aligned buffer)",
            ops.max_over_k, F(4, 4), 2, F(2, 8), 1)
    qkv = "attention: expected Q[P,Nq,H,128], K[P,Nk,H,128], V[P,Nk,H,128]"
    refused(qkv, ops.attention, F(1, 2, 1, 64), F(1, 3, 1, 64), F(1, 3, 1, 64), 1.0)
    refused(qkv, ops.attention, F(1, 2, 1, 128), F(1, 3, 1, 128), F(1, 4, 1, 128), 1.0)
    refused("attention: heads must be contiguous 128-float slices of a token row", ops.attention, F(1, 2, 1, 128), F(1, 3, 1, 128),
            wide(1, 3, 1, 128), 1.0)
    with pytest.raises(AssertionError, match="innermost dimension must be contiguous"):
        ops.gemm(wide(2, 4), F(3, 4))


def test_layernorm_and_softmax():
    refused(wants("residual", "torch.float32", "torch.float64"), ops.layernorm, F(2, 4), F(4), F(4), residual=F(2, 4, dtype=F64))
    refused("layernorm: expected x[..., D]", ops.layernorm, F(), F(1), F(1))
    refused("layernorm: a, b must have D elements and residual the shape of x", ops.layernorm, F(2, 4), F(4), F(3))
    refused("layernorm: a, b must have D elements and residual the shape of x", ops.layernorm, F(2, 4), F(4), F(4), residual=F(4))
    refused("layernorm: x, a, b and residual must start on 16-byte boundaries", ops.layernorm, F(9)[1:].view(2, 4), F(4), F(4))
    refused("layernorm: x, a, b and residual must start on 16-byte boundaries", ops.layernorm, F(2, 4), F(4), F(4), residual=F(9)[1:].view(2, 4))
    refused(wants("x", "torch.float32", "torch.float64"), ops.softmax_rows_, F(2, 4, dtype=F64))
    refused(wants("pts", "torch.float32", "torch.float64"), ops.softmax_corr, F(1, 2, 3), F(1, 3, 3, dtype=F64))
    refused("softmax_corr: expected scores[P,N,M], pts[P,M,3]", ops.softmax_corr, F(1, 2, 3), F(1, 2, 3))
    refused("softmax_corr: expected scores[P,N,M], pts[P,M,3]", ops.softmax_corr, F(2, 3), F(1, 3, 3))


# ---- mm3d_pn2 -----------------------------------------------------------------------------------------------------------------------
def test_mm3d_pn2():
    m = mm3d_pn2
    floating = "expected a floating-point tensor, got torch.int32"
    refused("furthest_point_sample: expected points_xyz[B,N,3] and 0 < num_points <= N", m.furthest_point_sample, F(1, 4, 3), 5)
    refused("furthest_point_sample: expected points_xyz[B,N,3] and 0 < num_points <= N", m.furthest_point_sample, F(1, 4, 3), 0)
    refused("furthest_point_sample: expected points_xyz[B,N,3] and 0 < num_points <= N", m.furthest_point_sample, F(1, 4, 2), 2)
    refused(f"points_xyz: {floating}", m.furthest_point_sample, I(1, 4, 3), 2)
    refused("gather_points: expected features[B,C,N], indices[B,M]", m.gather_points, F(1, 2, 4), I(2, 3))
    refused("gather_points: expected features[B,C,N], indices[B,M]", m.gather_points, F(1, 2, 4), I(1, 3, 1))
    refused(f"features: {floating}", m.gather_points, I(1, 2, 4), I(1, 3))
    refused("indices: expected int32 / int64 indices, got torch.float32", m.gather_points, F(1, 2, 4), F(1, 3))
    refused("indices: index out of range [0, 4)", m.gather_points, F(1, 2, 4), torch.tensor([[0, 4, 1]], dtype=torch.int32))
    refused("indices: index out of range [0, 4)", m.gather_points, F(1, 2, 4), torch.tensor([[0, -1, 1]]))
    refused("grouping_operation: expected features[B,C,N], indices[B,npoint,nsample]", m.grouping_operation, F(1, 2, 4), I(1, 3))
    refused("grouping_operation: expected features[B,C,N], indices[B,npoint,nsample]", m.grouping_operation, F(1, 2, 4), I(2, 3, 2))
    refused(f"features: {floating}", m.grouping_operation, I(1, 2, 4), I(1, 3, 2))
    refused("indices: index out of range [0, 4)", m.grouping_operation, F(1, 2, 4), torch.full((1, 3, 2), 4))
    ti = "three_interpolate: expected features[B,C,M], indices[B,N,3], weight[B,N,3]"
    refused(ti, m.three_interpolate, F(1, 2, 4), I(1, 3, 2), F(1, 3, 2))
    refused(ti, m.three_interpolate, F(1, 2, 4), I(1, 3, 3), F(1, 2, 3))
    refused(ti, m.three_interpolate, F(2, 2, 4), I(1, 3, 3), F(1, 3, 3))
    refused(f"weight: {floating}", m.three_interpolate, F(1, 2, 4), I(1, 3, 3), I(1, 3, 3))
    refused("indices: index out of range [0, 4)", m.three_interpolate, F(1, 2, 4), torch.full((1, 3, 3), 7), F(1, 3, 3))
    bq = "ball_query: expected xyz[B,N>=1,3], center_xyz[B,npoint,3]"
    refused(bq, m.ball_query, 0, 1, 2, F(1, 4, 3), F(2, 2, 3))
    refused(bq, m.ball_query, 0, 1, 2, F(1, 0, 3), F(1, 2, 3))
    refused(bq, m.ball_query, 0, 1, 2, F(1, 4, 3), F(1, 2, 2))
    refused("ball_query: expected 1 <= sample_num <= 64 and min_radius < max_radius", m.ball_query, 0, 1, 65, F(1, 4, 3), F(1, 2, 3))
    refused("ball_query: expected 1 <= sample_num <= 64 and min_radius < max_radius", m.ball_query, 0, 1, 0, F(1, 4, 3), F(1, 2, 3))
    refused("ball_query: expected 1 <= sample_num <= 64 and min_radius < max_radius", m.ball_query, 1, 1, 2, F(1, 4, 3), F(1, 2, 3))
    refused(f"xyz: {floating}", m.ball_query, 0, 1, 2, I(1, 4, 3), F(1, 2, 3))
    kc = "knn_cross: expected query[B,N,3], ref[B,M,3] and 1 <= k <= min(32, M)"
    refused(kc, m.knn_cross, 5, F(1, 2, 3), F(1, 4, 3))
    refused(kc, m.knn_cross, 0, F(1, 2, 3), F(1, 4, 3))
    refused(kc, m.knn_cross, 33, F(1, 2, 3), F(1, 40, 3))
    refused(kc, m.knn_cross, 2, F(1, 2, 3), F(2, 4, 3))
    refused(f"ref: {floating}", m.knn_cross, 2, F(1, 2, 3), I(1, 4, 3))
    refused("three_nn: expected target[B,N,3], source[B,M>=3,3]", m.three_nn, F(1, 2, 3), F(1, 2, 3))
    refused("three_nn: expected target[B,N,3], source[B,M>=3,3]", m.three_nn, F(1, 2, 3), F(2, 3, 3))
    refused(f"source: {floating}", m.three_nn, F(1, 2, 3), I(1, 3, 3))
    with pytest.raises(NotImplementedError, match="uniform_sample / return_unique_cnt are not built"):
        m.QueryAndGroup(1.0, 4, uniform_sample=True)
    with pytest.raises(ValueError, match="normalize_xyz needs a max_radius"):
        m.QueryAndGroup(None, 4, normalize_xyz=True)
    with pytest.raises(ValueError, match="without features, use_xyz must be set"):
        m.QueryAndGroup(1.0, 4, use_xyz=False)(F(1, 4, 3), F(1, 2, 3))
