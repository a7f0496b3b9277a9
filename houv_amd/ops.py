"""Thin Python operators over the C ABI (include/houv_hip.h), plus their registration as PyTorch-ROCm
custom ops ``torch.ops.houv.*``.  Outputs are caller-allocated and written in place, as in the reference's
pybind module (utils/metrics/CD/chamfer3D/chamfer_cuda.cpp:17-33)."""
import torch

from . import _lib

_F32, _I32, _F64 = torch.float32, torch.int32, torch.float64


def _want(t, dtype, name):
    if t.dtype != dtype:
        raise _lib.HouvHipError(f"{name}: expected {dtype}, got {t.dtype}")


def chamfer_forward(xyz1, xyz2, dist1, dist2, idx1, idx2):
    """``chamfer_3D.forward(xyz1, xyz2, dist1, dist2, idx1, idx2)`` (chamfer_cuda.cpp:17-19). Returns 1."""
    _lib.require_gpu(xyz1, xyz2, dist1, dist2, idx1, idx2)
    for t, d, n in ((xyz1, _F32, "xyz1"), (xyz2, _F32, "xyz2"), (dist1, _F32, "dist1"), (dist2, _F32, "dist2"),
                    (idx1, _I32, "idx1"), (idx2, _I32, "idx2")):
        _want(t, d, n)
    B, N, _ = xyz1.shape
    M = xyz2.shape[1]
    if xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz2.shape[0] != B:
        raise _lib.HouvHipError("chamfer_forward: expected xyz1[B,N,3], xyz2[B,M,3]")
    if dist1.numel() != B * N or idx1.numel() != B * N or dist2.numel() != B * M or idx2.numel() != B * M:
        raise _lib.HouvHipError("chamfer_forward: output shapes do not match [B,N] / [B,M]")
    _lib.call("houv_chamfer_forward", xyz1, xyz1, xyz2, B, N, M, dist1, dist2, idx1, idx2)
    return 1


def chamfer_backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2):
    """``chamfer_3D.backward(...)`` with the reference's argument order (chamfer_cuda.cpp:22-26).
    Accumulates into the (caller zero-filled) gradxyz1/gradxyz2."""
    _lib.require_gpu(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2)
    for t, d, n in ((xyz1, _F32, "xyz1"), (xyz2, _F32, "xyz2"), (gradxyz1, _F32, "gradxyz1"),
                    (gradxyz2, _F32, "gradxyz2"), (graddist1, _F32, "graddist1"), (graddist2, _F32, "graddist2"),
                    (idx1, _I32, "idx1"), (idx2, _I32, "idx2")):
        _want(t, d, n)
    B, N, _ = xyz1.shape
    M = xyz2.shape[1]
    if (gradxyz1.shape != xyz1.shape or gradxyz2.shape != xyz2.shape or graddist1.numel() != B * N
            or graddist2.numel() != B * M or idx1.numel() != B * N or idx2.numel() != B * M):
        raise _lib.HouvHipError("chamfer_backward: shape mismatch")
    _lib.call("houv_chamfer_backward", xyz1, xyz1, xyz2, B, N, M, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2)
    return 1


def kabsch(src, corr, weights=None):
    """Batched Kabsch: src, corr [B,3,N]; weights [B,1,N] or None -> R[B,3,3], t[B,3]
    (SVDHead.forward, registration/model_utils.py:220-255)."""
    _lib.require_gpu(src, corr, weights)
    _want(src, _F32, "src"); _want(corr, _F32, "corr")
    B, C, N = src.shape
    if C != 3 or corr.shape != src.shape:
        raise _lib.HouvHipError("kabsch: expected src, corr [B,3,N]")
    if weights is not None:
        _want(weights, _F32, "weights")
        if weights.numel() != B * N:
            raise _lib.HouvHipError("kabsch: expected weights [B,1,N]")
    R = torch.empty((B, 3, 3), dtype=_F32, device=src.device)
    t = torch.empty((B, 3), dtype=_F32, device=src.device)
    _lib.call("houv_kabsch", src, src, corr, weights, B, N, R, t)
    return R, t


def pose_forward(params, angle_base, trans_mode=0, src=None):
    """params fp32 [n,8] -> (R[n,3,3], T[n,3]) and, with src[n,N,3], moved[n,N,3] (houv.py:94-103)."""
    _lib.require_gpu(params, src)
    _want(params, _F32, "params")
    n = params.shape[0]
    R = torch.empty((n, 3, 3), dtype=_F32, device=params.device)
    T = torch.empty((n, 3), dtype=_F32, device=params.device)
    moved, N = None, 0
    if src is not None:
        _want(src, _F32, "src")
        N = src.shape[1]
        moved = torch.empty_like(src)
    _lib.call("houv_pose_forward", params, params, n, angle_base, trans_mode, src, N, R, T, moved)
    return (R, T) if src is None else (R, T, moved)


def _solve_args(who, src, tgt, state, K):
    """(P, N, M, P*K) of the solve entries' clouds src[P,N,3], tgt[P,M,3] and state [P*K,24] fp64."""
    _want(src, _F32, "src"); _want(tgt, _F32, "tgt"); _want(state, _F64, "state")
    P, N, _ = src.shape
    M = tgt.shape[1]
    if tgt.shape[0] != P or src.shape[2] != 3 or tgt.shape[2] != 3:
        raise _lib.HouvHipError(f"{who}: expected src[P,N,3], tgt[P,M,3]")
    n = P * int(K)
    if tuple(state.shape) != (n, 24):
        raise _lib.HouvHipError(f"{who}: state must be [{n},24], got {tuple(state.shape)}")
    return P, N, M, n


def _want_nn_ws(nn_ws, n, who):
    """The pruned search's workspace for n hypotheses (solve_workspace)."""
    if (nn_ws is None or nn_ws.dtype != torch.int16 or nn_ws.dim() != 3 or tuple(nn_ws.shape[:2]) != (n, 16)
            or not nn_ws.is_contiguous()):
        raise _lib.HouvHipError(f"{who}: nn_ws must be a contiguous int16 [P*K,16,stride] tensor (ops.solve_workspace)")


def solve_iterate_out(src, tgt, state, K, steps_done, n_iters, angle_base, trans_mode, use_views, f64_params, k_full,
                      k_view, lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad=None,
                      out_cd=None, nn_ws=None, ws_valid=0, large=False, chunk_iters=None, sched_ws=None):
    """The C-ABI call itself, caller-allocated outputs (``houv_solve_iterate`` / ``houv_solve_iterate_pruned`` when a
    workspace is given / ``houv_solve_iterate_large`` with ``large``): what ``torch.ops.houv.solve_iterate[_pruned|_large]``
    bind.  ``state`` [P*K,24] fp64 (and ``nn_ws``) are updated in place; the out_* tensors receive the LAST forward's values.
    With ``sched_ws`` (solve_sched_workspace) the call is ``houv_solve_stage[_pruned]``: ``n_iters`` is a whole stage, run in one
    launch as items of ``chunk_iters`` iterations.  Returns 1."""
    _lib.require_gpu(src, tgt, state, out_score, out_loss, out_R, out_T, out_grad, out_cd, nn_ws, sched_ws)
    P, N, M, n = _solve_args("solve_iterate", src, tgt, state, K)
    for t, numel, name in ((out_score, n, "out_score"), (out_loss, n, "out_loss"), (out_R, 9 * n, "out_R"),
                           (out_T, 3 * n, "out_T"), (out_grad, 8 * n, "out_grad"), (out_cd, 8 * n, "out_cd")):
        if t is not None:
            _want(t, _F32, name)
            if t.numel() != numel:
                raise _lib.HouvHipError(f"solve_iterate: {name} must hold {numel} floats, got {t.numel()}")
    stage = sched_ws is not None
    if large and nn_ws is not None:
        raise _lib.HouvHipError("solve_iterate: the large-cloud kernel is a brute-force sweep and takes no workspace")
    if large and stage:
        raise _lib.HouvHipError("solve_iterate: the large-cloud kernel has no stage form")
    name = ("houv_solve_stage" if stage else "houv_solve_iterate") + ("_large" if large else "_pruned" if nn_ws is not None else "")
    if stage and (sched_ws.dtype != torch.int32 or sched_ws.numel() < 4 + n):
        raise _lib.HouvHipError(f"solve_iterate: sched_ws must hold {4 + n} int32 (ops.solve_sched_workspace)")
    ws = sched = ()         # the tails the entry has: _lib._SOLVE_WS, _lib._SOLVE_SCHED
    if nn_ws is not None:   # exact pruned search: nn_ws int16 [P*K, 16, stride] (solve_workspace) persists between chunked launches
        _want_nn_ws(nn_ws, n, "solve_iterate")
        ws = (nn_ws, ws_valid, nn_ws.shape[2])
    if stage:
        sched = (chunk_iters, sched_ws)
    _lib.call(name, src, src, tgt, P, N, M, K, state, steps_done, n_iters, angle_base, trans_mode, bool(use_views), bool(f64_params),
              k_full, k_view, lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd, *ws, *sched)
    return 1


def solve_iterate_large_out(src, tgt, state, K, steps_done, n_iters, angle_base, trans_mode, use_views, f64_params, k_full,
                            k_view, lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad=None,
                            out_cd=None):
    """``houv_solve_iterate_large`` (clouds of up to 16384 points, none resident in LDS) with solve_iterate_out's arguments:
    what ``torch.ops.houv.solve_iterate_large`` binds."""
    return solve_iterate_out(src, tgt, state, K, steps_done, n_iters, angle_base, trans_mode, use_views, f64_params, k_full,
                             k_view, lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd,
                             large=True)


def solve_workspace(n_hypotheses, N, M, device):
    """Workspace of houv_solve_iterate_pruned for n hypotheses on clouds of N and M points: int16 [n, 16, stride] (rows 0..7
    the remembered nearest neighbours, one 4 x int16 record per point and direction; rows 8..15 scratch), stride = max(N, M)
    rounded up to 8.  The library needs the base 16-byte aligned (a fresh allocation is)."""
    stride = (max(int(N), int(M)) + 7) // 8 * 8
    return torch.empty((int(n_hypotheses), 16, stride), dtype=torch.int16, device=device)


def solve_seed(src, tgt, state, K, angle_base, trans_mode, use_views, nn_ws):
    """houv_solve_seed: first-guess neighbour records for the poses of ``state`` [P*K,24] fp64 written into ``nn_ws``
    (solve_workspace), so that the next solve_iterate on them may start with ``ws_valid=True``: its first iteration then runs the
    pruned search instead of the brute-force sweep, with the same results.  Clouds of 257..4096 points.  Returns 1."""
    _lib.require_gpu(src, tgt, state, nn_ws)
    P, N, M, n = _solve_args("solve_seed", src, tgt, state, K)
    _want_nn_ws(nn_ws, n, "solve_seed")
    _lib.call("houv_solve_seed", src, src, tgt, P, N, M, K, state, angle_base, trans_mode, bool(use_views), nn_ws, nn_ws.shape[2])
    return 1


def solve_sched_workspace(n_hypotheses, device):
    """Scheduling workspace of houv_solve_stage[_pruned] for n hypotheses: int32 [4 + n] (ticket counter, status word, two spares,
    done[h]).  One per stage in flight; the call zeroes it.  Word 1 is the status: non-zero after the launch = the stage failed."""
    return torch.empty(4 + int(n_hypotheses), dtype=torch.int32, device=device)


def solve_iterate(src, tgt, state, K, *, steps_done, n_iters, angle_base, trans_mode, use_views, f64_params, k_full,
                  k_view, lr, loss_scale, betas=(0.9, 0.999), eps=1e-8, want_grad=False, want_cd=False, nn_ws=None,
                  ws_valid=False, large=False, chunk_iters=None, sched_ws=None):
    """One launch of the fused HOUV loop (houv_solve_iterate; ``large``: houv_solve_iterate_large, clouds of up to 16384
    points; with ``sched_ws``: houv_solve_stage, a whole stage as items of ``chunk_iters`` iterations).  ``state`` [P*K,24] fp64 is updated in place.
    Returns dict(score[P*K], loss[P*K], R[P*K,3,3], T[P*K,3][, grad[P*K,8]][, cd[P*K,8]]) of the LAST forward."""
    _lib.require_gpu(src, tgt, state)
    dev = src.device
    n = src.shape[0] * int(K)
    out = dict(score=torch.empty(n, dtype=_F32, device=dev), loss=torch.empty(n, dtype=_F32, device=dev),
               R=torch.empty((n, 3, 3), dtype=_F32, device=dev), T=torch.empty((n, 3), dtype=_F32, device=dev))
    if want_grad:
        out["grad"] = torch.empty((n, 8), dtype=_F32, device=dev)
    if want_cd:
        out["cd"] = torch.empty((n, 8), dtype=_F32, device=dev)
    solve_iterate_out(src, tgt, state, K, steps_done, n_iters, angle_base, trans_mode, use_views, f64_params, k_full,
                      k_view, lr, betas[0], betas[1], eps, loss_scale, out["score"], out["loss"], out["R"], out["T"],
                      out.get("grad"), out.get("cd"), nn_ws, -1 if ws_valid == "verify" else int(bool(ws_valid)), large=large,
                      chunk_iters=chunk_iters, sched_ws=sched_ws)
    return out


KD_RULES = {"area": 0, "extent": 1}


def kd_sort(cloud, leaf=32, rule="area", return_order=False):
    """houv_kd_sort: cloud[P,N,3] fp32 (N <= 4096) reordered into the k-d leaf order of ``solver.kd_sort(cloud, leaf, rule)``, bit for
    bit.  Returns the sorted cloud, and with ``return_order`` also order[P,N] int32 (input index of each output point)."""
    _lib.require_gpu(cloud)
    _want(cloud, _F32, "cloud")
    if cloud.dim() != 3 or cloud.shape[2] != 3:
        raise _lib.HouvHipError("kd_sort: expected cloud[P,N,3]")
    if rule not in KD_RULES:
        raise _lib.HouvHipError(f"kd_sort: rule must be one of {sorted(KD_RULES)}, got {rule!r}")
    P, N, _ = cloud.shape
    out = torch.empty_like(cloud)
    order = torch.empty((P, N), dtype=_I32, device=cloud.device) if return_order else None
    _lib.call("houv_kd_sort", cloud, cloud, P, N, leaf, KD_RULES[rule], out, order)
    return (out, order) if return_order else out


def icp_refine(src, tgt, init=None, max_correspondence_distance=0.02, max_iteration=500, relative_fitness=1e-6,
               relative_rmse=1e-6):
    """Batched point-to-point ICP (houv_icp_refine; Open3D registration_icp semantics, train_ICP.py:148-151).
    src[P,N,3], tgt[P,M,3], init[P,4,4]|None -> dict(T[P,4,4], fitness[P], inlier_rmse[P], iterations[P])."""
    _lib.require_gpu(src, tgt, init)
    _want(src, _F32, "src"); _want(tgt, _F32, "tgt")
    P, N, _ = src.shape
    M = tgt.shape[1]
    if tgt.shape[0] != P or src.shape[2] != 3 or tgt.shape[2] != 3:
        raise _lib.HouvHipError("icp_refine: expected src[P,N,3], tgt[P,M,3]")
    if init is not None:
        _want(init, _F32, "init")
        if tuple(init.shape) != (P, 4, 4):
            raise _lib.HouvHipError("icp_refine: init must be [P,4,4]")
    dev = src.device
    T = torch.empty((P, 4, 4), dtype=_F32, device=dev)
    fit = torch.empty(P, dtype=_F32, device=dev)
    rmse = torch.empty(P, dtype=_F32, device=dev)
    iters = torch.empty(P, dtype=_I32, device=dev)
    _lib.call("houv_icp_refine", src, src, tgt, P, N, M, init, max_correspondence_distance, max_iteration, relative_fitness,
              relative_rmse, T, fit, rmse, iters)
    return dict(T=T, fitness=fit, inlier_rmse=rmse, iterations=iters)


def emd_workspace(B, N, device):
    """The workspace houv_emd_forward needs for B clouds of N points (uint8, houv_emd_workspace_bytes), None when it needs none
    (N <= 4096)."""
    return _lib.workspace("houv_emd_workspace_bytes", device, B, N, floor=0)[0]


def emd_forward(xyz1, xyz2, eps, iters, workspace=None):
    """Auction EMD (houv_emd_forward; the reference's ``emd.forward``, utils/metrics/EMD/emd_cuda.cu, made exact).
    xyz1[B,N,3] (bidders, the prediction), xyz2[B,N,3] (objects, the ground truth), any float dtype and layout: converted to
    contiguous fp32 as the reference does.  Returns (dist[B,N] squared distances fp32, assignment[B,N] int32,
    iters_run[B] int32).  Clouds above 4096 points take a workspace: ``workspace`` or one allocated here with torch."""
    _lib.require_gpu(xyz1.contiguous(), xyz2.contiguous())
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0]:
        raise _lib.HouvHipError("emd_forward: expected xyz1[B,N,3], xyz2[B,N,3]")
    xyz1 = xyz1.contiguous().to(_F32)
    xyz2 = xyz2.contiguous().to(_F32)
    B, N, _ = xyz1.shape
    M = xyz2.shape[1]
    dev = xyz1.device
    dist = torch.empty((B, N), dtype=_F32, device=dev)
    assignment = torch.empty((B, N), dtype=_I32, device=dev)
    iters_run = torch.empty((B,), dtype=_I32, device=dev)
    if workspace is None and N == M:
        workspace = emd_workspace(B, N, dev)
    if workspace is not None:
        _lib.require_gpu(workspace, xyz1)
        need = _lib.load().houv_emd_workspace_bytes(int(B), int(N))
        if workspace.numel() * workspace.element_size() < need:
            raise _lib.HouvHipError(f"emd_forward: the workspace holds fewer than the {need} bytes needed")
    _lib.call("houv_emd_forward", xyz1, xyz1, xyz2, B, N, M, eps, iters, dist, assignment, iters_run, workspace)
    return dist, assignment, iters_run


def emd_backward(xyz1, xyz2, graddist, assignment):
    """Gradient of emd_forward's dist for xyz1 (houv_emd_backward; the reference's ``emd.backward``):
    (2 * graddist) * (xyz1 - xyz2[assignment]), fp32 [B,N,3].  The reference returns zeros for xyz2."""
    xyz1 = xyz1.contiguous().to(_F32)
    xyz2 = xyz2.contiguous().to(_F32)
    graddist = graddist.contiguous().to(_F32)
    _lib.require_gpu(xyz1, xyz2, graddist, assignment)
    _want(assignment, _I32, "assignment")
    B, N, _ = xyz1.shape
    if xyz2.shape != xyz1.shape or graddist.numel() != B * N or assignment.numel() != B * N:
        raise _lib.HouvHipError("emd_backward: shape mismatch")
    gradxyz1 = torch.zeros_like(xyz1)
    _lib.call("houv_emd_backward", xyz1, xyz1, xyz2, B, N, graddist, assignment, gradxyz1)
    return gradxyz1


# ---------------------------------------------------------------------------------------------------
# DeepGMR head (houv_rri_features, houv_gmm_params, houv_gmm_register)
# ---------------------------------------------------------------------------------------------------
def rri_features(xyz, idx, k, skip=0):
    """xyz[B,N,3], idx[B,N,L] int32 neighbour lists into the same cloud -> out[B,N,4k]: (|p|, |q_j|, theta_j, phi_j) for the
    neighbours idx[..., skip:skip+k], channel 4*j + f (get_rri_cluster, registration/models/deepgmr.py:54-95).  2 <= k <= 31."""
    _lib.require_gpu(xyz, idx)
    _want(xyz, _F32, "xyz"); _want(idx, _I32, "idx")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or idx.dim() != 3 or idx.shape[:2] != xyz.shape[:2]:
        raise _lib.HouvHipError("rri_features: expected xyz[B,N,3], idx[B,N,L]")
    B, N, _ = xyz.shape
    out = torch.empty((B, N, 4 * int(k)), dtype=_F32, device=xyz.device)
    _lib.call("houv_rri_features", xyz, xyz, idx, B, N, k, idx.shape[2], skip, out)
    return out


def _gmm_params_args(who, gamma, pts, **more):
    """(B, N, J) of gamma[B,N,J], pts[B,N,3]; `more`: the backward's further fp32 operands by name."""
    ts = dict(gamma=gamma, pts=pts, **more)
    _lib.require_gpu(*ts.values())
    for n, t in ts.items():
        _want(t, _F32, n)
    if gamma.dim() != 3 or pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[:2] != gamma.shape[:2]:
        raise _lib.HouvHipError(f"{who}: expected gamma[B,N,J], pts[B,N,3]")
    return gamma.shape


def _gmm_register_args(who, pi_s, mu_s, mu_t, sigma_t, *g_T):
    """(B, J) of pi_s[B,J], mu_s[B,J,3], mu_t[B,J,3], sigma_t[B,J] and, when the backward passes it, g_T[B,4,4]."""
    ts = (pi_s, mu_s, mu_t, sigma_t) + g_T
    _lib.require_gpu(*ts)
    for t, n in zip(ts, ("pi_s", "mu_s", "mu_t", "sigma_t", "g_T")):
        _want(t, _F32, n)
    if pi_s.dim() != 2 or tuple(mu_s.shape) != tuple(pi_s.shape) + (3,) or mu_t.shape != mu_s.shape or sigma_t.shape != pi_s.shape \
            or any(tuple(g.shape) != (pi_s.shape[0], 4, 4) for g in g_T):
        raise _lib.HouvHipError(f"{who}: expected pi_s[B,J], mu_s[B,J,3], mu_t[B,J,3], sigma_t[B,J]" + (", g_T[B,4,4]" if g_T else ""))
    return pi_s.shape


def gmm_params(gamma, pts):
    """gamma[B,N,J] (J <= 32), pts[B,N,3] -> (pi[B,J], mu[B,J,3], sigma[B,J]): deepgmr.py:98-120 with the isotropic covariance kept
    as its scalar (the reference returns sigma * eye(3))."""
    B, N, J = _gmm_params_args("gmm_params", gamma, pts)
    pi = torch.empty((B, J), dtype=_F32, device=gamma.device)
    mu = torch.empty((B, J, 3), dtype=_F32, device=gamma.device)
    sigma = torch.empty((B, J), dtype=_F32, device=gamma.device)
    _lib.call("houv_gmm_params", gamma, gamma, pts, B, N, J, pi, mu, sigma)
    return pi, mu, sigma


def gmm_register(pi_s, mu_s, mu_t, sigma_t):
    """pi_s[B,J], mu_s[B,J,3], mu_t[B,J,3], sigma_t[B,J] -> T[B,4,4], bottom row (0,0,0,1) (deepgmr.py:123-143)."""
    B, J = _gmm_register_args("gmm_register", pi_s, mu_s, mu_t, sigma_t)
    T = torch.empty((B, 4, 4), dtype=_F32, device=pi_s.device)
    _lib.call("houv_gmm_register", pi_s, pi_s, mu_s, mu_t, sigma_t, B, J, T)
    return T


# ---------------------------------------------------------------------------------------------------
# DeepGMR training (houv_gmm_params_backward, houv_gmm_register_backward, houv_bn_rows_stats, houv_bn_relu_rows,
# houv_bn_relu_rows_backward)
# ---------------------------------------------------------------------------------------------------
def gmm_params_backward(gamma, pts, pi, mu, sigma, g_pi, g_mu, g_sigma):
    """The gradient of (pi, mu, sigma) = gmm_params(softmax(logits), pts) with respect to the logits, softmax backward
    included: gamma[B,N,J], pts[B,N,3], pi / mu / sigma as gmm_params returned them, their gradients -> g_logits[B,N,J]."""
    B, N, J = _gmm_params_args("gmm_params_backward", gamma, pts, pi=pi, mu=mu, sigma=sigma, g_pi=g_pi, g_mu=g_mu, g_sigma=g_sigma)
    if any(tuple(t.shape) != (B, J) for t in (pi, sigma, g_pi, g_sigma)) or any(tuple(t.shape) != (B, J, 3) for t in (mu, g_mu)):
        raise _lib.HouvHipError("gmm_params_backward: expected pi / sigma and their gradients [B,J], mu / g_mu [B,J,3]")
    g_logits = torch.empty_like(gamma)
    _lib.call("houv_gmm_params_backward", gamma, gamma, pts, pi, mu, sigma, g_pi, g_mu, g_sigma, B, N, J, g_logits)
    return g_logits


def gmm_register_backward(pi_s, mu_s, mu_t, sigma_t, g_T):
    """The gradient of T = gmm_register(pi_s, mu_s, mu_t, sigma_t): g_T[B,4,4] -> (g_pi_s[B,J], g_mu_s[B,J,3], g_mu_t[B,J,3],
    g_sigma_t[B,J]); the polar form of the rotation's derivative, in float64 registers."""
    B, J = _gmm_register_args("gmm_register_backward", pi_s, mu_s, mu_t, sigma_t, g_T)
    outs = (torch.empty_like(pi_s), torch.empty_like(mu_s), torch.empty_like(mu_t), torch.empty_like(sigma_t))
    _lib.call("houv_gmm_register_backward", pi_s, pi_s, mu_s, mu_t, sigma_t, g_T, B, J, *outs)
    return outs


def _bn_rows(z, name):
    """(R, C, ld) of rows z[R,C]: a row-major view whose columns are contiguous (a column slice of a wider buffer is fine)."""
    _lib.require_gpu_any(z)
    if z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1 or z.stride(1) != 1 or z.stride(0) < z.shape[1]:
        raise _lib.HouvHipError(f"{name}: expected rows [R,C] with contiguous columns and a row stride >= C")
    return z.shape[0], z.shape[1], z.stride(0)


def _bn_vectors(C, *vs):
    for v in vs:
        _lib.require_gpu(v); _want(v, _F32, "per-channel vector")
        if tuple(v.shape) != (C,):
            raise _lib.HouvHipError(f"bn_rows: expected per-channel vectors of {C} elements")


def bn_rows_stats(z):
    """z[R,C] (R >= 2, any row stride) -> (mean[C], var[C]): the batch statistics of training-mode BatchNorm, var biased about
    the mean.  Ordered sums: the same bits from call to call."""
    R, C, ld = _bn_rows(z, "bn_rows_stats")
    mean = torch.empty((C,), dtype=_F32, device=z.device)
    var = torch.empty((C,), dtype=_F32, device=z.device)
    ws, nbytes = _lib.workspace("houv_bn_rows_workspace_bytes", z.device, R, C, 0)
    _lib.call("houv_bn_rows_stats", z, z, R, C, ld, mean, var, ws, nbytes)
    return mean, var


def bn_relu_rows(z, mean, var, weight, bias, eps=1e-5, relu=True, n_group=0):
    """y[R,C] = relu?((z - mean) * rsqrt(var + eps) * weight + bias).  With n_group > 0 (a divisor of R) returns
    (y, gmax[R/n_group,C], garg[R/n_group,C] int32): the column maximum of y over each group of n_group rows and the lowest row
    index, counted over all R rows, that attains it -- a cloud's max-pool from the same read."""
    R, C, ld = _bn_rows(z, "bn_relu_rows")
    _bn_vectors(C, mean, var, weight, bias)
    n_group = int(n_group)
    if n_group < 0 or (n_group and R % n_group):
        raise _lib.HouvHipError(f"bn_relu_rows: n_group = {n_group} does not divide the {R} rows")
    y = torch.empty((R, C), dtype=_F32, device=z.device)
    gmax = garg = None
    if n_group:
        gmax = torch.empty((R // n_group, C), dtype=_F32, device=z.device)
        garg = torch.empty((R // n_group, C), dtype=_I32, device=z.device)
    ws, nbytes = _lib.workspace("houv_bn_rows_workspace_bytes", z.device, R, C, n_group)
    _lib.call("houv_bn_relu_rows", z, z, R, C, ld, mean, var, weight, bias, eps, bool(relu), n_group, y, C, gmax, garg, ws, nbytes)
    return (y, gmax, garg) if n_group else y


def bn_relu_rows_backward(gy, z, mean, var, weight, bias, eps=1e-5, relu=True, inplace=False):
    """The backward of bn_relu_rows under batch statistics: gy[R,C] -> (gz[R,C], gweight[C], gbias[C]); the ReLU mask and xhat
    are recomputed from z.  inplace: gz overwrites gy."""
    R, C, ld = _bn_rows(z, "bn_relu_rows_backward")
    Rg, Cg, ldg = _bn_rows(gy, "bn_relu_rows_backward")
    if (Rg, Cg) != (R, C):
        raise _lib.HouvHipError("bn_relu_rows_backward: gy and z differ in shape")
    _bn_vectors(C, mean, var, weight, bias)
    gz = gy if inplace else torch.empty((R, C), dtype=_F32, device=z.device)
    gweight = torch.empty((C,), dtype=_F32, device=z.device)
    gbias = torch.empty((C,), dtype=_F32, device=z.device)
    ws, nbytes = _lib.workspace("houv_bn_rows_workspace_bytes", z.device, R, C, 0)
    _lib.call("houv_bn_relu_rows_backward", z, gy, ldg, z, R, C, ld, mean, var, weight, bias, eps, bool(relu), gz, gz.stride(0),
              gweight, gbias, ws, nbytes)
    return gz, gweight, gbias


# ---------------------------------------------------------------------------------------------------
# IDAM head (houv_idam_simmat, houv_edge_diff)
# ---------------------------------------------------------------------------------------------------
def idam_simmat(src, tgt, es, et, W1, s1, t1, W2, b2, W3, s3, t3, w4, b4, want_rowmax=True, want_idx=True, want_corr=True,
                want_scores=False):
    """One IDAM iteration's similarity stage (registration/models/idam.py:267-320) in one kernel.  src[B,Ms,3], tgt[B,Mt,3],
    es[B,Ms,E], et[B,Mt,E]; W1[32,2E+4], s1, t1, W2[32,32], b2, W3[32,32], s3, t3, w4 [32], b4 [1] (BatchNorm folded) ->
    (rowmax[B,Ms,32], corr_idx[B,Ms] int32, corr[B,3,Ms], scores[B,Ms,Mt]), None for an output not asked for."""
    par = (W1, s1, t1, W2, b2, W3, s3, t3, w4, b4)
    _lib.require_gpu(src, tgt, es, et, *par)
    for t in (src, tgt, es, et) + par:
        _want(t, _F32, "idam_simmat")
    if src.dim() != 3 or tgt.dim() != 3 or es.dim() != 3 or et.dim() != 3 or src.shape[2] != 3 or tgt.shape[2] != 3 \
            or es.shape[:2] != src.shape[:2] or et.shape[:2] != tgt.shape[:2] or tgt.shape[0] != src.shape[0] \
            or et.shape[2] != es.shape[2]:
        raise _lib.HouvHipError("idam_simmat: expected src[B,Ms,3], tgt[B,Mt,3], es[B,Ms,E], et[B,Mt,E]")
    B, Ms, E = es.shape
    Mt = tgt.shape[1]
    if tuple(W1.shape) != (32, 2 * E + 4) or tuple(W2.shape) != (32, 32) or tuple(W3.shape) != (32, 32) or b4.numel() != 1 \
            or any(t.numel() != 32 for t in (s1, t1, b2, s3, t3, w4)):
        raise _lib.HouvHipError("idam_simmat: expected W1[32,2E+4], W2[32,32], W3[32,32], b4[1] and 32-element s1, t1, b2, s3, t3, w4")
    dev = src.device
    rowmax = torch.empty((B, Ms, 32), dtype=_F32, device=dev) if want_rowmax else None
    cidx = torch.empty((B, Ms), dtype=_I32, device=dev) if want_idx else None
    corr = torch.empty((B, 3, Ms), dtype=_F32, device=dev) if want_corr else None
    scores = torch.empty((B, Ms, Mt), dtype=_F32, device=dev) if want_scores else None
    _lib.call("houv_idam_simmat", src, src, tgt, es, et, B, Ms, Mt, E, *par, rowmax, cidx, corr, scores)
    return rowmax, cidx, corr, scores


def edge_diff(x, idx, k=None, ldo=None):
    """x[B,N,C], idx[B,N,L] int32 neighbour lists into the same cloud -> out[B*N*k, ldo] with out[(b*N+n)*k + j, :C] =
    x[b, idx[b,n,j]] - x[b,n] and zeros in columns C..ldo-1 (Propagate, registration/models/idam.py:121-124).  k defaults to
    L, ldo to C; an index outside 0..N-1 is clamped."""
    _lib.require_gpu(x, idx)
    _want(x, _F32, "x"); _want(idx, _I32, "idx")
    if x.dim() != 3 or idx.dim() != 3 or idx.shape[:2] != x.shape[:2]:
        raise _lib.HouvHipError("edge_diff: expected x[B,N,C], idx[B,N,L]")
    B, N, C = x.shape
    k = idx.shape[2] if k is None else int(k)
    ldo = C if ldo is None else int(ldo)
    out = torch.empty((B * N * k, ldo), dtype=_F32, device=x.device)
    _lib.call("houv_edge_diff", x, x, idx, B, N, k, C, idx.shape[2], ldo, out)
    return out


# ---------------------------------------------------------------------------------------------------
# PCN completion network (houv_mlp2_max, houv_pcn_fold)
# ---------------------------------------------------------------------------------------------------
PCN_ROW_TILE = 64      # HOUV_PCN_ROW_TILE: points per workgroup of both kernels (a partial tile begins at its multiples)


def _mlp2_dims(who, x, W1, W2, *b2):
    """(B, N, Cin, H, Cout) of a PointNet block's x[B,N,Cin], W1[H,Cin], W2[Cout,H]; the forward passes its b2[Cout] as well."""
    if x.dim() != 3 or W1.dim() != 2 or W2.dim() != 2 or W1.shape[1] != x.shape[2] or W2.shape[1] != W1.shape[0] \
            or any(b.numel() != W2.shape[0] for b in b2):
        raise _lib.HouvHipError(f"{who}: expected x[B,N,Cin], W1[H,Cin], W2[Cout,H]{', b2[Cout]' if b2 else ''}, got "
                                + ", ".join(str(tuple(t.shape)) for t in (x, W1, W2) + b2))
    return x.shape[0], x.shape[1], x.shape[2], W1.shape[0], W2.shape[0]


def _shift1_stride(who, shift1, B, H):
    """The row stride the entries are told for shift1: 0 for one bias [H] shared by all clouds, H for one row per cloud [B,H]."""
    if tuple(shift1.shape) not in ((H,), (B, H)):
        raise _lib.HouvHipError(f"{who}: shift1 must be [{H}] or [{B},{H}], got {tuple(shift1.shape)}")
    return 0 if shift1.dim() == 1 else H


def _mlp2_forward_args(who, x, W1, shift1, W2, b2):
    """(B, N, Cin, H, Cout, shift1's row stride) of mlp2_max's and mlp2_max_arg's operands."""
    _lib.require_gpu(x, W1, shift1, W2, b2)
    for t, n in ((x, "x"), (W1, "W1"), (shift1, "shift1"), (W2, "W2"), (b2, "b2")):
        _want(t, _F32, f"{who}: {n}")
    B, N, Cin, H, Cout = _mlp2_dims(who, x, W1, W2, b2)
    return B, N, Cin, H, Cout, _shift1_stride(who, shift1, B, H)


def mlp2_max(x, W1, shift1, W2, b2, want_y=False):
    """One PointNet block in one kernel (houv_mlp2_max): x[B,N,Cin], W1[H,Cin], shift1[H] (one bias for all clouds) or [B,H]
    (one row per cloud), W2[Cout,H], b2[Cout] -> (pooled[B,Cout], y[B,N,Cout] or None) with
    y = W2 . relu(W1 . x + shift1) + b2 and pooled = y.max(1).  (Cin, H, Cout) = (3, 128, 256) or (256, 512, 1024)."""
    B, N, Cin, H, Cout, stride = _mlp2_forward_args("mlp2_max", x, W1, shift1, W2, b2)
    dev = x.device
    pooled = torch.empty((B, Cout), dtype=_F32, device=dev)
    y = torch.empty((B, N, Cout), dtype=_F32, device=dev) if want_y else None
    ws = _lib.workspace("houv_mlp2_max_workspace_bytes", dev, B, N, Cout, floor=0)[0]
    _lib.call("houv_mlp2_max", x, x, B, N, Cin, W1, H, shift1, stride, W2, b2, Cout, pooled, y, ws)
    return pooled, y


def mlp2_max_arg(x, W1, shift1, W2, b2, want_y=False):
    """mlp2_max that also says where each maximum sits (houv_mlp2_max_arg): the same arguments ->
    (pooled[B,Cout], arg[B,Cout] int32, y or None).  pooled and y carry mlp2_max's bits; arg[b,c] is the lowest n with
    y[b,n,c] == pooled[b,c] (torch.max's rule on the CPU), -1 for a column that is NaN in every row."""
    B, N, Cin, H, Cout, stride = _mlp2_forward_args("mlp2_max_arg", x, W1, shift1, W2, b2)
    dev = x.device
    pooled = torch.empty((B, Cout), dtype=_F32, device=dev)
    arg = torch.empty((B, Cout), dtype=_I32, device=dev)
    y = torch.empty((B, N, Cout), dtype=_F32, device=dev) if want_y else None
    ws = _lib.workspace("houv_mlp2_max_arg_workspace_bytes", dev, B, N, Cout, floor=0)[0]
    _lib.call("houv_mlp2_max_arg", x, x, B, N, Cin, W1, H, shift1, stride, W2, b2, Cout, pooled, arg, y, ws)
    return pooled, arg, y


def mlp2_max_backward(x, W1, shift1, W2, arg, gpooled, rows=None, nrows=None, gy_rows=None, want_gx=False):
    """The backward pass of one PointNet block on its active rows only (houv_mlp2_max_backward).
    x, W1, shift1, W2 as in mlp2_max; arg[B,Cout] int32 from mlp2_max_arg; gpooled[B,Cout]; optionally a gradient on y carried
    on rows[B,R] int32 (strictly ascending in the first nrows[b] entries), nrows[B] int32, gy_rows[B,R,Cout].
    -> dict(gW1[H,Cin], gshift1[B,H], gW2[Cout,H], gb2[Cout], act_rows[B,Rcap] int32, nact[B] int32, gx_rows[B,Rcap,Cin] or
    None): act_rows lists each cloud's active rows ascending (-1 past nact[b]) and gx_rows holds the input gradient of those
    rows (zeros past nact[b]) -- the (rows, nrows, gy_rows) of the block below."""
    ts = (x, W1, shift1, W2, gpooled)
    _lib.require_gpu(*ts, arg)
    for t, n in zip(ts, ("x", "W1", "shift1", "W2", "gpooled")):
        _want(t, _F32, f"mlp2_max_backward: {n}")
    _want(arg, _I32, "mlp2_max_backward: arg")
    B, N, Cin, H, Cout = _mlp2_dims("mlp2_max_backward", x, W1, W2)
    if tuple(arg.shape) != (B, Cout) or tuple(gpooled.shape) != (B, Cout):
        raise _lib.HouvHipError(f"mlp2_max_backward: arg and gpooled must be [{B},{Cout}], got {tuple(arg.shape)}, {tuple(gpooled.shape)}")
    stride = _shift1_stride("mlp2_max_backward", shift1, B, H)
    R = 0
    if rows is not None or nrows is not None or gy_rows is not None:
        if rows is None or nrows is None or gy_rows is None:
            raise _lib.HouvHipError("mlp2_max_backward: rows, nrows and gy_rows come together")
        _lib.require_gpu(rows, nrows, gy_rows)
        _want(rows, _I32, "mlp2_max_backward: rows"); _want(nrows, _I32, "mlp2_max_backward: nrows")
        _want(gy_rows, _F32, "mlp2_max_backward: gy_rows")
        if rows.dim() != 2 or rows.shape[0] != B or tuple(nrows.shape) != (B,) or tuple(gy_rows.shape) != (B, rows.shape[1], Cout):
            raise _lib.HouvHipError(f"mlp2_max_backward: expected rows[{B},R], nrows[{B}], gy_rows[{B},R,{Cout}], got "
                                    f"{tuple(rows.shape)}, {tuple(nrows.shape)}, {tuple(gy_rows.shape)}")
        R = rows.shape[1]
        if R == 0:
            rows = nrows = gy_rows = None
    dev = x.device
    rcap = _lib.load().houv_mlp2_max_backward_rows(N, Cout, R)
    out = dict(gW1=torch.empty((H, Cin), dtype=_F32, device=dev), gshift1=torch.empty((B, H), dtype=_F32, device=dev),
               gW2=torch.empty((Cout, H), dtype=_F32, device=dev), gb2=torch.empty((Cout,), dtype=_F32, device=dev),
               act_rows=torch.empty((B, rcap), dtype=_I32, device=dev), nact=torch.empty((B,), dtype=_I32, device=dev),
               gx_rows=torch.empty((B, rcap, Cin), dtype=_F32, device=dev) if want_gx else None)
    ws = _lib.workspace("houv_mlp2_max_backward_workspace_bytes", dev, B, N, Cin, H, Cout, R)[0]
    _lib.call("houv_mlp2_max_backward", x, x, B, N, Cin, W1, H, shift1, stride, W2, Cout, arg, gpooled, rows, nrows, gy_rows, R,
              *out.values(), ws)      # out: gW1, gshift1, gW2, gb2, act_rows, nact, gx_rows, the entry's order
    return out


def _pcn_fold_args(who, coarse, cvec, grid, Wgp, W2, b2, W3, b3, *gfine):
    """(B, nc, scale) of pcn_fold's operands; `gfine`: the backward's further fp32 operand (its shape is the backward's to check)."""
    ts = (coarse, cvec, grid, Wgp, W2, b2, W3, b3) + gfine
    _lib.require_gpu(*ts)
    for t in ts:
        _want(t, _F32, who)
    if coarse.dim() != 3 or coarse.shape[2] != 3 or grid.dim() != 2 or grid.shape[0] != 2 \
            or tuple(cvec.shape) != (coarse.shape[0], 512):
        raise _lib.HouvHipError(f"{who}: expected coarse[B,nc,3], cvec[B,512], grid[2,scale], got {tuple(coarse.shape)}, "
                                f"{tuple(cvec.shape)}, {tuple(grid.shape)}")
    if tuple(Wgp.shape) != (512, 5) or tuple(W2.shape) != (512, 512) or b2.numel() != 512 or tuple(W3.shape) != (3, 512) \
            or b3.numel() != 3:
        raise _lib.HouvHipError(f"{who}: expected Wgp[512,5], W2[512,512], b2[512], W3[3,512], b3[3]")
    return coarse.shape[0], coarse.shape[1], grid.shape[1]


def pcn_fold(coarse, cvec, grid, Wgp, W2, b2, W3, b3):
    """The folding stage of PCN_decoder.forward (registration/models/pcn.py:108-125) in one kernel (houv_pcn_fold):
    coarse[B,nc,3], cvec[B,512], grid[2,scale], Wgp[512,5], W2[512,512], b2[512], W3[3,512], b3[3] -> fine[B,nc*scale,3]."""
    B, nc, scale = _pcn_fold_args("pcn_fold", coarse, cvec, grid, Wgp, W2, b2, W3, b3)
    fine = torch.empty((B, nc * scale, 3), dtype=_F32, device=coarse.device)
    _lib.call("houv_pcn_fold", coarse, coarse, cvec, grid, B, nc, scale, Wgp, W2, b2, W3, b3, fine)
    return fine


def pcn_fold_backward(coarse, cvec, grid, Wgp, W2, b2, W3, b3, gfine):
    """The backward pass of pcn_fold (houv_pcn_fold_backward): pcn_fold's arguments plus
    gfine[B,nc*scale,3] -> dict(gcoarse[B,nc,3], gcvec[B,512], gWgp[512,5], gW2[512,512], gb2[512], gW3[3,512], gb3[3])."""
    B, nc, scale = _pcn_fold_args("pcn_fold_backward", coarse, cvec, grid, Wgp, W2, b2, W3, b3, gfine)
    if tuple(gfine.shape) != (B, nc * scale, 3):
        raise _lib.HouvHipError(f"pcn_fold_backward: gfine must be [{B},{nc * scale},3], got {tuple(gfine.shape)}")
    dev = coarse.device
    new = lambda *shape: torch.empty(shape, dtype=_F32, device=dev)
    out = dict(gcoarse=new(B, nc, 3), gcvec=new(B, 512), gWgp=new(512, 5), gW2=new(512, 512), gb2=new(512), gW3=new(3, 512), gb3=new(3))
    ws, nbytes = _lib.workspace("houv_pcn_fold_backward_workspace_bytes", dev, B, nc, scale)
    _lib.call("houv_pcn_fold_backward", coarse, coarse, cvec, grid, B, nc, scale, Wgp, W2, b2, W3, b3, gfine,
              *(out[k] for k in ("gcoarse", "gcvec", "gWgp", "gW2", "gb2", "gW3", "gb3")), ws, nbytes)
    return out


# ---------------------------------------------------------------------------------------------------
# ECG completion network (houv_knn_feat, houv_dense_conv)
# ---------------------------------------------------------------------------------------------------
KNN_FEAT_BLOCK, KNN_FEAT_CHUNK = 32, 16   # HOUV_KNN_FEAT_BLOCK / _CHUNK: candidates per register block, channels per chunk
DENSE_CONV_GROWTH = 24                     # HOUV_DENSE_CONV_GROWTH


def _rows(t, name):
    """(B, N, C, row stride) of a [B,N,C] view whose rows are contiguous and evenly spaced over the whole batch (a column slice
    of one row-major buffer qualifies)."""
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1) or t.stride(1) < t.shape[2]:
        raise _lib.HouvHipError(f"{name}: expected [B,N,C] rows with unit channel stride and one row stride, got shape "
                                f"{tuple(t.shape)} strides {tuple(t.stride())}")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1)


def knn_feat(x, k, want_dist=False):
    """x[B,N,C] feature rows (C <= 256; a column slice of a wider row-major buffer is fine) -> idx[B,N,k] int32, nearest first,
    the point itself included, ranked by the fp32 chain d = fma(t, t, d), t = x[j,c] - x[i,c], c ascending, the lower index
    first among equal d (houv_knn_feat).  want_dist: (idx, dist2[B,N,k])."""
    _lib.require_gpu_any(x)
    B, N, C, ldx = _rows(x, "knn_feat: x")
    idx = torch.empty((B, N, int(k)), dtype=_I32, device=x.device)
    d2 = torch.empty((B, N, int(k)), dtype=_F32, device=x.device) if want_dist else None
    _lib.call("houv_knn_feat", x, x, B, N, C, ldx, k, idx, d2)
    return (idx, d2) if want_dist else idx


def _out_rows(who, name, out, shape, device):
    """(out, its row stride): the caller's `out`, or a dense fp32 one allocated here, of exactly `shape` and laid out as _rows
    asks.  The caller has taken a given `out` through require_gpu_any."""
    if out is None:
        out = torch.empty(shape, dtype=_F32, device=device)
    if tuple(out.shape) != shape:
        raise _lib.HouvHipError(f"{who}: {name} must be [{','.join(map(str, shape))}], got {tuple(out.shape)}")
    return out, _rows(out, f"{who}: {name}")[3]


def dense_conv(x, idx, W0, b0, W1, b1, W2, b2, relu_out=False, out=None):
    """Dense_conv.forward (completion/models/ecg.py:58-65; growth rate 24, dense_n 3) in one kernel (houv_dense_conv): x[B,N,C]
    rows (C = 24 or 48), idx[B,N,k] int32 neighbour lists, W0[24,2C], W1[24,24+C], W2[24,48+C], biases [24] ->
    out[B,N,C+72] = max over the neighbours of cat(y0, x_i, s1, s2), relu applied when relu_out.  `out` may be a [B,N,C+72]
    column slice of a wider row-major buffer (the caller's cat(dense, x)); its other columns are left alone."""
    B, N, C, ldx = _dense_conv_args("dense_conv", x, idx, W0, b0, W1, b1, W2, b2, out)
    out, ldo = _out_rows("dense_conv", "out", out, (B, N, C + 3 * DENSE_CONV_GROWTH), x.device)
    _lib.call("houv_dense_conv", x, x, ldx, idx, B, N, C, idx.shape[2], W0, b0, W1, b1, W2, b2, bool(relu_out), out, ldo)
    return out


def _dense_conv_args(who, x, idx, W0, b0, W1, b1, W2, b2, out=None):
    """(B, N, C, x's row stride) of dense_conv's operands; `out`: an output to take through the first check with them."""
    _lib.require_gpu_any(x, W0, b0, W1, b1, W2, b2, out)
    _lib.require_gpu(idx, W0, b0, W1, b1, W2, b2); _want(idx, _I32, f"{who}: idx")
    B, N, C, ldx = _rows(x, f"{who}: x")
    G = DENSE_CONV_GROWTH
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (B, N):
        raise _lib.HouvHipError(f"{who}: expected idx[{B},{N},k], got {tuple(idx.shape)}")
    if tuple(W0.shape) != (G, 2 * C) or tuple(W1.shape) != (G, G + C) or tuple(W2.shape) != (G, 2 * G + C) \
            or b0.numel() != G or b1.numel() != G or b2.numel() != G:
        raise _lib.HouvHipError(f"{who}: expected W0[24,{2 * C}], W1[24,{G + C}], W2[24,{2 * G + C}] and biases [24], got "
                                f"{tuple(W0.shape)}, {tuple(W1.shape)}, {tuple(W2.shape)}")
    return B, N, C, ldx


def dense_conv_arg(x, idx, W0, b0, W1, b1, W2, b2, relu_out=False, out=None):
    """dense_conv that also says where each maximum sits (houv_dense_conv_arg): the same arguments ->
    (out[B,N,C+72], arg[B,N,72] int8).  out carries dense_conv's bits; arg[b,i,q] is the lowest edge slot whose candidate attains
    the maximum of pooled column q (y0, s1, s2: 24 each; torch.max's rule on the CPU), -1 for a column that is NaN for every
    neighbour."""
    B, N, C, ldx = _dense_conv_args("dense_conv_arg", x, idx, W0, b0, W1, b1, W2, b2)
    G = DENSE_CONV_GROWTH
    _lib.require_gpu_any(x, out)
    out, ldo = _out_rows("dense_conv_arg", "out", out, (B, N, C + 3 * G), x.device)
    arg = torch.empty((B, N, 3 * G), dtype=torch.int8, device=x.device)
    _lib.call("houv_dense_conv_arg", x, x, ldx, idx, B, N, C, idx.shape[2], W0, b0, W1, b1, W2, b2, bool(relu_out), out, ldo, arg)
    return out, arg


def dense_conv_backward(x, idx, W0, b0, W1, b1, W2, b2, arg, gout, out=None, relu_out=False, gx=None):
    """The backward pass of dense_conv (houv_dense_conv_backward): dense_conv's arguments, arg[B,N,72]
    int8 from dense_conv_arg, gout[B,N,C+72] (the gradient of out; rows of any stride) and, when relu_out, the forward's out ->
    dict(gx[B,N,C], gW0[24,2C], gb0[24], gW1[24,24+C], gb1[24], gW2[24,48+C], gb2[24]).  `gx` may be a [B,N,C] column slice of a
    wider row-major buffer; its other columns are left alone.  Deterministic: no float atomics, fixed sum orders."""
    B, N, C, ldx = _dense_conv_args("dense_conv_backward", x, idx, W0, b0, W1, b1, W2, b2)
    G = DENSE_CONV_GROWTH
    _lib.require_gpu(arg)
    _lib.require_gpu_any(x, gout, out, gx)
    if arg.dtype != torch.int8 or tuple(arg.shape) != (B, N, 3 * G):
        raise _lib.HouvHipError(f"dense_conv_backward: arg must be int8 [{B},{N},{3 * G}], got {arg.dtype} {tuple(arg.shape)}")
    if tuple(gout.shape) != (B, N, C + 3 * G):
        raise _lib.HouvHipError(f"dense_conv_backward: gout must be [{B},{N},{C + 3 * G}], got {tuple(gout.shape)}")
    ldg = _rows(gout, "dense_conv_backward: gout")[3]
    ldo = 0
    if relu_out:
        if out is None or tuple(out.shape) != (B, N, C + 3 * G):
            raise _lib.HouvHipError(f"dense_conv_backward: relu_out needs the forward's out [{B},{N},{C + 3 * G}]")
        ldo = _rows(out, "dense_conv_backward: out")[3]
    else:
        out = None
    dev = x.device
    gx, ldgx = _out_rows("dense_conv_backward", "gx", gx, (B, N, C), dev)
    new = lambda *shape: torch.empty(shape, dtype=_F32, device=dev)
    res = dict(gx=gx, gW0=new(G, 2 * C), gb0=new(G), gW1=new(G, G + C), gb1=new(G), gW2=new(G, 2 * G + C), gb2=new(G))
    k = idx.shape[2]
    ws, nbytes = _lib.workspace("houv_dense_conv_backward_workspace_bytes", dev, B, N, C, k)
    _lib.call("houv_dense_conv_backward", x, x, ldx, idx, B, N, C, k, W0, b0, W1, b1, W2, b2, bool(relu_out), arg, out, ldo, gout, ldg,
              gx, ldgx, *(res[n] for n in ("gW0", "gb0", "gW1", "gb1", "gW2", "gb2")), ws, nbytes)
    return res


# ---------------------------------------------------------------------------------------------------
# VRCNet completion network (houv_sa_attn)
# ---------------------------------------------------------------------------------------------------
SA_ATTN_BLOCK = 128                        # HOUV_SA_ATTN_BLOCK: points per workgroup


def sa_attn(P, x, idx, Ww1, Ww2, bw2, Wout, bout, relu_out=False, out=None):
    """SA_module.forward (completion/models/vrcnet.py:49-67) after its input projections, in one kernel (houv_sa_attn).  With
    rel = C/16, mid = C/4, m = mid/8: P[B,N,2 rel + mid] = relu(x) . [W1; W2; W3]^T + bias (columns x1 | x2 | x3, one `gemm`),
    x[B,N,C] the pre-activation identity, idx[B,N,k] int32, Ww1[m, rel (k+1)], Ww2[k m, m], bw2[k m], Wout[C, mid], bout[C] ->
    out[B,N,C] = Wout relu(sum_j w_j x3_j) + bout + x, relu applied when relu_out.  C = 64, 128, 256 or 512, k <= 32.  P, x and
    `out` may be column slices of wider row-major buffers (P's row stride a multiple of 4, its address of 16 bytes); `out` may be
    x itself."""
    _lib.require_gpu_any(P, x, Ww1, Ww2, bw2, Wout, bout, out)
    _lib.require_gpu(idx, Ww1, Ww2, bw2, Wout, bout); _want(idx, _I32, "sa_attn: idx")
    B, N, C, ldx = _rows(x, "sa_attn: x")
    rel, mid, m = C // 16, C // 4, C // 32
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (B, N):
        raise _lib.HouvHipError(f"sa_attn: expected idx[{B},{N},k], got {tuple(idx.shape)}")
    k = idx.shape[2]
    if tuple(P.shape) != (B, N, 2 * rel + mid):
        raise _lib.HouvHipError(f"sa_attn: expected P[{B},{N},{2 * rel + mid}], got {tuple(P.shape)}")
    ldp = _rows(P, "sa_attn: P")[3]
    if tuple(Ww1.shape) != (m, rel * (k + 1)) or tuple(Ww2.shape) != (k * m, m) or bw2.numel() != k * m \
            or tuple(Wout.shape) != (C, mid) or bout.numel() != C:
        raise _lib.HouvHipError(f"sa_attn: expected Ww1[{m},{rel * (k + 1)}], Ww2[{k * m},{m}], bw2[{k * m}], Wout[{C},{mid}], "
                                f"bout[{C}], got {tuple(Ww1.shape)}, {tuple(Ww2.shape)}, {tuple(bw2.shape)}, {tuple(Wout.shape)}, "
                                f"{tuple(bout.shape)}")
    out, ldo = _out_rows("sa_attn", "out", out, (B, N, C), x.device)
    _lib.call("houv_sa_attn", x, P, ldp, x, ldx, idx, B, N, C, k, Ww1, Ww2, bw2, Wout, bout, bool(relu_out), out, ldo)
    return out


def sa_attn_backward(P, idx, Ww1, Ww2, bw2, G, gP=None):
    """The backward pass of sa_attn up to conv_out (houv_sa_attn_backward): sa_attn's P, idx, Ww1, Ww2, bw2
    and G[B,N,mid], the gradient of relu(o) (the caller's gy . Wout; rows of any stride) -> dict(gP[B,N,2 rel + mid], ro[B,N,mid] =
    relu(o) recomputed by the forward's chains, gWw1[m, rel (k+1)], gWw2[k m, m], gbw2[k m]).  `gP` may be a column slice of a wider
    row-major buffer; its other columns are left alone.  conv_out's own gradients (gWout = gy^T . ro, gbout = sum gy) and the
    residual's are the caller's.  Deterministic: no float atomics, fixed sum orders.  The workspace is allocated here."""
    _lib.require_gpu_any(P, Ww1, Ww2, bw2, G, gP)
    _lib.require_gpu(idx, Ww1, Ww2, bw2); _want(idx, _I32, "sa_attn_backward: idx")
    B, N, wp, ldp = _rows(P, "sa_attn_backward: P")
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (B, N):
        raise _lib.HouvHipError(f"sa_attn_backward: expected idx[{B},{N},k], got {tuple(idx.shape)}")
    k = idx.shape[2]
    if wp % 6 != 0 or wp * 8 // 3 not in (64, 128, 256, 512):
        raise _lib.HouvHipError(f"sa_attn_backward: P has {wp} columns; 2 rel + mid = 24, 48, 96 or 192 (C = 64 .. 512) are served")
    C = wp * 8 // 3
    rel, mid, m = C // 16, C // 4, C // 32
    if tuple(Ww1.shape) != (m, rel * (k + 1)) or tuple(Ww2.shape) != (k * m, m) or bw2.numel() != k * m:
        raise _lib.HouvHipError(f"sa_attn_backward: expected Ww1[{m},{rel * (k + 1)}], Ww2[{k * m},{m}], bw2[{k * m}], got "
                                f"{tuple(Ww1.shape)}, {tuple(Ww2.shape)}, {tuple(bw2.shape)}")
    if tuple(G.shape) != (B, N, mid):
        raise _lib.HouvHipError(f"sa_attn_backward: G must be [{B},{N},{mid}], got {tuple(G.shape)}")
    ldg = _rows(G, "sa_attn_backward: G")[3]
    dev = P.device
    new = lambda *shape: torch.empty(shape, dtype=_F32, device=dev)
    gP, ldgp = _out_rows("sa_attn_backward", "gP", gP, (B, N, wp), dev)
    res = dict(gP=gP, ro=new(B, N, mid), gWw1=new(m, rel * (k + 1)), gWw2=new(k * m, m), gbw2=new(k * m))
    ws, nbytes = _lib.workspace("houv_sa_attn_backward_workspace_bytes", dev, B, N, C, k)
    _lib.call("houv_sa_attn_backward", P, P, ldp, idx, B, N, C, k, Ww1, Ww2, bw2, G, ldg, gP, ldgp, res["ro"], mid, res["gWw1"],
              res["gWw2"], res["gbw2"], ws, nbytes)
    return res


def _edge_pool_lists(who, p_idx, pn_idx, B):
    _lib.require_gpu(p_idx, pn_idx); _want(p_idx, _I32, f"{who}: p_idx"); _want(pn_idx, _I32, f"{who}: pn_idx")
    if p_idx.dim() != 2 or p_idx.shape[0] != B or pn_idx.dim() != 3 or tuple(pn_idx.shape[:2]) != tuple(p_idx.shape):
        raise _lib.HouvHipError(f"{who}: expected p_idx[{B},S] and pn_idx[{B},S,pk], got {tuple(p_idx.shape)} and {tuple(pn_idx.shape)}")
    return p_idx.shape[1], pn_idx.shape[2]


def edge_pool(feat, p_idx, pn_idx, out=None, want_arg=False):
    """edge_preserve_sampling's feature half in one kernel (houv_edge_pool): feat[B,N,C] rows, p_idx[B,S]
    and pn_idx[B,S,pk] int32 -> out[B,S,2C] = cat(feat[p_idx], max over the pk listed rows).  feat and `out` may be column slices
    of wider row-major buffers; out's other columns are left alone.  want_arg: (out, arg[B,S,C] int8), the lowest slot that
    attains each maximum (-1 for a column that is NaN in every listed row)."""
    _lib.require_gpu_any(feat, out)
    B, N, C, ldx = _rows(feat, "edge_pool: feat")
    S, pk = _edge_pool_lists("edge_pool", p_idx, pn_idx, B)
    out, ldo = _out_rows("edge_pool", "out", out, (B, S, 2 * C), feat.device)
    arg = torch.empty((B, S, C), dtype=torch.int8, device=feat.device) if want_arg else None
    _lib.call("houv_edge_pool", feat, feat, ldx, p_idx, pn_idx, B, N, S, C, pk, out, ldo, arg)
    return (out, arg) if want_arg else out


def edge_pool_backward(g, p_idx, pn_idx, arg, N):
    """The backward pass of edge_pool (houv_edge_pool_backward): g[B,S,2C] (the gradient of out; rows of
    any stride), edge_pool's lists and arg, and the number of rows N of feat -> gfeat[B,N,C], every element written: the sum of
    what landed on a row in ascending (s, slot), the centre first.  Deterministic: no float atomics.  The workspace (int32 only)
    is allocated here."""
    _lib.require_gpu_any(g)
    B, S, C2, ldg = _rows(g, "edge_pool_backward: g")
    S_, pk = _edge_pool_lists("edge_pool_backward", p_idx, pn_idx, B)
    C = C2 // 2
    _lib.require_gpu(arg)
    if S_ != S or C2 != 2 * C or arg.dtype != torch.int8 or tuple(arg.shape) != (B, S, C):
        raise _lib.HouvHipError(f"edge_pool_backward: expected g[{B},{S_},2C] and int8 arg[{B},{S_},C], got {tuple(g.shape)} and "
                                f"{arg.dtype} {tuple(arg.shape)}")
    dev = g.device
    gfeat = torch.empty((B, int(N), C), dtype=_F32, device=dev)
    ws, nbytes = _lib.workspace("houv_edge_pool_backward_workspace_bytes", dev, B, N, S, pk)
    _lib.call("houv_edge_pool_backward", g, g, ldg, p_idx, pn_idx, arg, B, N, S, C, pk, gfeat, C, ws, nbytes)
    return gfeat


def cd_loss_backward(output, gt, dist1, dist2, idx1, idx2, g_p, g_t, gout=None, workspace=None):
    """The gradient of calc_cd(output, gt) with respect to output (houv_cd_loss_backward): output[B,M,3],
    gt[B,N,3], what chamfer_forward(gt, output) gave (dist1[B,N], dist2[B,M], int32 idx1[B,N] rows of output, idx2[B,M] rows of
    gt) and the upstream gradients g_p[B], g_t[B] of cd_p and cd_t -> gout[B,M,3], every element written: the own term, then the
    terms of the ground-truth points that chose the row, in ascending order.  Deterministic: no float atomics.  `gout` and the
    int32 `workspace` (houv_cd_loss_backward_workspace_bytes) are allocated here unless given."""
    _lib.require_gpu(output, gt, dist1, dist2, idx1, idx2, g_p, g_t, gout, workspace)
    for t, d, n in ((output, _F32, "output"), (gt, _F32, "gt"), (dist1, _F32, "dist1"), (dist2, _F32, "dist2"), (idx1, _I32, "idx1"),
                    (idx2, _I32, "idx2"), (g_p, _F32, "g_p"), (g_t, _F32, "g_t")):
        _want(t, d, f"cd_loss_backward: {n}")
    if output.dim() != 3 or gt.dim() != 3 or output.shape[2] != 3 or gt.shape[2] != 3 or gt.shape[0] != output.shape[0]:
        raise _lib.HouvHipError(f"cd_loss_backward: expected output[B,M,3] and gt[B,N,3], got {tuple(output.shape)} and {tuple(gt.shape)}")
    B, M, _ = output.shape
    N = gt.shape[1]
    if (tuple(dist1.shape) != (B, N) or tuple(idx1.shape) != (B, N) or tuple(dist2.shape) != (B, M) or tuple(idx2.shape) != (B, M)
            or g_p.numel() != B or g_t.numel() != B):
        raise _lib.HouvHipError(f"cd_loss_backward: expected dist1, idx1 [{B},{N}], dist2, idx2 [{B},{M}] and g_p, g_t [{B}], got "
                                f"{tuple(dist1.shape)}, {tuple(idx1.shape)}, {tuple(dist2.shape)}, {tuple(idx2.shape)}, "
                                f"{tuple(g_p.shape)}, {tuple(g_t.shape)}")
    dev = output.device
    if gout is None:
        gout = torch.empty((B, M, 3), dtype=_F32, device=dev)
    _want(gout, _F32, "cd_loss_backward: gout")
    if tuple(gout.shape) != (B, M, 3):
        raise _lib.HouvHipError(f"cd_loss_backward: gout must be [{B},{M},3], got {tuple(gout.shape)}")
    if workspace is None:
        ws = _lib.workspace("houv_cd_loss_backward_workspace_bytes", dev, B, N, M)[0]
        workspace = ws[:ws.numel() // 4 * 4].view(_I32)     # whole int32 words, whatever size the query names
    _want(workspace, _I32, "cd_loss_backward: workspace")
    _lib.call("houv_cd_loss_backward", output, output, gt, dist1, dist2, idx1, idx2, g_p, g_t, B, N, M, gout, workspace,
              4 * workspace.numel())
    return gout


def _ef_expand_args(who, proj, idx, W2a, W3, r):
    """(B, N, O, k, ldp, ldw) of ef_expand's operands: proj[B,N,2O+2Or] rows (one row stride), idx[B,N,k] int32, W2a[O r, O] rows
    of any stride (a column slice of conv2's weight), W3[O,O] dense."""
    _lib.require_gpu_any(proj, W2a, W3)
    B, N, W, ldp = _rows(proj, f"{who}: proj")
    r = int(r)
    O = W3.shape[0]
    if W3.dim() != 2 or W3.shape[1] != O or not W3.is_contiguous() or r < 1 or W != 2 * O + 2 * O * r:
        raise _lib.HouvHipError(f"{who}: expected dense W3[O,O] and proj[B,N,2O+2Or], got W3 {tuple(W3.shape)}, proj {tuple(proj.shape)}, r={r}")
    if W2a.dim() != 2 or tuple(W2a.shape) != (O * r, O) or W2a.stride(1) != 1 or W2a.stride(0) < O:
        raise _lib.HouvHipError(f"{who}: expected W2a[{O * r},{O}] rows with unit column stride, got {tuple(W2a.shape)} strides {tuple(W2a.stride())}")
    _lib.require_gpu(idx); _want(idx, _I32, f"{who}: idx")
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (B, N):
        raise _lib.HouvHipError(f"{who}: expected idx[{B},{N},k], got {tuple(idx.shape)}")
    return B, N, O, idx.shape[2], ldp, W2a.stride(0)


def ef_expand(proj, idx, W2a, W3, b3, r, out=None, want_arg=False):
    """EF_expansion past its per-point projections in one kernel (houv_ef_expand): proj[B,N,2O+2Or] =
    [U | V | P | Q] rows, idx[B,N,k] int32, W2a[O r, O] (the first O columns of conv2's weight; a column slice is fine), W3[O,O],
    b3[O] -> out[B, N r, O], the maximum over the k listed neighbours of conv3(relu(conv2(...))).  proj and `out` may be column
    slices of wider row-major buffers.  want_arg: (out, arg[B, N r, O] int8), the lowest slot that attains each maximum (-1 for
    a column that is NaN at every slot)."""
    B, N, O, k, ldp, ldw = _ef_expand_args("ef_expand", proj, idx, W2a, W3, r)
    r = int(r)
    _lib.require_gpu(b3); _want(b3, _F32, "ef_expand: b3")
    if tuple(b3.shape) != (O,):
        raise _lib.HouvHipError(f"ef_expand: b3 must be [{O}], got {tuple(b3.shape)}")
    _lib.require_gpu_any(out)
    out, ldo = _out_rows("ef_expand", "out", out, (B, N * r, O), proj.device)
    arg = torch.empty((B, N * r, O), dtype=torch.int8, device=proj.device) if want_arg else None
    _lib.call("houv_ef_expand", proj, proj, ldp, idx, B, N, O, k, r, W2a, ldw, W3, b3, out, ldo, arg)
    return (out, arg) if want_arg else out


def ef_expand_backward(proj, idx, arg, W2a, W3, g, r, gproj=None):
    """The backward pass of ef_expand (houv_ef_expand_backward): ef_expand's operands, its arg and
    g[B, N r, O] (rows of any stride) -> {"gproj": [B,N,2O+2Or] (every element written; `gproj`, when given, may be a column
    slice), "gW2a": [O r, O], "gW3": [O,O], "gb3": [O]}.  Deterministic: no float atomics.  The workspace is allocated here."""
    B, N, O, k, ldp, ldw = _ef_expand_args("ef_expand_backward", proj, idx, W2a, W3, r)
    r = int(r)
    _lib.require_gpu_any(g); _lib.require_gpu(arg)
    if tuple(g.shape) != (B, N * r, O) or arg.dtype != torch.int8 or tuple(arg.shape) != (B, N * r, O):
        raise _lib.HouvHipError(f"ef_expand_backward: expected g[{B},{N * r},{O}] and int8 arg of that shape, got {tuple(g.shape)} and "
                                f"{arg.dtype} {tuple(arg.shape)}")
    ldg = _rows(g, "ef_expand_backward: g")[3]
    dev = proj.device
    W = 2 * O + 2 * O * r
    _lib.require_gpu_any(gproj)
    gproj, ldgp = _out_rows("ef_expand_backward", "gproj", gproj, (B, N, W), dev)
    res = {"gproj": gproj, "gW2a": torch.empty((O * r, O), dtype=_F32, device=dev), "gW3": torch.empty((O, O), dtype=_F32, device=dev),
           "gb3": torch.empty((O,), dtype=_F32, device=dev)}
    ws, nbytes = _lib.workspace("houv_ef_expand_backward_workspace_bytes", dev, B, N, O, k, r)
    _lib.call("houv_ef_expand_backward", proj, proj, ldp, idx, arg, B, N, O, k, r, W2a, ldw, W3, g, ldg, gproj, ldgp, res["gW2a"],
              res["gW3"], res["gb3"], ws, nbytes)
    return res


# ---------------------------------------------------------------------------------------------------
# torch.ops.houv.* registration (PyTorch-ROCm custom ops; the schema marks the in-place outputs)
# ---------------------------------------------------------------------------------------------------
_registered = False


def register_torch_ops():
    global _registered
    if _registered:
        return
    lib = torch.library.Library("houv", "DEF")
    lib.define("chamfer_forward(Tensor xyz1, Tensor xyz2, Tensor(a!) dist1, Tensor(b!) dist2, Tensor(c!) idx1, "
               "Tensor(d!) idx2) -> int")
    lib.define("chamfer_backward(Tensor xyz1, Tensor xyz2, Tensor(a!) gradxyz1, Tensor(b!) gradxyz2, Tensor graddist1, "
               "Tensor graddist2, Tensor idx1, Tensor idx2) -> int")
    lib.define("kabsch(Tensor src, Tensor corr, Tensor? weights) -> (Tensor, Tensor)")
    # the fused loop: the C ABI's argument list, mutable tensors marked; returns 1 like the C call
    solve_args = ("Tensor src, Tensor tgt, Tensor(a!) state, int K, int steps_done, int n_iters, int angle_base, "
                  "int trans_mode, bool use_views, bool f64_params, int k_full, int k_view, float lr, float beta1, "
                  "float beta2, float eps, float loss_scale, Tensor(b!) out_score, Tensor(c!) out_loss, Tensor(d!) out_R, "
                  "Tensor(e!) out_T, Tensor(f!)? out_grad, Tensor(g!)? out_cd")
    lib.define(f"solve_iterate({solve_args}) -> int")
    lib.define(f"solve_iterate_pruned({solve_args}, Tensor(h!) nn_ws, int ws_valid) -> int")
    lib.define(f"solve_iterate_large({solve_args}) -> int")
    lib.define("icp_refine(Tensor src, Tensor tgt, Tensor? init, float max_correspondence_distance, int max_iteration, "
               "float relative_fitness, float relative_rmse) -> (Tensor, Tensor, Tensor, Tensor)")
    lib.define("pose_forward(Tensor params, int angle_base, int trans_mode, Tensor? src) -> (Tensor, Tensor, Tensor)")
    lib.define("kd_sort(Tensor cloud, int leaf, str rule) -> (Tensor, Tensor)")
    lib.define("emd_forward(Tensor xyz1, Tensor xyz2, float eps, int iters) -> (Tensor, Tensor, Tensor)")
    lib.define("emd_backward(Tensor xyz1, Tensor xyz2, Tensor graddist, Tensor assignment) -> Tensor")
    lib.define("rri_features(Tensor xyz, Tensor idx, int k, int skip) -> Tensor")
    lib.define("gmm_params(Tensor gamma, Tensor pts) -> (Tensor, Tensor, Tensor)")
    lib.define("gmm_register(Tensor pi_s, Tensor mu_s, Tensor mu_t, Tensor sigma_t) -> Tensor")
    lib.define("gmm_params_backward(Tensor gamma, Tensor pts, Tensor pi, Tensor mu, Tensor sigma, Tensor g_pi, Tensor g_mu, "
               "Tensor g_sigma) -> Tensor")
    lib.define("gmm_register_backward(Tensor pi_s, Tensor mu_s, Tensor mu_t, Tensor sigma_t, Tensor g_T) -> "
               "(Tensor, Tensor, Tensor, Tensor)")
    lib.define("bn_rows_stats(Tensor z) -> (Tensor, Tensor)")
    lib.define("bn_relu_rows(Tensor z, Tensor mean, Tensor var, Tensor weight, Tensor bias, float eps, bool relu, int n_group) -> "
               "(Tensor, Tensor, Tensor)")
    lib.define("bn_relu_rows_backward(Tensor gy, Tensor z, Tensor mean, Tensor var, Tensor weight, Tensor bias, float eps, "
               "bool relu) -> (Tensor, Tensor, Tensor)")
    lib.define("idam_simmat(Tensor src, Tensor tgt, Tensor es, Tensor et, Tensor W1, Tensor s1, Tensor t1, Tensor W2, Tensor b2, "
               "Tensor W3, Tensor s3, Tensor t3, Tensor w4, Tensor b4) -> (Tensor, Tensor, Tensor, Tensor)")
    lib.define("edge_diff(Tensor x, Tensor idx, int k, int ldo) -> Tensor")
    lib.define("mlp2_max(Tensor x, Tensor W1, Tensor shift1, Tensor W2, Tensor b2) -> (Tensor, Tensor)")
    lib.define("mlp2_max_arg(Tensor x, Tensor W1, Tensor shift1, Tensor W2, Tensor b2) -> (Tensor, Tensor, Tensor)")
    lib.define("mlp2_max_backward(Tensor x, Tensor W1, Tensor shift1, Tensor W2, Tensor arg, Tensor gpooled, Tensor? rows, "
               "Tensor? nrows, Tensor? gy_rows) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    lib.define("pcn_fold(Tensor coarse, Tensor cvec, Tensor grid, Tensor Wgp, Tensor W2, Tensor b2, Tensor W3, Tensor b3) -> Tensor")
    lib.define("pcn_fold_backward(Tensor coarse, Tensor cvec, Tensor grid, Tensor Wgp, Tensor W2, Tensor b2, Tensor W3, Tensor b3, "
               "Tensor gfine) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    lib.define("knn_feat(Tensor x, int k) -> (Tensor, Tensor)")
    lib.define("dense_conv(Tensor x, Tensor idx, Tensor W0, Tensor b0, Tensor W1, Tensor b1, Tensor W2, Tensor b2, "
               "bool relu_out) -> Tensor")
    lib.define("sa_attn(Tensor P, Tensor x, Tensor idx, Tensor Ww1, Tensor Ww2, Tensor bw2, Tensor Wout, Tensor bout, "
               "bool relu_out) -> Tensor")
    lib.impl("chamfer_forward", chamfer_forward, "CUDA")
    lib.impl("chamfer_backward", chamfer_backward, "CUDA")
    lib.impl("kabsch", kabsch, "CUDA")
    lib.impl("solve_iterate", solve_iterate_out, "CUDA")
    lib.impl("solve_iterate_pruned", solve_iterate_out, "CUDA")
    lib.impl("solve_iterate_large", solve_iterate_large_out, "CUDA")

    def _icp(src, tgt, init, max_correspondence_distance, max_iteration, relative_fitness, relative_rmse):
        r = icp_refine(src, tgt, init, max_correspondence_distance, max_iteration, relative_fitness, relative_rmse)
        return r["T"], r["fitness"], r["inlier_rmse"], r["iterations"]

    def _pose(params, angle_base, trans_mode, src):
        r = pose_forward(params, angle_base, trans_mode, src)
        return (r[0], r[1], r[2] if src is not None else params.new_empty((0,)))
    lib.impl("icp_refine", _icp, "CUDA")
    lib.impl("pose_forward", _pose, "CUDA")

    def _kd_sort(cloud, leaf, rule):
        return kd_sort(cloud, leaf, rule, return_order=True)
    lib.impl("kd_sort", _kd_sort, "CUDA")
    lib.impl("emd_forward", emd_forward, "CUDA")
    lib.impl("emd_backward", emd_backward, "CUDA")
    lib.impl("rri_features", rri_features, "CUDA")
    lib.impl("gmm_params", gmm_params, "CUDA")
    lib.impl("gmm_register", gmm_register, "CUDA")
    lib.impl("gmm_params_backward", gmm_params_backward, "CUDA")
    lib.impl("gmm_register_backward", gmm_register_backward, "CUDA")
    lib.impl("bn_rows_stats", bn_rows_stats, "CUDA")

    def _bn_relu_rows(z, mean, var, weight, bias, eps, relu, n_group):
        r = bn_relu_rows(z, mean, var, weight, bias, eps, relu, n_group)
        return r if n_group else (r, z.new_empty((0, z.shape[1])), z.new_empty((0, z.shape[1]), dtype=_I32))
    lib.impl("bn_relu_rows", _bn_relu_rows, "CUDA")
    lib.impl("bn_relu_rows_backward", bn_relu_rows_backward, "CUDA")

    def _simmat(*a):
        return idam_simmat(*a, want_scores=True)
    lib.impl("idam_simmat", _simmat, "CUDA")
    lib.impl("edge_diff", edge_diff, "CUDA")

    def _mlp2_max(*a):
        return mlp2_max(*a, want_y=True)
    lib.impl("mlp2_max", _mlp2_max, "CUDA")

    def _mlp2_max_arg(*a):
        return mlp2_max_arg(*a, want_y=True)
    lib.impl("mlp2_max_arg", _mlp2_max_arg, "CUDA")

    def _mlp2_max_backward(*a):
        r = mlp2_max_backward(*a, want_gx=True)
        return tuple(r[k] for k in ("gW1", "gshift1", "gW2", "gb2", "act_rows", "nact", "gx_rows"))
    lib.impl("mlp2_max_backward", _mlp2_max_backward, "CUDA")
    lib.impl("pcn_fold", pcn_fold, "CUDA")

    def _pcn_fold_backward(*a):
        r = pcn_fold_backward(*a)
        return tuple(r[k] for k in ("gcoarse", "gcvec", "gWgp", "gW2", "gb2", "gW3", "gb3"))
    lib.impl("pcn_fold_backward", _pcn_fold_backward, "CUDA")

    def _knn_feat(x, k):
        return knn_feat(x, k, want_dist=True)
    lib.impl("knn_feat", _knn_feat, "CUDA")
    lib.impl("dense_conv", dense_conv, "CUDA")
    lib.impl("sa_attn", sa_attn, "CUDA")
    register_torch_ops._lib = lib      # keep alive
    _registered = True


# ---------------------------------------------------------------------------------------------------
# DCP feature-head building blocks (houv_knn, houv_edgeconv1, houv_max_over_k, houv_gemm_f32, houv_layernorm,
# houv_softmax_rows, houv_softmax_corr): thin wrappers; shapes are checked, buffers are allocated with torch.
# ---------------------------------------------------------------------------------------------------
def knn(xyz, k):
    """xyz[B,N,3] -> idx[B,N,k] int32, nearest first, self included (dcp.py:35-42)."""
    _lib.require_gpu(xyz); _want(xyz, _F32, "xyz")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise _lib.HouvHipError("knn: expected xyz[B,N,3]")
    B, N, _ = xyz.shape
    idx = torch.empty((B, N, k), dtype=_I32, device=xyz.device)
    _lib.call("houv_knn", xyz, xyz, B, N, k, idx)
    return idx


def edgeconv1(xyz, idx, W, scale, shift):
    """-> act[B*N*k, 64] = relu(scale * conv1(cat(neighbour, centre)) + shift)."""
    _lib.require_gpu(xyz, idx, W, scale, shift)
    for t, d, n in ((xyz, _F32, "xyz"), (idx, _I32, "idx"), (W, _F32, "W"), (scale, _F32, "scale"), (shift, _F32, "shift")):
        _want(t, d, n)
    if idx.dim() != 3 or xyz.dim() != 3 or xyz.shape[2] != 3 or idx.shape[:2] != xyz.shape[:2]:
        raise _lib.HouvHipError("edgeconv1: expected xyz[B,N,3], idx[B,N,k]")
    if tuple(W.shape) != (64, 6) or scale.numel() != 64 or shift.numel() != 64:
        raise _lib.HouvHipError("edgeconv1: expected W[64,6], scale[64], shift[64]")
    B, N, k = idx.shape
    out = torch.empty((B * N * k, 64), dtype=_F32, device=xyz.device)
    _lib.call("houv_edgeconv1", xyz, xyz, idx, B, N, k, W, scale, shift, out)
    return out


def _aligned16(*tensors):
    return all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def max_over_k(act, k, out, col0):
    """out[:, col0:col0+C] = max over groups of k consecutive rows of act[npts*k, C].  The kernel moves 16 bytes at a time:
    act and the written view out[:, col0:] must start on 16-byte boundaries."""
    _lib.require_gpu(act); _lib.require_gpu_any(out)
    _want(act, _F32, "act"); _want(out, _F32, "out")
    if act.dim() != 2 or out.dim() != 2 or k <= 0 or col0 < 0:
        raise _lib.HouvHipError("max_over_k: expected act[npts*k,C], out[npts, >= col0+C]")
    C = act.shape[1]
    if act.shape[0] % k or C % 4 or out.stride(0) % 4 or out.stride(1) != 1 \
            or out.shape[0] != act.shape[0] // k or col0 + C > out.shape[1]:
        raise _lib.HouvHipError("max_over_k: expected act[npts*k,C], out[npts, >= col0+C] (C and the row stride multiples of 4)")
    npts = act.shape[0] // k
    view = out[:, col0:col0 + C]
    if not _aligned16(act, view):
        raise _lib.HouvHipError("max_over_k: act and out[:, col0:] must start on 16-byte boundaries (col0 a multiple of 4 "
                                "in a 16-byte aligned buffer)")
    _lib.call("houv_max_over_k", act, act, npts, k, C, view, out.stride(0))


# bench.py sets this to a list to collect (start_event, end_event, flops) per houv_gemm_f32 launch
GEMM_LOG = None


def gemm(A, B, C=None, *, trans_b=True, alpha=1.0, scale=None, shift=None, residual=None, relu=False):
    """2-D or batched (3-/4-D leading dims = (outer[, inner])) fp32 GEMM on the MFMA kernel.
    A[..., M, K]; B[..., N, K] if trans_b else B[..., K, N]; returns C[..., M, N].  Inner-most dims may be strided
    row-major views (row stride = lda), which is how per-head attention operands are addressed without copies."""
    _lib.require_gpu_any(A, B, C, scale, shift, residual)
    lead = A.shape[:-2]
    M, K = A.shape[-2:]
    N = B.shape[-2] if trans_b else B.shape[-1]
    if C is None:
        C = torch.empty(lead + (M, N), dtype=_F32, device=A.device)
    outer = lead[0] if len(lead) >= 1 else 1
    inner = lead[1] if len(lead) == 2 else 1

    def strides(t):
        ld = t.stride(-2)
        assert t.stride(-1) == 1, "innermost dimension must be contiguous"
        so = t.stride(0) if len(lead) >= 1 else 0
        si = t.stride(1) if len(lead) == 2 else 0
        return ld, so, si
    lda, sAo, sAi = strides(A)
    ldb, sBo, sBi = strides(B)
    ldc, sCo, sCi = strides(C)
    ldr, sRo, sRi = strides(residual) if residual is not None else (0, 0, 0)
    if GEMM_LOG is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(A.device))
    _lib.call("houv_gemm_f32", A, A, B, C, M, N, K, lda, ldb, ldc, bool(trans_b), outer, inner, sAo, sAi, sBo, sBi, sCo, sCi, alpha,
              scale, shift, residual, ldr, sRo, sRi, bool(relu))
    if GEMM_LOG is not None:
        ev1.record(torch.cuda.current_stream(A.device))
        GEMM_LOG.append((ev0, ev1, 2.0 * outer * inner * M * N * K))
    return C


# set to False to route models.dcp's attention through gemm -> softmax_rows -> gemm (the [P,H,Nq,Nk] scores materialised)
FUSED_ATTENTION = True


def attention(Q, K, V, scale):
    """Fused multi-head attention (dcp.py:26-32): Q[P,Nq,H,128], K/V[P,Nk,H,128] (views of token-major [P,N,H*128] buffers)
    -> context[P,Nq,H,128] = softmax(Q K^T * scale) V per head; the scores never reach HBM (houv_attention_f32)."""
    _lib.require_gpu_any(Q, K, V)
    P, Nq, H, dk = Q.shape
    Nk = K.shape[1]
    if dk != 128 or tuple(K.shape) != (P, Nk, H, dk) or tuple(V.shape) != (P, Nk, H, dk):
        raise _lib.HouvHipError("attention: expected Q[P,Nq,H,128], K[P,Nk,H,128], V[P,Nk,H,128]")
    for t in (Q, K, V):
        if t.stride(3) != 1 or t.stride(2) != dk:
            raise _lib.HouvHipError("attention: heads must be contiguous 128-float slices of a token row")
    out = torch.empty((P, Nq, H, dk), dtype=_F32, device=Q.device)
    if GEMM_LOG is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(Q.device))
    _lib.call("houv_attention_f32", Q, Q, K, V, out, P, H, Nq, Nk, dk, Q.stride(1), K.stride(1), V.stride(1), out.stride(1),
              Q.stride(0) if P else 0, K.stride(0) if P else 0, V.stride(0) if P else 0, out.stride(0) if P else 0, scale)
    if GEMM_LOG is not None:
        ev1.record(torch.cuda.current_stream(Q.device))
        GEMM_LOG.append((ev0, ev1, 4.0 * P * H * Nq * Nk * dk))
    return out


def layernorm(x, a, b, eps=1e-6, residual=None):
    _lib.require_gpu(x, a, b, residual)
    for t, n in ((x, "x"), (a, "a"), (b, "b"), (residual, "residual")):
        if t is not None:
            _want(t, _F32, n)
    if x.dim() < 1:
        raise _lib.HouvHipError("layernorm: expected x[..., D]")
    D = x.shape[-1]
    if a.numel() != D or b.numel() != D or (residual is not None and residual.shape != x.shape):
        raise _lib.HouvHipError("layernorm: a, b must have D elements and residual the shape of x")
    if not _aligned16(x, a, b, residual):     # rows are read 16 bytes at a time (require_gpu has refused strided views)
        raise _lib.HouvHipError("layernorm: x, a, b and residual must start on 16-byte boundaries")
    rows = x.numel() // D
    out = torch.empty_like(x)
    _lib.call("houv_layernorm", x, x, rows, D, a, b, eps, residual, out)
    return out


def softmax_rows_(x):
    _lib.require_gpu(x); _want(x, _F32, "x")
    L = x.shape[-1]
    _lib.call("houv_softmax_rows", x, x, x.numel() // L, L)
    return x


def softmax_corr(scores, pts):
    """scores[P,N,M], pts[P,M,3] -> corr[P,3,N] = pts^T softmax(scores)^T."""
    _lib.require_gpu(scores, pts); _want(scores, _F32, "scores"); _want(pts, _F32, "pts")
    if scores.dim() != 3 or tuple(pts.shape) != (scores.shape[0], scores.shape[2], 3):
        raise _lib.HouvHipError("softmax_corr: expected scores[P,N,M], pts[P,M,3]")
    P, N, M = scores.shape
    corr = torch.empty((P, 3, N), dtype=_F32, device=scores.device)
    _lib.call("houv_softmax_corr", scores, scores, P, N, M, pts, corr)
    return corr
