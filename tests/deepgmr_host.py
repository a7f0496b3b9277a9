"""NumPy restatements of the DeepGMR contracts of include/houv_hip.h (houv_rri_features, houv_gmm_params, houv_gmm_register;
DESIGN.md section 9.7), written from the header, with the arithmetic type as an argument: float32 shows what the formula
itself loses in fp32, float64 is the yardstick the kernels are held to."""
import numpy as np


def rri_psi(xyz, idx, k, dtype=np.float64):
    """xyz[B,N,3], idx[B,N,k] -> (rp[B,N], rq[B,N,k], theta[B,N,k], psi[B,N,k,k]) with psi[..., j, i] in [0, 2 pi]."""
    xyz = np.asarray(xyz, dtype=dtype)
    idx = np.asarray(idx)[..., :k].astype(np.int64)
    B, N, _ = xyz.shape
    two_pi = dtype(2 * np.pi)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = xyz[:, :, None, :]                                             # [B,N,1,3]
        q = xyz[np.arange(B)[:, None, None], idx]                          # [B,N,k,3]
        rp = np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])        # [B,N,1]
        rq = np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2])        # [B,N,k]
        pn = p / rp[..., None]
        qn = q / rq[..., None]
        dot = (pn[..., 0] * qn[..., 0] + pn[..., 1] * qn[..., 1]) + pn[..., 2] * qn[..., 2]         # [B,N,k]
        theta = np.arccos(np.clip(dot, dtype(-1), dtype(1)))
        T = q - dot[..., None] * p                                         # the cosine times the UNNORMALISED p
        Ti = T[:, :, None, :, :]                                           # [B,N,1,k(i),3]
        Tj = T[:, :, :, None, :]                                           # [B,N,k(j),1,3]
        cx = Ti[..., 1] * Tj[..., 2] - Ti[..., 2] * Tj[..., 1]
        cy = Ti[..., 2] * Tj[..., 0] - Ti[..., 0] * Tj[..., 2]
        cz = Ti[..., 0] * Tj[..., 1] - Ti[..., 1] * Tj[..., 0]
        n = pn[:, :, :, None, :]                                           # [B,N,1,1,3]
        s = (cx * n[..., 0] + cy * n[..., 1]) + cz * n[..., 2]
        c = (Ti[..., 0] * Tj[..., 0] + Ti[..., 1] * Tj[..., 1]) + Ti[..., 2] * Tj[..., 2]
        psi = np.arctan2(s, c).astype(dtype)
        psi = np.where(psi < 0, psi + two_pi, psi)
        psi = np.where(psi == 0, dtype(0), psi)                            # -0 -> 0
    return rp[..., 0].astype(dtype), rq.astype(dtype), theta.astype(dtype), psi.astype(dtype)


def rri_features(xyz, idx, k, dtype=np.float64):
    """-> out[B,N,4k], channel 4*j + f; phi_j = second smallest of psi[j, :], NaNs last (np.sort puts them there)."""
    rp, rq, theta, psi = rri_psi(xyz, idx, k, dtype)
    phi = np.sort(psi, axis=-1)[..., 1]
    B, N = rp.shape
    out = np.stack([np.broadcast_to(rp[..., None], rq.shape), rq, theta, phi], axis=-1)
    return out.reshape(B, N, 4 * k).astype(dtype)


def gmm_params(gamma, pts, dtype=np.float64):
    """gamma[B,N,J], pts[B,N,3] -> pi[B,J], mu[B,J,3], sigma[B,J] (scalar of the isotropic covariance, not divided by 3)."""
    g = np.asarray(gamma, dtype=dtype)
    p = np.asarray(pts, dtype=dtype)
    N = g.shape[1]
    pi = g.sum(1) / dtype(N)
    npi = pi * dtype(N)
    mu = np.einsum("bnj,bnc->bjc", g, p) / npi[..., None]
    d = p[:, :, None, :] - mu[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    sigma = (g * d2).sum(1) / npi
    return pi.astype(dtype), mu.astype(dtype), sigma.astype(dtype)


def gmm_register(pi_s, mu_s, mu_t, sigma_t, dtype=np.float64, return_svd=False):
    """-> T[B,4,4] = [[R, t], [0,0,0,1]], R = V diag(1,1,det(V U^T)) U^T of Ms = U S V^T."""
    w = np.asarray(pi_s, dtype=dtype)
    ms = np.asarray(mu_s, dtype=dtype)
    mt = np.asarray(mu_t, dtype=dtype)
    sg = np.asarray(sigma_t, dtype=dtype)
    cs = np.einsum("bj,bjc->bc", w, ms)
    ct = np.einsum("bj,bjc->bc", w, mt)
    a = w[..., None] * (ms - cs[:, None])
    c = (mt - ct[:, None]) / sg[..., None]
    Ms = np.einsum("bji,bjl->bil", a, c).astype(dtype)
    U, S, Vt = np.linalg.svd(Ms)
    V = np.swapaxes(Vt, 1, 2)
    d = np.linalg.det(V @ np.swapaxes(U, 1, 2)).astype(dtype)
    D = np.tile(np.eye(3, dtype=dtype), (len(w), 1, 1))
    D[:, 2, 2] = d
    R = V @ D @ np.swapaxes(U, 1, 2)
    t = ct - np.einsum("bil,bl->bi", R, cs)
    T = np.zeros((len(w), 4, 4), dtype=dtype)
    T[:, :3, :3] = R
    T[:, :3, 3] = t
    T[:, 3, 3] = 1
    return (T, Ms, S, d) if return_svd else T
