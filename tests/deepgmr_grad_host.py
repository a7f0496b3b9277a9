"""NumPy restatements of the DeepGMR training contracts of include/houv_hip.h (houv_bn_rows_stats, houv_bn_relu_rows,
houv_bn_relu_rows_backward, houv_gmm_params_backward, houv_gmm_register_backward), written from the
header with the arithmetic type as an argument: float32 shows what the formulas themselves lose in fp32, float64 is the yardstick
the kernels are held to.  `train_step` chains them with tests/deepgmr_host.py into one training step of the whole model."""
import numpy as np

import deepgmr_host as fwd

CHUNK = 128                    # rows per partial of the statistics and of the backward's column sums (bn_rows.hip kBnChunk)


def _rows_sum(a, dtype):
    """Column sums of a chunk, the rows added one after the other in ascending order."""
    s = np.zeros(a.shape[1], dtype)
    for row in a:
        s = s + row
    return s


def bn_rows_stats(z, dtype=np.float64):
    """z[R,C] -> (mean[C], var[C]), var biased about the mean: per chunk of CHUNK rows (count, mean, M2) by two passes, the
    chunks combined in chunk order (Chan et al.); never E[z^2] - mean^2."""
    z = np.asarray(z, dtype=dtype)
    R, C = z.shape
    n, mean, m2 = dtype(0), np.zeros(C, dtype), np.zeros(C, dtype)
    for r0 in range(0, R, CHUNK):
        c = z[r0:r0 + CHUNK]
        nb = dtype(len(c))
        mb = _rows_sum(c, dtype) / nb
        d = c - mb
        m2b = _rows_sum(d * d, dtype)
        if r0 == 0:
            n, mean, m2 = nb, mb, m2b
            continue
        tot = n + nb
        delta = mb - mean
        mean = mean + delta * (nb / tot)
        m2 = (m2 + m2b) + (delta * delta) * (n * (nb / tot))
        n = tot
    return mean.astype(dtype), (m2 / dtype(R)).astype(dtype)


def _normalised(z, mean, var, weight, bias, eps, dtype):
    z = np.asarray(z, dtype=dtype)
    rstd = dtype(1) / np.sqrt(np.asarray(var, dtype=dtype) + dtype(eps))
    xhat = (z - np.asarray(mean, dtype=dtype)) * rstd
    return xhat, rstd, xhat * np.asarray(weight, dtype=dtype) + np.asarray(bias, dtype=dtype)


def bn_relu_rows(z, mean, var, weight, bias, eps=1e-5, relu=True, n_group=0, dtype=np.float64):
    """-> y[R,C] (, gmax[R/n_group,C], garg[R/n_group,C] int32: the column maximum over each group of n_group rows and the lowest
    row index, counted over all R rows, that attains it)."""
    _, _, y = _normalised(z, mean, var, weight, bias, eps, dtype)
    if relu:
        y = np.maximum(y, dtype(0))
    if not n_group:
        return y
    R, C = y.shape
    g = y.reshape(R // n_group, n_group, C)
    arg = g.argmax(1)                                                      # first occurrence = lowest row
    return y, g.max(1), (arg + np.arange(R // n_group)[:, None] * n_group).astype(np.int32)


def bn_relu_rows_backward(gy, z, mean, var, weight, bias, eps=1e-5, relu=True, dtype=np.float64):
    """-> gz[R,C], gweight[C], gbias[C]; the ReLU mask and xhat are recomputed from z."""
    xhat, rstd, y = _normalised(z, mean, var, weight, bias, eps, dtype)
    g = np.asarray(gy, dtype=dtype)
    if relu:
        g = g * (y > 0)
    R = dtype(len(g))
    sg = np.zeros(g.shape[1], dtype)
    sgx = np.zeros(g.shape[1], dtype)
    for r0 in range(0, len(g), CHUNK):                                     # chunk order, as the kernel combines its partials
        sg = sg + _rows_sum(g[r0:r0 + CHUNK], dtype)
        sgx = sgx + _rows_sum(g[r0:r0 + CHUNK] * xhat[r0:r0 + CHUNK], dtype)
    gz = (np.asarray(weight, dtype=dtype) * rstd) * ((g - sg / R) - xhat * (sgx / R))
    return gz.astype(dtype), sgx.astype(dtype), sg.astype(dtype)


def gmm_params_backward(gamma, pts, pi, mu, sigma, g_pi, g_mu, g_sigma, dtype=np.float64):
    """-> g_logits[B,N,J]: the gradient of (pi, mu, sigma) = gmm_params(softmax(logits), pts) with respect to the logits."""
    f = lambda a: np.asarray(a, dtype=dtype)
    gamma, pts, pi, mu, sigma, g_pi, g_mu, g_sigma = map(f, (gamma, pts, pi, mu, sigma, g_pi, g_mu, g_sigma))
    N = dtype(gamma.shape[1])
    s0 = (pi * N)[:, None, :]                                              # [B,1,J]
    d = pts[:, :, None, :] - mu[:, None, :, :]                             # [B,N,J,3]  (host only: the kernel never builds it)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    gm = (g_mu[:, None, :, 0] * d[..., 0] + g_mu[:, None, :, 1] * d[..., 1]) + g_mu[:, None, :, 2] * d[..., 2]
    gg = g_pi[:, None, :] / N + (gm + g_sigma[:, None, :] * (d2 - sigma[:, None, :])) / s0
    dot = (gamma * gg).sum(2, keepdims=True)
    return (gamma * (gg - dot)).astype(dtype)


def _skew_solve(U, lam, X):
    """B~_ij = (U^T skew(X) U)_ij / (lam_i + lam_j), i != j; skew(X) = (X - X^T) / 2."""
    A = U.T @ ((X - X.T) / 2) @ U
    Bt = np.zeros_like(A)
    for i in range(3):
        for j in range(3):
            if i != j:
                Bt[i, j] = A[i, j] / (lam[i] + lam[j])
    return Bt


def gmm_register_backward(pi_s, mu_s, mu_t, sigma_t, g_T, dtype=np.float64, return_gap=False):
    """-> g_pi_s[B,J], g_mu_s[B,J,3], g_mu_t[B,J,3], g_sigma_t[B,J] of T = gmm_register(...), through the polar form of the
    rotation's derivative: with Ms = U S V^T, R = V D U^T, lam = (s1, s2, D33 s3),
    g_Ms = -2 U B~ U^T R^T, B~_ij = (U^T skew(R^T G_R) U)_ij / (lam_i + lam_j)."""
    w, ms, mt, sg, gT = (np.asarray(a, dtype=dtype) for a in (pi_s, mu_s, mu_t, sigma_t, g_T))
    B, J = w.shape
    out = [np.zeros_like(w), np.zeros_like(ms), np.zeros_like(mt), np.zeros_like(sg)]
    gap = np.inf
    for b in range(B):
        cs, ct = w[b] @ ms[b], w[b] @ mt[b]
        a = w[b][:, None] * (ms[b] - cs)
        c = (mt[b] - ct) / sg[b][:, None]
        Ms = a.T @ c
        U, S, Vt = np.linalg.svd(Ms)
        V = Vt.T
        d = np.linalg.det(V @ U.T)
        D = np.diag(np.array([1, 1, d], dtype=dtype))
        R = V @ D @ U.T
        lam = np.array([S[0], S[1], d * S[2]], dtype=dtype)
        gap = min(gap, lam[0] + lam[1], lam[0] + lam[2], lam[1] + lam[2])
        g_t = gT[b, :3, 3]
        G_R = gT[b, :3, :3] - np.outer(g_t, cs)
        g_Ms = -2 * U @ _skew_solve(U, lam, R.T @ G_R) @ U.T @ R.T
        g_a = c @ g_Ms.T                                                   # [J,3]: g_a_j = g_Ms c_j
        g_c = a @ g_Ms                                                     # g_c_j = g_Ms^T a_j
        g_cs = -R.T @ g_t - (w[b][:, None] * g_a).sum(0)
        g_ct = g_t - (g_c / sg[b][:, None]).sum(0)
        out[0][b] = (g_a * (ms[b] - cs)).sum(1) + ms[b] @ g_cs + mt[b] @ g_ct
        out[1][b] = w[b][:, None] * (g_a + g_cs)
        out[2][b] = g_c / sg[b][:, None] + w[b][:, None] * g_ct
        out[3][b] = -(g_c * c).sum(1) / sg[b]
    out = [o.astype(dtype) for o in out]
    return (out, float(gap)) if return_gap else out


# ----------------------------------------------------------------------------------------------------------------------------
# one training step of the whole model (registration/models/deepgmr.py, Model.forward with prefix "train", then backward)
# ----------------------------------------------------------------------------------------------------------------------------
ENC = ("backbone.encoder.0", "backbone.encoder.1", "backbone.encoder.2", "backbone.encoder.3")
DEC = ("backbone.decoder.0", "backbone.decoder.1", "backbone.decoder.2")
LAST = "backbone.decoder.3"


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


class _Backbone:
    """PointNet.forward in train mode on rows x[B*N, 4k] and its backward; records the batch statistics and the max-pool rows."""

    def __init__(self, state, dtype, eps=1e-5):
        self.s = {k: np.asarray(v, dtype=dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}
        self.dtype, self.eps = dtype, eps
        self.grads = {}
        self.stats = []                                                    # (layer name, mean, biased var, R) per call

    def _add(self, name, g):
        self.grads[name] = self.grads.get(name, 0) + g

    def _layer(self, name, z):
        mean, var = bn_rows_stats(z, self.dtype)
        self.stats.append((name, mean, var, len(z)))
        return mean, var

    def forward(self, x, B, N):
        dt, s = self.dtype, self.s
        tape, h = [], np.asarray(x, dtype=dt)
        for name in ENC:
            W = s[name + ".conv.weight"][:, :, 0]
            z = h @ W.T
            mean, var = self._layer(name, z)
            tape.append((name, h, z, mean, var))
            h = bn_relu_rows(z, mean, var, s[name + ".bn.weight"], s[name + ".bn.bias"], self.eps, True, 0, dt)
        C = h.shape[1]
        arg = h.reshape(B, N, C).argmax(1)                                  # lowest row on ties
        f_glob = np.take_along_axis(h.reshape(B, N, C), arg[:, None, :], 1)[:, 0]
        W = s[DEC[0] + ".conv.weight"][:, :, 0]
        z = h @ W[:, :C].T + np.repeat(f_glob @ W[:, C:].T, N, axis=0)
        mean, var = self._layer(DEC[0], z)
        tape.append((DEC[0], (h, f_glob, arg), z, mean, var))
        h = bn_relu_rows(z, mean, var, s[DEC[0] + ".bn.weight"], s[DEC[0] + ".bn.bias"], self.eps, True, 0, dt)
        for name in DEC[1:]:
            W = s[name + ".conv.weight"][:, :, 0]
            z = h @ W.T
            mean, var = self._layer(name, z)
            tape.append((name, h, z, mean, var))
            h = bn_relu_rows(z, mean, var, s[name + ".bn.weight"], s[name + ".bn.bias"], self.eps, True, 0, dt)
        logits = h @ s[LAST + ".weight"][:, :, 0].T + s[LAST + ".bias"]
        self.tape, self.last_in, self.shape, self.pool_rows = tape, h, (B, N), arg
        return logits

    def backward(self, g_logits):
        dt, s = self.dtype, self.s
        B, N = self.shape
        self._add(LAST + ".weight", (g_logits.T @ self.last_in)[:, :, None])
        self._add(LAST + ".bias", g_logits.sum(0))
        g = g_logits @ s[LAST + ".weight"][:, :, 0]
        for name, h, z, mean, var in reversed(self.tape):
            gz, gw, gb = bn_relu_rows_backward(g, z, mean, var, s[name + ".bn.weight"], s[name + ".bn.bias"], self.eps, True, dt)
            self._add(name + ".bn.weight", gw)
            self._add(name + ".bn.bias", gb)
            W = s[name + ".conv.weight"][:, :, 0]
            if name == DEC[0]:
                f_loc, f_glob, arg = h
                C = f_loc.shape[1]
                gres = gz.reshape(B, N, -1).sum(1)                          # [B,512]: the residual row's gradient
                self._add(name + ".conv.weight", np.concatenate([gz.T @ f_loc, gres.T @ f_glob], 1)[:, :, None])
                g = gz @ W[:, :C]
                gglob = gres @ W[:, C:]                                     # [B,1024], back to f_loc through the max-pool rows
                g3 = g.reshape(B, N, C)
                np.put_along_axis(g3, arg[:, None, :], np.take_along_axis(g3, arg[:, None, :], 1) + gglob[:, None, :], 1)
                g = g3.reshape(B * N, C)
            else:
                self._add(name + ".conv.weight", (gz.T @ h)[:, :, None])
                g = gz @ W if name != ENC[0] else None


def train_step(state, src, tgt, T_gt, knn1, knn2, k, dtype=np.float64):
    """One forward + backward of the reference's DeepGMR in train mode, from the restatements above.  state: the reference's
    state_dict as arrays; knn1 / knn2: the neighbour lists the features are built on.  -> dict(loss, grads{name: array},
    stats[(layer, mean, var, R)] in call order, pool1, pool2 (the max-pool rows [B,1024], row index within the cloud))."""
    dt = dtype
    src, tgt, T_gt = (np.asarray(a, dtype=dt) for a in (src, tgt, T_gt))
    B, N, _ = src.shape
    net = _Backbone(state, dt)
    clouds, tapes = (src, tgt), []
    for pts, idx in ((src, knn1), (tgt, knn2)):
        x = fwd.rri_features(pts, idx, k, dt).reshape(B * N, 4 * k)
        logits = net.forward(x, B, N)
        gamma = _softmax(logits).reshape(B, N, -1)
        pi, mu, sigma = fwd.gmm_params(gamma, pts, dt)
        tapes.append((net.tape, net.last_in, net.pool_rows, gamma, pi, mu, sigma))
    (_, _, pool1, g1, pi1, mu1, sg1), (_, _, pool2, g2, pi2, mu2, sg2) = tapes
    T12 = fwd.gmm_register(pi1, mu1, mu2, sg2, dt)
    T21 = fwd.gmm_register(pi2, mu2, mu1, sg1, dt)
    eye = np.eye(4, dtype=dt)
    Ginv = np.linalg.inv(T_gt)
    E1, E2 = T12 @ Ginv - eye, T21 @ T_gt - eye
    loss = (E1 * E1).mean() + (E2 * E2).mean()
    scale = dt(2) / dt(E1.size)
    gT12 = scale * E1 @ np.swapaxes(Ginv, 1, 2)
    gT21 = scale * E2 @ np.swapaxes(T_gt, 1, 2)
    a_pi1, a_mu1, a_mu2, a_sg2 = gmm_register_backward(pi1, mu1, mu2, sg2, gT12, dt)
    b_pi2, b_mu2, b_mu1, b_sg1 = gmm_register_backward(pi2, mu2, mu1, sg1, gT21, dt)
    heads = ((a_pi1, a_mu1 + b_mu1, b_sg1), (b_pi2, a_mu2 + b_mu2, a_sg2))
    for i in (1, 0):                                                        # autograd order: the second cloud's graph first
        tape, last_in, pool, gamma, pi, mu, sigma = tapes[i]
        net.tape, net.last_in, net.pool_rows = tape, last_in, pool
        gl = gmm_params_backward(gamma, clouds[i], pi, mu, sigma, *heads[i], dtype=dt)
        net.backward(gl.reshape(B * N, -1))
    return dict(loss=loss, grads=net.grads, stats=net.stats, pool1=pool1, pool2=pool2, T12=T12, T21=T21)
