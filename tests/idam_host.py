"""NumPy restatements of the IDAM contracts of include/houv_hip.h (houv_idam_simmat, houv_edge_diff) and of
the model around them (registration/models/idam.py: Propagate / GNN, the significance head, one full iteration, the whole
test-prefix forward), with the arithmetic type as an argument: float32 shows what the formulas themselves lose in fp32, float64
is the yardstick the kernels are held to.  `state` is a dict of NumPy arrays under the reference's state_dict names."""
import numpy as np

K_NN = 12
BN_EPS = 1e-5


def edge_diff(x, idx, k=None, ldo=None):
    """x[B,N,C], idx[B,N,L] -> out[B*N*k, ldo]: x[b, clamp(idx[b,n,j])] - x[b,n] in columns < C, zeros after (same dtype as x)."""
    x = np.asarray(x)
    B, N, C = x.shape
    k = idx.shape[2] if k is None else k
    ldo = C if ldo is None else ldo
    q = np.clip(np.asarray(idx)[..., :k].astype(np.int64), 0, N - 1)
    out = np.zeros((B, N, k, ldo), dtype=x.dtype)
    out[..., :C] = x[np.arange(B)[:, None, None], q] - x[:, :, None, :]
    return out.reshape(B * N * k, ldo)


def _chain(x, W, start=None):
    """x[..., K] . W[C, K]^T (+ start[C]) as the contract's chain over k ascending: element-wise operations only, so that equal
    inputs give equal results wherever they sit in the array (a BLAS product does not promise that)."""
    acc = np.zeros(x.shape[:-1] + (W.shape[0],), dtype=x.dtype) + (0 if start is None else start)
    for k in range(W.shape[1]):
        acc = acc + x[..., k, None] * W[:, k]
    return acc


def simmat(src, tgt, es, et, par, dtype=np.float64):
    """par = (W1[32,2E+4], s1, t1, W2, b2, W3, s3, t3, w4, b4) -> dict(rowmax[B,Ms,32], scores[B,Ms,Mt], corr_idx[B,Ms],
    corr[B,3,Ms]); arg-max takes the lowest j among equal scores (np.argmax returns the first)."""
    src, tgt, es, et = (np.asarray(a, dtype=dtype) for a in (src, tgt, es, et))
    W1, s1, t1, W2, b2, W3, s3, t3, w4, b4 = (np.asarray(a, dtype=dtype) for a in par)
    E = es.shape[2]
    P = _chain(es, W1[:, :E])                                              # [B,Ms,32]
    Q = _chain(et, W1[:, E:2 * E])                                         # [B,Mt,32]
    diff = src[:, :, None, :] - tgt[:, None, :, :]                         # [B,Ms,Mt,3]
    d = np.sqrt((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2])
    u = diff / (d + dtype(1e-8))[..., None]
    pair = _chain(u, W1[:, 2 * E + 1:], d[..., None] * W1[:, 2 * E])
    pre = (P[:, :, None, :] + Q[:, None, :, :]) + pair
    h1 = np.maximum(s1 * pre + t1, dtype(0))
    h2 = _chain(h1, W2, b2)
    rowmax = h2.max(axis=2)
    h3 = np.maximum(s3 * _chain(h2, W3) + t3, dtype(0))
    scores = np.clip(_chain(h3, w4[None, :], b4.reshape(1))[..., 0], dtype(-20), dtype(20))
    cidx = scores.argmax(axis=-1)
    corr = np.swapaxes(tgt[np.arange(len(tgt))[:, None], cidx], 1, 2)
    return dict(rowmax=rowmax.astype(dtype), scores=scores.astype(dtype), corr_idx=cidx.astype(np.int32), corr=corr)


def flagged_rows(scores64, bound):
    """A row is flagged when its best two DISTINCT float64 score values differ by less than `bound` and are not both exactly
    +-20 (a row with a single distinct value is never flagged)."""
    s = np.sort(scores64, axis=-1)[..., ::-1]
    top = s[..., :1]
    lower = np.where(s < top, s, -np.inf).max(axis=-1)                     # the second distinct value, -inf when there is none
    top = top[..., 0]
    both_clamped = (np.abs(top) == 20) & (np.abs(lower) == 20)
    return (top - lower < bound) & ~both_clamped


# ---------------------------------------------------------------------------------------------------------------- the model
def _bn(state, prefix, dtype):
    w, b, m, v = (np.asarray(state[f"{prefix}.{n}"], dtype=dtype) for n in ("weight", "bias", "running_mean", "running_var"))
    scale = w / np.sqrt(v + dtype(BN_EPS))
    return scale, b - m * scale


def _w(state, name, dtype):
    a = np.asarray(state[name], dtype=dtype)
    return a.reshape(a.shape[0], a.shape[1])


def simmat_params(state, i, dtype=np.float64):
    """The ten arrays of houv_idam_simmat for iteration i, BatchNorm folded."""
    a, b = f"sim_mat_conv1.{i}.conv", f"sim_mat_conv2.{i}.conv"
    s1, t1 = _bn(state, f"{a}.0.bn", dtype)
    s3, t3 = _bn(state, f"{b}.0.bn", dtype)
    return (_w(state, f"{a}.0.conv.weight", dtype), s1, t1, _w(state, f"{a}.1.weight", dtype),
            np.asarray(state[f"{a}.1.bias"], dtype=dtype), _w(state, f"{b}.0.conv.weight", dtype), s3, t3,
            _w(state, f"{b}.1.weight", dtype)[0], np.asarray(state[f"{b}.1.bias"], dtype=dtype))


def conv1d_block(state, prefix, n_bn, x, dtype):
    """Conv1DBlock on rows x[..., C]: n_bn conv+BN+ReLU layers, then a biased convolution."""
    for l in range(n_bn):
        s, t = _bn(state, f"{prefix}.conv.{l}.bn", dtype)
        x = np.maximum(s * (x @ _w(state, f"{prefix}.conv.{l}.conv.weight", dtype).T) + t, dtype(0))
    return x @ _w(state, f"{prefix}.conv.{n_bn}.weight", dtype).T + np.asarray(state[f"{prefix}.conv.{n_bn}.bias"], dtype=dtype)


def propagate(state, prefix, x, idx, dtype):
    """x[B,N,C], idx[B,N,k] -> [B,N,64] (idam.py:115-128): subtract, then convolve."""
    B, N, C = x.shape
    k = idx.shape[2]
    d = edge_diff(x, idx).reshape(B, N, k, C)
    s, t = _bn(state, f"{prefix}.conv2d.conv.0.bn", dtype)
    h = np.maximum(s * (d @ _w(state, f"{prefix}.conv2d.conv.0.conv.weight", dtype).T) + t, dtype(0))
    h = h @ _w(state, f"{prefix}.conv2d.conv.1.weight", dtype).T + np.asarray(state[f"{prefix}.conv2d.conv.1.bias"], dtype=dtype)
    return conv1d_block(state, f"{prefix}.conv1d", 0, h.max(axis=2), dtype)


def embed(state, cloud, idx, dtype=np.float64):
    """GNN (idam.py:131-149) on cloud[B,N,3] with neighbour lists idx[B,N,12] (self included) -> [B,N,E]."""
    x = np.asarray(cloud, dtype=dtype)
    for l in range(1, 6):
        x = propagate(state, f"emb_nn.propogate{l}", x, idx, dtype)
    return x


def significance(state, emb, dtype=np.float64):
    return conv1d_block(state, "significance_fc", 2, np.asarray(emb, dtype=dtype), dtype)[..., 0]


def keep(sig, M):
    """topk(M) on the significance: indices by descending score."""
    return np.argsort(-sig, axis=-1, kind="stable")[:, :M]


def kabsch(src, corr, w, dtype):
    """SVDHead (idam.py:152-188) on rows src[B,M,3], corr[B,M,3], w[B,M]: unweighted centring, weighted covariance."""
    sc = src - src.mean(axis=1, keepdims=True)
    cc = corr - corr.mean(axis=1, keepdims=True)
    H = np.einsum("bn,bni,bnj->bij", w, sc, cc)
    U, S, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, 1, 2)
    R = V @ np.swapaxes(U, 1, 2)
    neg = np.linalg.det(R) < 0
    V[neg, :, 2] *= -1
    R = V @ np.swapaxes(U, 1, 2)
    t = -np.einsum("bij,bj->bi", R, (w[..., None] * src).sum(1)) + (w[..., None] * corr).sum(1)
    return R.astype(dtype), t.astype(dtype)


def iteration(state, i, src, tgt, es, et, dtype=np.float64):
    """One pass of idam.py:267-342 on the kept points (rows).  -> dict(rowmax, scores, corr_idx, weights, R, t, src) with `src`
    the moved source for the next iteration."""
    src, tgt = np.asarray(src, dtype=dtype), np.asarray(tgt, dtype=dtype)
    out = simmat(src, tgt, es, et, simmat_params(state, i, dtype), dtype)
    logit = conv1d_block(state, f"weight_fc.{i}", 1, out["rowmax"], dtype)[..., 0]
    w = dtype(1) / (dtype(1) + np.exp(-logit))
    M = w.shape[1]
    med = np.sort(w, axis=-1)[:, (M - 1) // 2][:, None]                    # the LOWER median (torch.median)
    w = w * (w >= med)
    w = w / (w.sum(-1, keepdims=True) + dtype(1e-8))
    R, t = kabsch(src, np.swapaxes(out["corr"], 1, 2), w, dtype)
    out.update(weights=w.astype(dtype), R=R, t=t, src=(src @ np.swapaxes(R, 1, 2) + t[:, None]).astype(dtype))
    return out


def forward(state, src, tgt, knn_src, knn_tgt, num_iters=3, dtype=np.float64):
    """The test-prefix forward (idam.py:204-346).  -> dict(emb_src, emb_tgt, sig_src, sig_tgt, src_idx, tgt_idx, iters, T)."""
    src, tgt = np.asarray(src, dtype=dtype), np.asarray(tgt, dtype=dtype)
    B, N, _ = src.shape
    e_t = embed(state, tgt, knn_tgt, dtype)
    e_s = embed(state, src, knn_src, dtype)
    g_s, g_t = significance(state, e_s, dtype), significance(state, e_t, dtype)
    i_s, i_t = keep(g_s, N // 6), keep(g_t, N // 6)
    bi = np.arange(B)[:, None]
    s, t_pts, es, et = src[bi, i_s], tgt[bi, i_t], e_s[bi, i_s], e_t[bi, i_t]
    R = np.tile(np.eye(3, dtype=dtype), (B, 1, 1))
    t = np.zeros((B, 3), dtype=dtype)
    iters = []
    for i in range(num_iters):
        it = iteration(state, i, s, t_pts, es, et, dtype)
        s = it["src"]
        R = it["R"] @ R
        t = np.einsum("bij,bj->bi", it["R"], t) + it["t"]
        iters.append(it)
    T = np.zeros((B, 4, 4), dtype=dtype)
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, t, 1
    return dict(emb_src=e_s, emb_tgt=e_t, sig_src=g_s, sig_tgt=g_t, src_idx=i_s, tgt_idx=i_t, iters=iters, T=T)


def compose(Rs, ts, dtype=np.float64):
    """The pose of the whole forward from the per-iteration poses (idam.py:340-344): R <- R_i R, t <- R_i t + t_i -> T[B,4,4]."""
    B = len(Rs[0])
    R = np.tile(np.eye(3, dtype=dtype), (B, 1, 1))
    t = np.zeros((B, 3), dtype=dtype)
    for R_i, t_i in zip(Rs, ts):
        R_i, t_i = np.asarray(R_i, dtype=dtype), np.asarray(t_i, dtype=dtype)
        R = R_i @ R
        t = np.einsum("bij,bj->bi", R_i, t) + t_i
    T = np.zeros((B, 4, 4), dtype=dtype)
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, t, 1
    return T


def stepwise(state, src_at, tgt, es, et, dtype=np.float64):
    """Every iteration from GIVEN inputs: src_at[i][B,M,3] is the (moved) kept source on entry to iteration i, as some other run
    had it.  Two precisions, or a model and its yardstick, then never drift apart through one flipped median mask or one
    near-tied correspondence: each iteration is compared on common ground.  -> (list of `iteration` dicts, T composed of them)."""
    its = [iteration(state, i, s, tgt, es, et, dtype) for i, s in enumerate(src_at)]
    return its, compose([it["R"] for it in its], [it["t"] for it in its], dtype)
