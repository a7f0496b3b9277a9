"""NumPy restatement of houv_ef_expand and houv_ef_expand_backward: EF_expansion with everything that
depends on one point alone computed once per point.  dtype-parametrised: float64 is the yardstick, float32 measures the spread
of the format on a case.  `faults` plants the mistakes tests/test_ef_expand_host.py must be able to see."""
import numpy as np


def relu(a):
    return np.where(a < 0, np.zeros_like(a), a)                                   # a NaN stays a NaN


def projections(x, W1, b1, W2, b2, dtype=np.float64):
    """x[B,N,C] rows, conv1 [O,2C] / [O], conv2 [O r, O + 2C] / [O r] -> (proj[B,N,2O+2Or] = [U | V | P | Q], W2a[O r, O])."""
    x, W1, b1, W2, b2 = (np.asarray(a, dtype=dtype) for a in (x, W1, b1, W2, b2))
    C, O = x.shape[2], W1.shape[0]
    rx = relu(x)
    U = x @ W1[:, :C].T + b1
    V = x @ W1[:, C:].T
    P = rx @ W2[:, O:O + C].T + b2
    Q = rx @ W2[:, O + C:].T
    return np.concatenate([U, V, P, Q], axis=2).astype(dtype), np.ascontiguousarray(W2[:, :O])


def _edges(proj, idx, W2a, r, faults=()):
    """h1[B,N,k,O], t[B,N,k,r,O] of every edge (n, j), m = clamp(idx[b,n,j])."""
    B, N, W = proj.shape
    O = W // (2 + 2 * r)
    m = idx.astype(np.int64)
    if "unclamped" in faults:
        m = m % N
    else:
        m = np.clip(m, 0, N - 1)
    U, V, P, Q = proj[..., :O], proj[..., O:2 * O], proj[..., 2 * O:2 * O + O * r], proj[..., 2 * O + O * r:]
    bi = np.arange(B)[:, None, None]
    h1 = U[:, :, None, :] + V[bi, m]                                              # B N k O
    t = np.einsum("bnjc,oc->bnjo", relu(h1), W2a)                                 # B N k Or
    if "no_P" not in faults:
        t = t + P[:, :, None, :]
    t = t + Q[bi, m]
    if "stride" in faults:                                                        # sub-row s = every r-th channel from s
        t = t.reshape(B, N, -1, O, r).transpose(0, 1, 2, 4, 3)
    else:                                                                         # sub-row s = the s-th run of O channels
        t = t.reshape(B, N, -1, r, O)
    return m, h1, t


def slots(proj, idx, W2a, W3, b3, r, dtype=np.float64, faults=()):
    """e[B,N,k,r,O]: conv3's output of every (point, slot, sub-row), before the maximum."""
    proj, W2a, W3, b3 = (np.asarray(a, dtype=dtype) for a in (proj, W2a, W3, b3))
    _, _, t = _edges(proj, idx, W2a, r, faults)
    e = np.einsum("bnjsc,oc->bnjso", relu(t), W3) + b3
    assert e.dtype == dtype
    return e


def forward(proj, idx, W2a, W3, b3, r, dtype=np.float64, faults=()):
    """-> (out[B, N r, O], arg[B, N r, O] int8): the maximum over the slots, the LOWEST slot that attains it (faults: the
    highest), a NaN skipped, an all-NaN column NaN with arg -1."""
    e = slots(proj, idx, W2a, W3, b3, r, dtype, faults)                           # B N k r O
    B, N, k, _, O = e.shape
    best = np.full((B, N, r, O), np.nan, dtype=dtype)
    arg = np.full((B, N, r, O), -1, dtype=np.int8)
    for j in range(k):
        v = e[:, :, j]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(v) & ((arg < 0) | ((v >= best) if "highest" in faults else (v > best)))
        best = np.where(take, v, best)
        arg = np.where(take, np.int8(j), arg)
    return best.reshape(B, N * r, O), arg.reshape(B, N * r, O)


def backward(proj, idx, arg, W2a, W3, g, r, dtype=np.float64):
    """-> dict(gproj[B,N,2O+2Or], gW2a[O r, O], gW3[O,O], gb3[O]) under the given arg."""
    proj, W2a, W3, g = (np.asarray(a, dtype=dtype) for a in (proj, W2a, W3, g))
    B, N, W = proj.shape
    O = W3.shape[0]
    m, h1, t = _edges(proj, idx, W2a, r)
    k = m.shape[2]
    a = np.asarray(arg).reshape(B, N, 1, r, O)
    ge = np.where(a == np.arange(k).reshape(1, 1, k, 1, 1), g.reshape(B, N, 1, r, O), dtype(0))      # B N k r O
    gh2 = np.einsum("bnjsc,ci->bnjsi", ge, W3)
    gt = np.where(t > 0, gh2, dtype(0))
    gh1 = np.einsum("bnjsc,sci->bnji", gt, W2a.reshape(r, O, O))
    gh1 = np.where(h1 > 0, gh1, dtype(0))
    gtf = gt.reshape(B, N, k, r * O)
    gV, gQ = np.zeros((B, N, O), dtype=dtype), np.zeros((B, N, r * O), dtype=dtype)
    for b in range(B):
        np.add.at(gV[b], m[b].reshape(-1), gh1[b].reshape(-1, O))
        np.add.at(gQ[b], m[b].reshape(-1), gtf[b].reshape(-1, r * O))
    gproj = np.concatenate([gh1.sum(2), gV, gtf.sum(2), gQ], axis=2)
    rh1 = relu(h1)
    return {"gproj": gproj.astype(dtype),
            "gW2a": np.einsum("bnjso,bnjc->soc", gt, np.where(np.isnan(rh1), dtype(0), rh1)).reshape(r * O, O).astype(dtype),
            "gW3": np.einsum("bnjsc,bnjsi->ci", ge, np.where(np.isnan(t), dtype(0), relu(t))).astype(dtype),
            "gb3": ge.sum((0, 1, 2, 3)).astype(dtype)}


def block(x, idx, W1, b1, W2, b2, W3, b3, r, dtype=np.float64, G=None, arg=None):
    """The whole EF_expansion on rows x[B,N,C] given its lists: -> (out, arg) or, with G[B, N r, O], (out, arg, gradients of
    L = <G, out> with respect to x and the six parameters, under `arg` when given, else the forward's own)."""
    x, W1, b1, W2, b2, W3, b3 = (np.asarray(a, dtype=dtype) for a in (x, W1, b1, W2, b2, W3, b3))
    C, O = x.shape[2], W3.shape[0]
    proj, W2a = projections(x, W1, b1, W2, b2, dtype)
    out, own = forward(proj, idx, W2a, W3, b3, r, dtype)
    if G is None:
        return out, own
    g = backward(proj, idx, own if arg is None else arg, W2a, W3, G, r, dtype)
    gp = g["gproj"]
    gU, gV, gP, gQ = gp[..., :O], gp[..., O:2 * O], gp[..., 2 * O:2 * O + O * r], gp[..., 2 * O + O * r:]
    rx = relu(x)
    rows = lambda a: a.reshape(-1, a.shape[-1])
    gx = gU @ W1[:, :C] + gV @ W1[:, C:] + (gP @ W2[:, O:O + C] + gQ @ W2[:, O + C:]) * (x > 0)
    grads = {"x": gx,
             "conv1.weight": np.concatenate([rows(gU).T @ rows(x), rows(gV).T @ rows(x)], axis=1), "conv1.bias": rows(gU).sum(0),
             "conv2.weight": np.concatenate([g["gW2a"], rows(gP).T @ rows(rx), rows(gQ).T @ rows(rx)], axis=1),
             "conv2.bias": rows(gP).sum(0), "conv3.weight": g["gW3"], "conv3.bias": g["gb3"]}
    return out, own, {n: v.astype(dtype) for n, v in grads.items()}


def margins(x, idx, W1, b1, W2, b2, W3, b3, r):
    """(smallest non-zero |ReLU input|, smallest lead of a maximum over its runner-up, the float32-vs-float64 spread of the ReLU
    inputs and of the candidates) of the float64 restatement: what a fixture's seed must keep apart."""
    res = {}
    for dt in (np.float64, np.float32):
        a = [np.asarray(v, dtype=dt) for v in (x, W1, b1, W2, b2, W3, b3)]
        proj, W2a = projections(*a[:5], dt)
        _, h1, t = _edges(proj, idx, W2a, r)
        res[dt] = (h1, t, slots(proj, idx, W2a, a[5], a[6], r, dt))
    h1, t, e = res[np.float64]
    spread = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(res[np.float32], res[np.float64]))
    kinks = np.concatenate([np.abs(h1).reshape(-1), np.abs(t).reshape(-1), np.abs(np.asarray(x, dtype=np.float64)).reshape(-1)])
    top = np.sort(e, axis=2)
    lead = float((top[:, :, -1] - top[:, :, -2]).min()) if e.shape[2] > 1 else np.inf
    return float(kinks[kinks > 0].min()), lead, spread
