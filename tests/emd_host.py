"""NumPy float32 restatement of the auction EMD contract (include/houv_hip.h `houv_emd_forward`): the same
expression order, the same tie rules (bid: lowest j among equal values; award: largest increment, then lowest i) and the same
forced last step.  Shared by test_emd_host.py (CPU) and test_gpu_emd.py (bit equality with the HIP kernels)."""
import numpy as np

_F = np.float32


def _bid(x1, x2, price, U, eps, chunk=512):
    """(j*, inc) of every bidder in U against all objects, in row chunks to bound the temporaries."""
    N = x2.shape[0]
    js = np.empty(len(U), dtype=np.int64)
    incs = np.empty(len(U), dtype=_F)
    for c0 in range(0, len(U), chunk):
        u = U[c0:c0 + chunk]
        dx = x2[None, :, 0] - x1[u, None, 0]
        dy = x2[None, :, 1] - x1[u, None, 1]
        dz = x2[None, :, 2] - x1[u, None, 2]
        v = (_F(3.0) - np.sqrt((dx * dx + dy * dy) + dz * dz)) - price[None, :]
        j = np.argmax(v, axis=1)                                   # first occurrence: lowest j on ties
        rows = np.arange(len(u))
        best = v[rows, j]
        if N == 1:
            second = best
        else:
            v[rows, j] = -np.inf
            second = v.max(axis=1)
        js[c0:c0 + chunk] = j
        incs[c0:c0 + chunk] = (best - second) + _F(eps)
    return js, incs


def emd_cloud(x1, x2, eps, iters):
    """One cloud: x1[N,3], x2[N,3] float32 -> (dist[N] float32, assignment[N] int32, iterations run)."""
    x1 = np.ascontiguousarray(x1, dtype=_F)
    x2 = np.ascontiguousarray(x2, dtype=_F)
    N = x1.shape[0]
    assert x2.shape[0] == N and N >= 1 and iters >= 1 and eps > 0
    price = np.zeros(N, dtype=_F)
    assign = np.full(N, -1, dtype=np.int64)
    owner = np.full(N, -1, dtype=np.int64)
    t = 0
    while t < iters:
        U = np.nonzero(assign == -1)[0]
        if len(U) == 0:
            break
        js, incs = _bid(x1, x2, price, U, eps)
        if t == iters - 1:
            assign[U] = js                                          # forced last step: no eviction
        else:
            order = np.lexsort((U, -incs, js))                      # by object, then largest inc, then lowest bidder
            js_o = js[order]
            first = np.ones(len(order), dtype=bool)
            first[1:] = js_o[1:] != js_o[:-1]
            win = order[first]
            wi, wj, winc = U[win], js[win], incs[win]
            old = owner[wj]
            assign[old[old >= 0]] = -1
            owner[wj] = wi
            assign[wi] = wj
            price[wj] = price[wj] + winc
        t += 1
    d = x1 - x2[assign]
    dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return dist.astype(_F), assign.astype(np.int32), t


def emd(xyz1, xyz2, eps, iters):
    """Batched: xyz1[B,N,3], xyz2[B,N,3] -> (dist[B,N], assignment[B,N], iters_run[B])."""
    out = [emd_cloud(a, b, eps, iters) for a, b in zip(np.asarray(xyz1), np.asarray(xyz2))]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))
