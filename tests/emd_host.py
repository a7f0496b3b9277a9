"""NumPy float32 restatement of the auction EMD contract (include/houv_hip.h `houv_emd_forward`): the same
expression order, the same tie rules (bid: lowest j among equal values; award: largest increment, then lowest i) and the same
forced last step.  Shared by test_emd_host.py (CPU) and test_gpu_emd.py (bit equality with the HIP kernels)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_F = np.float32
_THREADS = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(_THREADS)
    return _POOL


def _bid_rows(x1, x2, price, u, eps):
    """(j*, inc) of the bidders u against all objects: one [len(u), N] fp32 matrix, every step rounded to fp32 in the
    contract's order (in place, to spare the temporaries)."""
    N = x2.shape[0]
    v = x2[None, :, 0] - x1[u, None, 0]
    v *= v
    w = x2[None, :, 1] - x1[u, None, 1]
    w *= w
    v += w                                                         # dx*dx + dy*dy
    np.subtract(x2[None, :, 2], x1[u, None, 2], out=w)
    w *= w
    v += w                                                         # (dx*dx + dy*dy) + dz*dz
    np.sqrt(v, out=v)
    np.subtract(_F(3.0), v, out=v)
    v -= price[None, :]
    j = np.argmax(v, axis=1)                                       # first occurrence: lowest j on ties
    rows = np.arange(len(u))
    best = v[rows, j]
    if N == 1:
        second = best
    else:
        v[rows, j] = -np.inf
        second = v.max(axis=1)
    return j, (best - second) + _F(eps)


def _bid(x1, x2, price, U, eps, chunk=128):
    """(j*, inc) of every bidder in U against all objects, in row chunks to bound the temporaries; the chunks are independent
    and NumPy releases the interpreter lock inside its loops, so large calls spread them over a few threads."""
    js = np.empty(len(U), dtype=np.int64)
    incs = np.empty(len(U), dtype=_F)
    starts = range(0, len(U), chunk)

    def one(c0):
        js[c0:c0 + chunk], incs[c0:c0 + chunk] = _bid_rows(x1, x2, price, U[c0:c0 + chunk], eps)

    if len(U) * x2.shape[0] < (1 << 21) or _THREADS < 2:
        for c0 in starts:
            one(c0)
    else:
        list(_pool().map(one, starts))
    return js, incs


def emd_cloud(x1, x2, eps, iters, trace=None):
    """One cloud: x1[N,3], x2[N,3] float32 -> (dist[N] float32, assignment[N] int32, iterations run).  ``trace``: a list that
    receives |U| of every iteration that bids (what selects the kernels' bid branch: emd_cases.bid_shape)."""
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
        if trace is not None:
            trace.append(len(U))
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


def emd(xyz1, xyz2, eps, iters, trace=None):
    """Batched: xyz1[B,N,3], xyz2[B,N,3] -> (dist[B,N], assignment[B,N], iters_run[B]).  ``trace``: a list that receives one
    |U| list per cloud."""
    out = []
    for a, b in zip(np.asarray(xyz1), np.asarray(xyz2)):
        tr = None
        if trace is not None:
            tr = []
            trace.append(tr)
        out.append(emd_cloud(a, b, eps, iters, tr))
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))


def emd_backward(x1, x2, graddist, assignment, into=None):
    """fp32 restatement of houv_emd_backward: x1[B,N,3], x2[B,N,3], graddist[B,N], assignment[B,N] ->
    g = graddist * 2; out += g * (x1 - x2[assignment]), accumulated into ``into`` (changed in place and returned) or zeros."""
    x1 = np.ascontiguousarray(x1, dtype=_F)
    x2 = np.ascontiguousarray(x2, dtype=_F)
    B, N, _ = x1.shape
    out = np.zeros((B, N, 3), dtype=_F) if into is None else into
    assert out.dtype == _F and out.shape == (B, N, 3)
    g = np.asarray(graddist, dtype=_F).reshape(B, N) * _F(2.0)
    y = np.take_along_axis(x2, np.asarray(assignment).reshape(B, N, 1).astype(np.int64), axis=1)
    out += g[:, :, None] * (x1 - y)
    return out
