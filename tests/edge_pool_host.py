"""A sequential NumPy restatement of houv_edge_pool and houv_edge_pool_backward (include/houv_hip.h), the
contract the device kernels are held to bit for bit: the forward's running maximum with its tie and NaN rules, and the backward
as the literal loop in the stated order.  `dtype` float32 gives the device's arithmetic, float64 the reference for the
module-level tests."""
import numpy as np


def clamp(idx, N):
    return np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)


def forward(feat, p_idx, pn_idx, highest_slot=False):
    """feat [B,N,C], p_idx [B,S], pn_idx [B,S,pk] -> (out [B,S,2C], arg int8 [B,S,C]).  highest_slot plants a fault: a tied
    maximum goes to its last slot."""
    B, N, C = feat.shape
    S, pk = pn_idx.shape[1:]
    p, pn = clamp(p_idx, N), clamp(pn_idx, N)
    out = np.empty((B, S, 2 * C), dtype=feat.dtype)
    arg = np.full((B, S, C), -1, dtype=np.int8)
    for b in range(B):
        out[b, :, :C] = feat[b, p[b]]
        best = np.full((S, C), np.nan, dtype=feat.dtype)
        for j in range(pk):
            v = feat[b, pn[b, :, j]]                                     # (S,C)
            with np.errstate(invalid="ignore"):
                # a NaN never enters; a later slot only when strictly greater
                enters = ~np.isnan(v) & ((arg[b] < 0) | ((v >= best) if highest_slot else (v > best)))
            best = np.where(enters, v, best)
            arg[b] = np.where(enters, j, arg[b])
        out[b, :, C:] = best
    return out, arg


def backward(g, p_idx, pn_idx, arg, N, drop_centre=False, unclamped=False):
    """g [B,S,2C] -> gfeat [B,N,C] in g's dtype: per (b, n, c) the terms are added one after the other, starting from the first,
    in ascending s, the centre before the neighbours, j ascending; 0 where nothing lands.  The two flags plant faults (the
    host tests show that each changes the result)."""
    B, S, C2 = g.shape
    C, pk = C2 // 2, pn_idx.shape[2]
    fix = (lambda i: np.asarray(i, dtype=np.int64)) if unclamped else (lambda i: clamp(i, N))
    p, pn = fix(p_idx), fix(pn_idx)
    gfeat = np.zeros((B, N, C), dtype=g.dtype)
    landed = np.zeros((B, N, C), dtype=bool)

    def add(b, n, cols, vals):
        if not 0 <= n < N:
            return
        first = cols & ~landed[b, n]
        gfeat[b, n, first] = vals[first]                                 # the first term is taken as it is (its bits, a -0 included)
        later = cols & landed[b, n]
        gfeat[b, n, later] = gfeat[b, n, later] + vals[later]
        landed[b, n] |= cols

    for b in range(B):
        for s in range(S):
            if not drop_centre:
                add(b, int(p[b, s]), np.ones(C, dtype=bool), g[b, s, :C])
            a = arg[b, s].astype(np.int64)
            for j in range(pk):
                add(b, int(pn[b, s, j]), a == j, g[b, s, C:])
    return gfeat
