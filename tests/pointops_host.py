"""Host restatements of the point-op contracts of include/houv_hip.h (houv_furthest_point_sample, houv_knn_cross through
tests/hostmath, houv_ball_query, houv_three_interpolate, houv_scatter_points_grad) in NumPy fp32, the input families of the
FPS / k-NN tests, and the model_utils_completion helpers in torch, fed index tensors from outside.
NumPy evaluates fp32 array expressions operation by operation in fp32 (no contraction, no wider intermediates), so the
expression trees below are the kernels'."""
import ctypes
import functools
import math

import numpy as np
import torch

F = np.float32


def fps(points, npoint, dtype=F):
    """points (N,3) -> (npoint,) int32: houv_furthest_point_sample's contract for one cloud.  Every running minimum starts at
    1e10, the first pick is point 0, then npoint-1 times: d = (dx*dx + dy*dy) + dz*dz to the last pick, md = min(md, d), pick =
    the arg-max of md with the LOWEST index among equals (np.argmax returns the first).  Once every md is 0 (more picks than
    distinct points) that is index 0, again and again.  dtype float64 is the yardstick of the CPU test."""
    p = np.asarray(points, dtype=dtype)
    md = np.full(len(p), 1e10, dtype)
    out = [0]
    for _ in range(1, npoint):
        q = p[out[-1]]
        dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == dtype
        md = np.minimum(md, d)
        out.append(int(np.argmax(md)))
    return np.array(out, np.int32)


def lattice(rng, *shape):
    """Points on the 1/8 lattice of [0,1)^3 (512 sites): every difference, square and sum of squares is a multiple of 1/64
    below 3, exact in fp32 whatever the order or contraction."""
    return (rng.integers(0, 8, shape + (3,)) / 8.0).astype(F)


@functools.lru_cache(maxsize=None)
def fps_cloud(B, N, kind="random"):
    """(B,N,3) fp32, a different cloud per batch row.  Read-only: shared between tests."""
    rng = np.random.default_rng(1000 * N + B)
    x = lattice(rng, B, N) if kind == "lattice" else rng.random((B, N, 3), dtype=F)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def fps_expected(B, N, npoint, kind="random"):
    x = fps_cloud(B, N, kind)
    out = np.stack([fps(x[b], npoint) for b in range(B)])
    out.setflags(write=False)
    return out


def knn_cross(query, ref, k):
    """(idx[B,N,k] int32, dist2[B,N,k] fp32) of hm_knn_cross_fmaf: per query the k smallest (distance, index) pairs of ref in
    lexicographic order, distance = fmaf(dz, dz, fmaf(dy, dy, dx*dx)) with d = ref - query (metric_sqdist<0>)."""
    import hostmath
    hm = hostmath.load()
    q = np.ascontiguousarray(query, dtype=F)
    r = np.ascontiguousarray(ref, dtype=F)
    B, N, _ = q.shape
    M = r.shape[1]
    assert r.shape[0] == B and 1 <= k <= M
    idx = np.zeros((B, N, k), np.int32)
    dist = np.zeros((B, N, k), F)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    hm.hm_knn_cross_fmaf(q.ctypes.data_as(fp), r.ctypes.data_as(fp), B, N, M, k, idx.ctypes.data_as(ip), dist.ctypes.data_as(fp))
    return idx, dist


KNN_FAMILIES = ("random", "repeat", "identical", "copies", "lattice", "descending")


@functools.lru_cache(maxsize=None)
def knn_inputs(family, B, N, M):
    """(query[B,N,3], ref[B,M,3]) fp32, read-only.
    random      uniform, tie-free
    repeat      the second half of ref repeats the first: every distance is tied once, the lower index comes first
    identical   ref is M copies of one point: the list must be 0 .. k-1
    copies      every query is a point of ref (d = 0 heads its list)
    lattice     both clouds on the 1/8 lattice: exact distances, hundreds of ties per list
    descending  ref sorted by DEcreasing distance from the origin, queries within 0.05 of it: nearly every reference is a new
                best, so every reference passes the stale threshold and the queues flush at their maximum rate"""
    rng = np.random.default_rng([KNN_FAMILIES.index(family), B, N, M])
    q = rng.random((B, N, 3), dtype=F)
    r = rng.random((B, M, 3), dtype=F)
    if family == "repeat":
        h = M // 2
        if h:
            r[:, M - h:] = r[:, :h]
    elif family == "identical":
        r[:] = r[:, :1]
    elif family == "copies":
        pick = rng.integers(0, M, (B, N))
        q = np.take_along_axis(r, pick[..., None], axis=1)
    elif family == "lattice":
        q, r = lattice(rng, B, N), lattice(rng, B, M)
    elif family == "descending":
        order = np.argsort(-(r.astype(np.float64) ** 2).sum(-1), axis=1, kind="stable")
        r = np.take_along_axis(r, order[..., None], axis=1)
        q = (q * F(0.05) / F(np.sqrt(3.0))).astype(F)
    q, r = np.ascontiguousarray(q, dtype=F), np.ascontiguousarray(r, dtype=F)
    q.setflags(write=False)
    r.setflags(write=False)
    return q, r


@functools.lru_cache(maxsize=None)
def knn_expected(family, B, N, M, k):
    """The k-list as a prefix of ONE host list per input (depth min(M, 32)): a prefix of a lexicographically sorted list is the
    sorted shorter list."""
    depth = min(M, 32)
    if k != depth:
        idx, dist = knn_expected(family, B, N, M, depth)
        return idx[..., :k], dist[..., :k]
    idx, dist = knn_cross(*knn_inputs(family, B, N, M), k)
    idx.setflags(write=False)
    dist.setflags(write=False)
    return idx, dist


def ball_query(xyz, center, min_radius, max_radius, nsample):
    """xyz (B,N,3), center (B,Mc,3) fp32 -> idx (B,Mc,nsample) int32, cnt (B,Mc) int32."""
    xyz, center = np.asarray(xyz, F), np.asarray(center, F)
    B, N, _ = xyz.shape
    Mc = center.shape[1]
    min2, max2 = F(min_radius) * F(min_radius), F(max_radius) * F(max_radius)
    idx = np.zeros((B, Mc, nsample), np.int32)
    cnt = np.zeros((B, Mc), np.int32)
    for b in range(B):
        x, y, z = xyz[b, :, 0][None], xyz[b, :, 1][None], xyz[b, :, 2][None]
        cx, cy, cz = center[b, :, 0][:, None], center[b, :, 1][:, None], center[b, :, 2][:, None]
        d2 = ((cx - x) * (cx - x) + (cy - y) * (cy - y)) + (cz - z) * (cz - z)
        assert d2.dtype == F
        hit = (d2 == 0) | ((d2 >= min2) & (d2 < max2))
        for c in range(Mc):
            hits = np.flatnonzero(hit[c])[:nsample]          # ascending index
            cnt[b, c] = len(hits)
            if len(hits):
                idx[b, c, :] = hits[0]
                idx[b, c, :len(hits)] = hits
    return idx, cnt


def three_interpolate(features, idx, weight):
    """features (B,C,M), idx (B,N,3), weight (B,N,3) -> (B,C,N) = (w0*f0 + w1*f1) + w2*f2."""
    features, weight = np.asarray(features, F), np.asarray(weight, F)
    idx = np.asarray(idx, np.int64)
    B, C, M = features.shape
    out = np.empty((B, C, idx.shape[1]), F)
    for b in range(B):
        f = [features[b][:, idx[b, :, j]] for j in range(3)]
        w = [weight[b, :, j][None] for j in range(3)]
        out[b] = (w[0] * f[0] + w[1] * f[1]) + w[2] * f[2]
    assert out.dtype == F
    return out


def scatter_points_grad(grad_out, idx, weight, N, S):
    """grad_out (B,C,M/S), idx (B,M), weight (B,M) or None -> (B,C,N): per destination the fp32 sum of grad_out[.., m/S] * weight[m]
    over m ascending, sequential, starting from the first term.  np.add.at is unbuffered and walks the indices in order, which
    is that loop started from +0 instead of from the first term: the two differ only where a sum of -0 terms is -0, which the
    explicit first-term pass restores."""
    grad_out = np.asarray(grad_out, F)
    idx = np.asarray(idx, np.int64)
    B, C, _ = grad_out.shape
    M = idx.shape[1]
    out = np.zeros((B, C, N), F)
    for b in range(B):
        terms = grad_out[b][:, np.arange(M) // S]                           # (C,M)
        if weight is not None:
            terms = terms * np.asarray(weight, F)[b][None]
        assert terms.dtype == F
        firsts = np.full(N, M, np.int64)
        np.minimum.at(firsts, idx[b], np.arange(M))                         # lowest m of each destination
        has = firsts < M
        rest = np.ones(M, bool)
        rest[firsts[has]] = False
        out[b][:, has] = terms[:, firsts[has]]
        tt = np.ascontiguousarray(terms[:, rest].T)                         # (M',C): np.add.at adds row by row, in order
        acc = np.ascontiguousarray(out[b].T)                                # (N,C)
        np.add.at(acc, idx[b][rest], tt)
        out[b] = acc.T
    return out


def scatter_points_grad_loop(grad_out, idx, weight, N, S):
    """The same contract as a plain Python loop over m (small cases: pins the np.add.at form above)."""
    grad_out = np.asarray(grad_out, F)
    B, C, _ = grad_out.shape
    M = idx.shape[1]
    out = np.zeros((B, C, N), F)
    for b in range(B):
        seen = np.zeros(N, bool)
        for m in range(M):
            k = int(idx[b, m])
            t = grad_out[b, :, m // S]
            if weight is not None:
                t = t * F(weight[b, m])
            out[b, :, k] = out[b, :, k] + t if seen[k] else t
            seen[k] = True
    return out


# ---- the helpers of houv_amd.model_utils_completion in plain torch, fed the index tensors the GPU ops chose ---------------
def _take(features, idx):
    """features (B,C,N), idx (B,...) -> (B,C,...)"""
    B, C, _ = features.shape
    flat = idx.reshape(B, 1, -1).expand(-1, C, -1).long()
    return torch.gather(features, 2, flat).view(B, C, *idx.shape[1:])


def edge_preserve_sampling(feature_input, point_input, p_idx, pn_idx):
    point_output = _take(point_input.transpose(1, 2), p_idx).transpose(1, 2)
    neighbour = _take(feature_input, pn_idx).max(dim=3).values
    return torch.cat((_take(feature_input, p_idx), neighbour), 1), point_output


def get_repulsion_loss(pred, idx, radius=0.07):
    flipped = pred.transpose(1, 2)
    off = _take(flipped, idx) - flipped.unsqueeze(-1)
    d2 = (off ** 2).sum(1)
    d2 = -torch.topk(-d2, 5).values[:, :, 1:]
    d2 = torch.clamp(d2, min=1e-12)
    return torch.mean(radius - torch.sqrt(d2) * torch.exp(-d2 / 0.03 ** 2))


def get_uniform_loss(pcd, fps_idx, ball_idx, percentages=(0.004, 0.006, 0.008, 0.010, 0.012), radius=1.0):
    """ball_idx: one (B,npoint,nsample) tensor per percentage.  Inside a ball the distance to the nearest OTHER slot comes from
    the expanded-form pairwise matrix the reference ranks (second largest of -d2)."""
    B, N, _ = pcd.shape
    loss = 0
    for p, idx in zip(percentages, ball_idx):
        nsample = int(N * p)
        expect = math.sqrt(math.pi * radius ** 2 * p / nsample)
        g = _take(pcd.transpose(1, 2), idx).permute(0, 2, 3, 1).reshape(-1, nsample, 3)
        d2 = ((g.unsqueeze(2) - g.unsqueeze(1)) ** 2).sum(-1)
        var = torch.topk(-d2, 2, dim=-1).values
        d = torch.sqrt(torch.abs(-var[:, :, 1:] + 1e-8)).mean(-1)
        loss = loss + torch.mean((d - expect) ** 2 / (expect + 1e-8)) * (p * 100) ** 2
    return loss / len(percentages)


def symmetric_sample(points, idx):
    kept = _take(points.transpose(1, 2), idx).transpose(1, 2)
    flip = torch.stack([kept[..., 0], kept[..., 1], -kept[..., 2]], dim=2)
    return torch.cat([kept, flip], 1)


def three_nn_weights(dist):
    inv = 1.0 / torch.clamp(dist, min=1e-10)
    return inv / inv.sum(2, keepdim=True)
