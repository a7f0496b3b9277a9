"""Host restatements of the point-op contracts of include/houv_hip.h (houv_ball_query, houv_three_interpolate,
houv_scatter_points_grad) in NumPy fp32, and of the model_utils_completion helpers in torch, fed index tensors from outside.
NumPy evaluates fp32 array expressions operation by operation in fp32 (no contraction, no wider intermediates), so the
expression trees below are the kernels'."""
import math

import numpy as np
import torch

F = np.float32


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
