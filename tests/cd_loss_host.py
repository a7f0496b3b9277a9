"""Host restatement of the completion Chamfer loss node (houv_cd_loss_backward) in numpy, in float32 or
float64, in the kernel's own summation order: per output row the own term, then its list (the ground-truth points that chose
it, ascending) -- one entry after the other up to LONG entries, otherwise 64 strided partial sums started at -0 and the xor
butterfly 32, 16, 8, 4, 2, 1.  `fault` plants one of FAULTS, for the tests that show each of them changes the result."""
import numpy as np

LONG = 32            # kCdLong of cd_loss.hip: a list longer than this takes the wave path
WAVE = 64
FAULTS = ("inverse_from_idx2", "n_m_swapped", "no_own_term", "factor_2")


def nearest(a, b):
    """a[B,n,3], b[B,m,3] -> (squared distance [B,n], index [B,n]) of each a's nearest b in float64, the lower index on a tie."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)
    idx = d.argmin(-1)
    return np.take_along_axis(d, idx[..., None], -1)[..., 0], idx.astype(np.int32)


def margins(a, b):
    """The smallest gap, over the points of a, between the distances to the nearest and the second nearest point of b."""
    d = np.sqrt(((np.asarray(a, np.float64)[:, :, None, :] - np.asarray(b, np.float64)[:, None, :, :]) ** 2).sum(-1))
    if d.shape[2] < 2:
        return np.inf
    s = np.sort(d, -1)
    return float((s[..., 1] - s[..., 0]).min())


def loss(out, gt, dtype=np.float64):
    """calc_cd's (cd_p[B], cd_t[B]) with the nearest neighbours searched."""
    d1, _ = nearest(gt, out)
    d2, _ = nearest(out, gt)
    d1, d2 = d1.astype(dtype), d2.astype(dtype)
    return (np.sqrt(d1).mean(1) + np.sqrt(d2).mean(1)) / dtype(2), d1.mean(1) + d2.mean(1)


def _butterfly(v):
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v


def backward(out, gt, dist1, dist2, idx1, idx2, g_p, g_t, dtype=np.float64, fault=None, want_mag=False):
    """gout[B,M,3] in `dtype`; with want_mag also, per row, the sum of its terms' magnitudes and its list's length."""
    assert fault is None or fault in FAULTS
    f = dtype
    out, gt, dist1, dist2 = (np.asarray(t).astype(f) for t in (out, gt, dist1, dist2))
    g_p, g_t = np.asarray(g_p).astype(f).reshape(-1), np.asarray(g_t).astype(f).reshape(-1)
    B, M, _ = out.shape
    N = gt.shape[1]
    n1, n2 = (M, N) if fault == "n_m_swapped" else (N, M)
    four = f(2) if fault == "factor_2" else f(4)
    keys = np.clip(np.asarray(idx2 if fault == "inverse_from_idx2" else idx1), 0, M - 1)
    own = np.clip(np.asarray(idx2), 0, N - 1)
    gout = np.empty((B, M, 3), f)
    mag, length = np.zeros((B, M)), np.zeros((B, M), np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            a_t1, a_p1 = g_t[b] / f(n1), g_p[b] / (four * f(n1))
            a_t2, a_p2 = g_t[b] / f(n2), g_p[b] / (four * f(n2))
            s2 = f(2) * (a_t2 + a_p2 / np.sqrt(dist2[b]))
            first = s2[:, None] * (out[b] - gt[b, own[b]])
            for j in range(M):
                lst = np.clip(np.nonzero(keys[b] == j)[0], 0, N - 1)
                s1 = f(2) * (a_t1 + a_p1 / np.sqrt(dist1[b, lst]))
                terms = s1[:, None] * (out[b, j][None, :] - gt[b, lst])
                acc = np.zeros(3, f) if fault == "no_own_term" else first[j].copy()
                if len(lst) <= LONG:
                    for t in terms:
                        acc = acc + t
                else:
                    part = np.full((WAVE, 3), -0.0, f)
                    for n, t in enumerate(terms):
                        part[n % WAVE] = part[n % WAVE] + t
                    acc = acc + _butterfly(part)[0]
                gout[b, j] = acc
                # the terms' magnitudes with |g_t| and |g_p| in the weights: what the float32 rounding of a row scales with when the
                # two shares of a weight cancel
                m1 = f(2) * (abs(a_t1) + abs(a_p1) / np.sqrt(dist1[b, lst]))
                m2 = f(2) * (abs(a_t2) + abs(a_p2) / np.sqrt(dist2[b, j]))
                mag[b, j] = (m2 * np.abs(out[b, j] - gt[b, own[b, j]])).max() + (m1[:, None] * np.abs(out[b, j][None, :] - gt[b, lst])).sum(0).max(initial=0.0)
                length[b, j] = len(lst)
    return (gout, mag, length) if want_mag else gout


def composition_grad(out, gt, idx1, idx2, g_p, g_t):
    """torch autograd (CPU, float64) of the gather-based composition with the indices given: sqrt and mean over
    ((out[idx] - gt) ** 2).sum(-1)."""
    import torch
    o = torch.tensor(np.asarray(out, np.float64), requires_grad=True)
    g = torch.tensor(np.asarray(gt, np.float64))
    i1, i2 = torch.tensor(np.asarray(idx1)).long(), torch.tensor(np.asarray(idx2)).long()
    d1 = ((torch.gather(o, 1, i1[..., None].expand(-1, -1, 3)) - g) ** 2).sum(-1)
    d2 = ((o - torch.gather(g, 1, i2[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    cd_p = (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2
    cd_t = d1.mean(1) + d2.mean(1)
    ((cd_p * torch.tensor(np.asarray(g_p, np.float64))).sum() + (cd_t * torch.tensor(np.asarray(g_t, np.float64))).sum()).backward()
    return o.grad.numpy(), d1.detach().numpy(), d2.detach().numpy()
