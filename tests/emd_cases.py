"""Clouds and case tables of the auction-EMD parity tests, shared by test_emd_host.py (CPU: the tables reach every bid branch,
shown with the restatement alone) and test_gpu_emd.py (GPU: the kernels give the restatement's bits on those tables)."""
import torch


def clouds(B, N, seed, kind="rand"):
    """(x1, x2) float32 [B,N,3] on the CPU.  Every kind but ``rand`` forces ties or a crowded object."""
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand((B, N, 3), generator=g)
    x2 = torch.rand((B, N, 3), generator=g)
    if kind == "grid":                              # coarse grid: equal distances, equal values and equal increments
        x1 = torch.round(x1 * 4) / 4
        x2 = torch.round(x2 * 4) / 4
    elif kind == "dup":                             # duplicated targets: equal values for distinct objects
        x2[:, 1::2] = x2[:, 0:N - 1:2] if N > 1 else x2[:, 1::2]
    elif kind == "dupbid":                          # duplicated bidders: equal increments for one object, the lowest i wins
        x1[:, 1::2] = x1[:, 0:N - 1:2]
    elif kind == "lastobj":                         # half of the bidders crowd round the last object
        x1[:, ::2] = x2[:, N - 1:N] + 0.01 * (x1[:, ::2] - 0.5)
    elif kind == "identity":                        # every bidder takes itself at t = 0
        x2 = x1.clone()
    else:
        assert kind == "rand", kind
    return x1, x2


# Mirrors emd_bid and the dispatch just before its call (houv_amd/csrc/emd.hip); must follow them when the dispatch changes.
EMD_BLOCK = 1024
EMD_TILE = 4096


def bid_shape(cnt):
    """(bidders per lane P, lanes per bidder G, passes of the ``base`` loop) of the bid phase for cnt unassigned bidders."""
    assert cnt >= 1
    P = 4 if cnt > EMD_BLOCK else 1
    q = max(1, (EMD_BLOCK * P) // cnt)
    lg = min(6, q.bit_length() - 1)
    cap = (EMD_BLOCK >> lg) * P
    return P, 1 << lg, -(-cnt // cap)


REACHABLE_LDS = frozenset([(4, 1, 1), (4, 2, 1), (1, 1, 1), (1, 2, 1), (1, 4, 1), (1, 8, 1), (1, 16, 1), (1, 32, 1), (1, 64, 1)])
REACHABLE_STREAM = REACHABLE_LDS | frozenset([(4, 1, 2), (4, 1, 3), (4, 1, 4)])


def lds_clouds(case):
    """The clouds of one row of LDS_CASES."""
    N, iters, eps, B, kind = case
    return clouds(B, N, seed=N * 100 + iters, kind=kind)


def stream_clouds(case):
    """The clouds of one row of STREAM_CASES (or STREAM_MAX)."""
    N, iters, eps, B, kind = case
    return clouds(B, N, seed=N + iters, kind=kind)


# In-LDS kernel (N <= 4096): (N, iters, eps, B, kind)
LDS_CASES = []
for n_i, N in enumerate([1, 2, 63, 64, 257, 1000, 2048, 4096]):
    for k_i, iters in enumerate([1, 2, 7, 50]):
        LDS_CASES.append((N, iters, (0.005, 0.05)[(n_i + k_i) % 2], 2 + (n_i + k_i) % 3 if N < 2048 else 2,
                          ("rand", "grid", "dup")[(n_i + 2 * k_i) % 3]))
LDS_CASES += [
    # the compaction loop's second trip of one lane (1025), its last full trip (1024), one lane short (1023), and a stride
    # that differs from N at the top size (4095: emd_stride = 4096)
    (1023, 12, 0.05, 2, "rand"),
    (1024, 12, 0.005, 2, "grid"),
    (1025, 12, 0.05, 2, "dup"),
    (4095, 6, 0.05, 1, "rand"),
    # duplicated bidders: equal increments for one object
    (2, 5, 0.005, 3, "dupbid"),
    (257, 40, 0.005, 2, "dupbid"),
    (1025, 12, 0.05, 2, "dupbid"),
    (2048, 7, 0.005, 1, "dupbid"),
    # eps extremes on grid clouds: with 1e-10 the ties never resolve (|U| stalls) and the forced last step decides
    (257, 20, 1e-10, 2, "grid"),
    (257, 20, 10.0, 2, "grid"),
]

# Streamed kernel (4097..16384): same columns.  The first four are the cases from before the branch table was drawn up: they
# reach (4,1,2), (4,1,1) and (4,2,1) only.
STREAM_CASES_OLD = [(4097, 1, 0.05, 1, "rand"), (4097, 3, 0.05, 1, "grid"), (8192, 2, 0.05, 1, "dup"), (8192, 3, 0.05, 1, "rand")]
STREAM_COMPLETE = (4097, 5000, 1.0, 1, "rand")                # runs to completion: the whole P = 1 tail
STREAM_LASTOBJ3 = (8193, 6, 0.05, 1, "lastobj")               # three bid passes, an object tile of length 1
STREAM_LASTOBJ4 = (12289, 3, 0.05, 1, "lastobj")              # four bid passes, the last of one bidder
STREAM_DUPBID = (4099, 150, 0.05, 1, "dupbid")                # equal-increment ties in the tile-wise award
# duplicated objects down the whole P = 1 tail: every bidder's best and second are equal, so every merge of two lanes'
# partial results is decided by the lowest-j rule (random clouds never tie there)
STREAM_TIES = (4098, 400, 1.0, 1, "dup")
STREAM_CASES_NEW = [STREAM_COMPLETE, STREAM_LASTOBJ3, STREAM_LASTOBJ4, STREAM_DUPBID, STREAM_TIES]
STREAM_CASES = STREAM_CASES_OLD + STREAM_CASES_NEW
STREAM_MAX = (16384, 2, 0.05, 1, "rand")                      # the contract's maximum: 16-bit index packing at its limit

# Streamed batch with three different iters_run: N % 4 != 0, so the per-cloud workspace slices are no multiples of N.
BATCH_N, BATCH_ITERS, BATCH_EPS = 4099, 30, 1.0
BATCH_KINDS = (("identity", 1), ("rand", 2), ("grid", 3))     # (kind, seed) of clouds 0, 1, 2


def batch_clouds(order=(0, 1, 2)):
    parts = [clouds(1, BATCH_N, seed=BATCH_KINDS[c][1], kind=BATCH_KINDS[c][0]) for c in order]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
