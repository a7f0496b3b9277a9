"""Host restatements of the DCP feature-head blocks of include/houv_hip.h (houv_knn, houv_edgeconv1, houv_layernorm,
houv_softmax_rows, houv_softmax_corr), the seeded inputs tests/test_gpu_dcp_ops.py feeds the kernels, and the error measures it
holds them to.  Two kinds of restatement:

* exact, where the contract is exact: k-NN lists through tests/hostmath (std::fmaf, the distance of metric_sqdist<0>);
* float64, written from the formulas of the reference's dcp.py that the kernel comments cite; and next to each the SAME formula
  composed from fp32 torch operations on the CPU, whose error against float64 is the yardstick a kernel's error is held to
  (`margin`): a kernel is never bounded by its own output.

Nothing here imports houv_amd."""
import ctypes
import functools
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24           # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------------
# k-NN
# ---------------------------------------------------------------------------------------------------------------------
KNN_K = (1, 3, 8, 16, 20)
KNN_N = (63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048, 2050, 4100)     # and N = k for every k
KNN_B = 2
KNN_DUP_N = (513, 2050, 4100)          # clouds with planted duplicates: a split boundary case, two and four 1024-stages
KNN_DUP_COPIES = 40


def knn_sizes(k):
    return tuple(sorted({k} | {n for n in KNN_N if n >= k}))


def knn_cloud(N):
    """[KNN_B, N, 3] fp32 uniform in [0, 1): every batch entry its own cloud.  The seed depends on N alone, so the lists of a
    smaller k are prefixes of those of a larger one.  Among a few thousand fp32 distances per query two of the 21 smallest now
    and then coincide exactly: tests/test_dcp_ops_host.py asserts that these seeds have no such tie."""
    gen = torch.Generator().manual_seed(7919 * N)
    return torch.rand(KNN_B, N, 3, generator=gen)


def knn_dup_groups(N):
    """(source start, copy start) of the planted duplicates: copies lie two quarters of the split kernel (ceil(N / 4) references
    each) and, from 2050 points on, two 1024-stages of the single-scan kernel away from their sources."""
    return ((0, int(N * 0.55)), (int(N * 0.3), int(N * 0.9)))


def knn_dup_cloud(N):
    x = knn_cloud(N).clone()
    for src, dst in knn_dup_groups(N):
        x[:, dst:dst + KNN_DUP_COPIES] = x[:, src:src + KNN_DUP_COPIES]
    return x


def knn_host(xyz, k):
    """(idx[B,N,k] int64, dist[B,N,k] fp32): the (distance, index)-lexicographic k smallest per query, distances as
    fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32 (hm_knn_fmaf)."""
    import hostmath
    hm = hostmath.load()
    x = np.ascontiguousarray(xyz.numpy() if isinstance(xyz, torch.Tensor) else xyz, dtype=np.float32)
    B, N, _ = x.shape
    assert 1 <= k <= N
    idx = np.zeros((B, N, k), np.int32)
    dist = np.zeros((B, N, k), np.float32)
    hm.hm_knn_fmaf(x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), B, N, k, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                   dist.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return torch.from_numpy(idx).long(), torch.from_numpy(dist)


@functools.lru_cache(maxsize=None)
def knn_lists(N, dup=False):
    """Host lists of the test cloud of N points to depth min(N, 21): one more than the largest k, so the CPU test can see that the
    (k+1)-th distance differs from the k-th."""
    return knn_host(knn_dup_cloud(N) if dup else knn_cloud(N), min(N, max(KNN_K) + 1))


def knn_float64(xyz, k):
    """dcp.py:35-42 in float64: -|xi|^2 + 2 xi.xj - |xj|^2, the k largest."""
    xd = xyz.double().transpose(1, 2)
    inner = 2 * xd.transpose(2, 1) @ xd
    xx = (xd ** 2).sum(1, keepdim=True)
    return (-xx.transpose(2, 1) + inner - xx).topk(k=k, dim=-1)[1]


# ---------------------------------------------------------------------------------------------------------------------
# edgeconv1: relu(scale * (W . cat(neighbour, centre)) + shift)     dcp.py:44-66, :272, :277, :285-286
# ---------------------------------------------------------------------------------------------------------------------
EDGECONV_CASES = ((1, 1, 1), (2, 37, 5), (3, 300, 20), (8, 2048, 20), (1, 17000, 16))


def edgeconv_inputs(B, N, k):
    """xyz[B,N,3], random idx[B,N,k] in [0, N) (used where houv_knn has no k), W[64,6], scale[64], shift[64]."""
    gen = torch.Generator().manual_seed(B * 100003 + N * 17 + k)
    xyz = torch.rand(B, N, 3, generator=gen) * 2 - 1
    idx = torch.randint(0, N, (B, N, k), generator=gen, dtype=torch.int32)
    W = torch.randn(64, 6, generator=gen)
    scale = torch.randn(64, generator=gen)
    shift = torch.randn(64, generator=gen) * 0.5
    return xyz, idx, W, scale, shift


def edge_features(xyz, idx):
    """f[B*N*k, 6] = cat(neighbour, centre) (dcp.py:64: `torch.cat((feature, x), dim=3)`), in xyz's dtype."""
    B, N, k = idx.shape
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    flat = (idx.long() + torch.arange(B).view(B, 1, 1) * N).reshape(-1)       # neighbours stay inside their own cloud
    nb = xyz.reshape(B * N, 3)[flat].reshape(B, N, k, 3)
    ctr = xyz.unsqueeze(2).expand(B, N, k, 3)
    return torch.cat((nb, ctr), dim=3).reshape(B * N * k, 6)


def edgeconv1_ref(xyz, idx, W, scale, shift):
    """float64: (pre-activation, output, elementwise bound).  Bound: the kernel makes six fused multiply-adds, one multiply and
    one add per output, each rounding at most 2^-24 of a partial result no larger than scale_c * sum_t |f_t w_ct| + |shift_c|;
    ReLU is 1-Lipschitz; 1e-37 covers results flushed below the normal range."""
    f = edge_features(xyz.double(), idx)
    pre = (f @ W.double().t()) * scale.double() + shift.double()
    bound = 8 * EPS32 * ((f.abs() @ W.double().abs().t()) * scale.double().abs() + shift.double().abs()) + 1e-37
    return pre, torch.relu(pre), bound


def edgeconv1_f32(xyz, idx, W, scale, shift):
    """The same formula from fp32 torch operations."""
    return torch.relu((edge_features(xyz, idx) @ W.t()) * scale + shift)


# ---------------------------------------------------------------------------------------------------------------------
# the margin for the kernels whose error depends on the accumulation order
# ---------------------------------------------------------------------------------------------------------------------
def ulp32(mag):
    """One unit in the last place of fp32 at magnitude `mag`."""
    return float(np.spacing(np.float32(abs(float(mag))))) if mag else float(np.spacing(np.float32(0)))


def margin(err_composed, out_magnitude):
    """Admissible kernel error: 4x the error of the fp32 torch composition of the same formula on the same inputs, plus 2 ulp of
    the output magnitude (another summation tree, the device's expf against the host's exp)."""
    return 4.0 * err_composed + 2.0 * ulp32(out_magnitude)


def max_err(got, ref64):
    return float((got.double() - ref64).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# layernorm: a (x - mean) / (std_unbiased + eps) + b [+ r]        dcp.py:144-154
# ---------------------------------------------------------------------------------------------------------------------
LN_D = (4, 8, 64, 252, 256, 260, 512, 2048)
LN_ROWS = (1, 3, 4, 5, 37, 4099)
LN_VARIANTS = ("1e-3", "1", "1e3", "offset")
LN_EPS = 1e-6


def layernorm_inputs(D, rows, variant):
    """x[rows,D], a[D], b[D], r[rows,D].  `offset`: one row in four (the first always) has mean 1e3 and spread 1."""
    gen = torch.Generator().manual_seed(D * 10007 + rows * 13 + LN_VARIANTS.index(variant))
    x = torch.randn(rows, D, generator=gen)
    if variant == "offset":
        x[::4] += 1000.0
    else:
        x = x * float(variant)
    a = torch.rand(D, generator=gen) + 0.5
    b = torch.randn(D, generator=gen)
    r = torch.randn(rows, D, generator=gen)
    return x, a, b, r


def layernorm_ref(x, a, b, r=None, eps=LN_EPS):
    x, a, b = x.double(), a.double(), b.double()
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    std = (((x - mean) ** 2).sum(-1, keepdim=True) / (D - 1)).sqrt()       # torch.std: Bessel's correction
    out = a * (x - mean) / (std + eps) + b
    return out if r is None else out + r.double()


def layernorm_margin(x, a, err_composed, out_magnitude, eps=LN_EPS):
    """`margin` plus the one term it cannot carry: the rounding of the row mean.  A row with mean 1e3 and spread 1 has a condition
    number of 1e3: an error dm of the fp32 mean moves every output of the row by a * dm / (std + eps), and |dm| is up to an ulp
    of 1e3 whatever the summation order -- the composition's own dm is anywhere between 0 and that, so on a case with a single
    such row 4x its error says nothing (measured at D = 64, 3 rows: kernel 7.7e-5 = 1.3 ulp of 1e3, composition 3.9e-6).
    Derivation for the kernel's mean: a lane adds ceil(D / 256) four-element sums (two roundings each, then ceil(D / 256) - 1 for
    the running sum), the wave adds 64 lanes in six levels, one division by D: at most R = ceil(D / 256) + 8 roundings on the path
    to any element, each at most 2^-24 of a partial sum no larger than sum |x|, so |dm| <= R 2^-24 mean|x|.  For centred rows
    (mean|x| < std) the term is under a * R * 2^-24, a few ulp of the output."""
    xd = x.double()
    D = x.shape[-1]
    R = -(-D // 256) + 8
    mean = xd.sum(-1, keepdim=True) / D
    std = (((xd - mean) ** 2).sum(-1, keepdim=True) / (D - 1)).sqrt()
    dm = R * EPS32 * xd.abs().mean(-1, keepdim=True)
    return margin(err_composed, out_magnitude) + float((dm / (std + eps)).max() * a.double().abs().max())


def layernorm_f32(x, a, b, r=None, eps=LN_EPS):
    assert x.dtype == F32
    out = a * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + eps) + b
    return out if r is None else out + r


# ---------------------------------------------------------------------------------------------------------------------
# softmax over the last dimension        dcp.py:31
# ---------------------------------------------------------------------------------------------------------------------
SM_L = (1, 3, 4, 64, 77, 252, 256, 2048, 4092, 4096, 4100, 5000)
SM_ROWS = (1, 4, 5, 1000)
SM_VARIANTS = ("1", "10", "40", "special")


def softmax_inputs(L, rows, variant):
    """Logits [rows, L].  `special`: every third row holds -inf in about a third of its entries (never in column 0), the last
    row one entry that dominates all others by e^80."""
    gen = torch.Generator().manual_seed(L * 7 + rows * 1009 + SM_VARIANTS.index(variant))
    x = torch.randn(rows, L, generator=gen)
    if variant != "special":
        return x * float(variant)
    x = x * 4
    hole = torch.rand(rows, L, generator=gen) < 0.33
    hole[:, 0] = False
    hole[torch.arange(rows) % 3 != 0] = False
    x[hole] = -math.inf
    x[-1, L // 2] = 80.0
    return x


def softmax_ref(x):
    x = x.double()
    e = (x - x.max(-1, keepdim=True)[0]).exp()
    return e / e.sum(-1, keepdim=True)


def softmax_f32(x):
    assert x.dtype == F32
    e = (x - x.max(-1, keepdim=True)[0]).exp()
    return e / e.sum(-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------------
# softmax_corr: corr[p,c,n] = sum_m softmax(scores[p,n,:])[m] * pts[p,m,c]        dcp.py:346-348
# ---------------------------------------------------------------------------------------------------------------------
SC_CASES = ((1, 1, 1), (2, 3, 63), (3, 50, 77), (2, 257, 64), (1, 2048, 2048))
SC_VARIANTS = ("plain", "peaked")
SC_COORD_SCALE = (1.0, 10.0, 100.0)


def softmax_corr_inputs(P, N, M, variant):
    """scores[P,N,M] (peaked: the same rows times 10), pts[P,M,3] with a scale of its own per coordinate."""
    gen = torch.Generator().manual_seed(P * 31 + N * 1013 + M)
    scores = torch.randn(P, N, M, generator=gen) * 4
    pts = torch.randn(P, M, 3, generator=gen) * torch.tensor(SC_COORD_SCALE)
    return (scores * 10 if variant == "peaked" else scores), pts


def softmax_corr_ref(scores, pts):
    return torch.matmul(pts.double().transpose(1, 2), softmax_ref(scores).transpose(2, 1))


def softmax_corr_f32(scores, pts):
    return torch.matmul(pts.transpose(1, 2), softmax_f32(scores).transpose(2, 1))


def per_coordinate_err(got, ref64):
    """[3] max error of corr[P,3,N] per coordinate (their scales differ by 10x each)."""
    return (got.double() - ref64).abs().amax(dim=(0, 2))
