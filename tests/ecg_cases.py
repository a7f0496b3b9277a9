"""Shared inputs of the ECG tests (CPU and GPU): the golden cases of tests/golden/g26_ecg.npz, the feature clouds of the
houv_knn_feat tests with their host lists, and the Dense_conv cases.  Everything is computed once and handed out read-only."""
import functools
import os
import sys

import numpy as np

import ecg_host as host

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import ecg_weights  # noqa: E402

F = np.float32
GOLDEN_CASES = {"p512": (512, 512, 512), "p1280": (1280, 512, 512)}     # (num_points, num_coarse, num_input), B = 2
KNN_FAMILIES = ("random", "quarter", "identical")


def tau(C):
    """The relative bound on a feature-space comparison: every term of the chain d = fma(t, t, d) is non-negative, so the fp32
    value is within (C + 2) 2^-24 of the exact one to first order (one rounding of t, C of the chain, t*t exact inside the fma:
    (C + 2) covers 2 eps per term on the first and eps on the rest); a comparison of two such values doubles it, and a factor
    2 is kept for the second-order terms: tau = 4 (C + 3) 2^-24."""
    return 4 * (C + 3) * 2.0 ** -24


def scale_of(num_points, num_coarse, num_input):
    return int(np.ceil(num_points / (num_coarse + num_input)))


@functools.lru_cache(maxsize=None)
def state(name):
    num_points, num_coarse, num_input = GOLDEN_CASES[name]
    st = ecg_weights.make_state(num_coarse, scale_of(num_points, num_coarse, num_input))
    for v in st.values():
        v.setflags(write=False)
    return st


def reference_decisions(g, name):
    return {n: g[f"{name}_{n}"].astype(np.int64) for n in host.DECISIONS if f"{name}_{n}" in g.files}


def safe_mask(g, name, decision):
    shape = g[f"{name}_{decision}"].shape
    return np.unpackbits(g[f"{name}_{decision}_safe"])[:int(np.prod(shape))].reshape(shape).astype(bool)


@functools.lru_cache(maxsize=None)
def knn_cloud(family, B, N, C, ld):
    """x[B,N,ld] fp32 whose first C columns are the features (the rest is filler the kernel must not read as features).
    random     normal features, tie-free
    quarter    multiples of 1/4 in [-1, 1]: every difference, square and sum is exact in fp32, many exact ties
    identical  N copies of one row: every list must be 0 .. k-1"""
    rng = np.random.default_rng([KNN_FAMILIES.index(family), B, N, C])
    x = rng.standard_normal((B, N, ld)).astype(F)
    if family == "quarter":
        x = (rng.integers(-4, 5, (B, N, ld)) / 4.0).astype(F)
    elif family == "identical":
        x[:, :, :C] = x[:, :1, :C]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def knn_expected(family, B, N, C, ld):
    """hm_knn_feat's list of depth min(N, 32); a k-list is its prefix (a prefix of a lexicographically sorted list is the
    sorted shorter list)."""
    import ecg_hostmath
    idx, dist = ecg_hostmath.knn_feat(knn_cloud(family, B, N, C, ld), min(N, 32), C)
    idx.setflags(write=False)
    dist.setflags(write=False)
    return idx, dist


def float64_ranking(x, C, k):
    """(order[B,N,k+1 or N], sorted exact squared distances) of the stable float64 sort."""
    rows = np.asarray(x[:, :, :C], np.float64)
    d = host.sqdist_rows(rows, rows)
    order = np.argsort(d, axis=-1, kind="stable")
    return order, np.take_along_axis(d, order, axis=-1)


@functools.lru_cache(maxsize=None)
def dense_case(B, N, C, k, kind="random"):
    """(x[B,N,C], idx[B,N,k] int32, W0, b0, W1, b1, W2, b2) fp32, weights and features O(1).
    random    neighbour lists drawn at random (repeats happen)
    self      every neighbour is the point itself
    repeat    one neighbour repeated k times
    last      x_j = x_i for all but the last neighbour, which is far away: the maximum of most channels is attained there only
    negative  W2 = 0 and b2 < 0: every s2 is negative for every neighbour (a pool that starts at 0 returns 0)
    zero      all weights 0: the output must be [relu(b0), x, relu(b1), b2] exactly"""
    rng = np.random.default_rng([B, N, C, k, sum(map(ord, kind))])
    G = host.G
    x = rng.standard_normal((B, N, C)).astype(F)
    idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
    u = lambda n_out, n_in: (rng.uniform(-1, 1, (n_out, n_in)) * 2 / np.sqrt(n_in)).astype(F)
    W0, W1, W2 = u(G, 2 * C), u(G, G + C), u(G, 2 * G + C)
    b0, b1, b2 = (rng.uniform(-0.5, 0.5, G).astype(F) for _ in range(3))
    if kind == "self":
        idx[:] = np.arange(N, dtype=np.int32)[None, :, None]
    elif kind == "repeat":
        idx[:] = idx[:, :, :1]
    elif kind == "last":
        idx[:] = np.arange(N, dtype=np.int32)[None, :, None]
        idx[:, :, -1] = (np.arange(N, dtype=np.int32)[None, :] + 1) % N
    elif kind == "negative":
        W2[:] = 0
        b2 = -np.abs(b2) - F(0.25)
    elif kind == "zero":
        W0[:], W1[:], W2[:] = 0, 0, 0
    out = (x, idx, W0, b0, W1, b1, W2, b2)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dense_expected(B, N, C, k, kind="random"):
    """(float64 restatement [B,N,C+72] as rows, max |float32 restatement - float64|)."""
    x, idx, *w = dense_case(B, N, C, k, kind)
    xc = np.ascontiguousarray(np.swapaxes(x, 1, 2))
    f64 = host.dense_conv(xc, idx.astype(np.int64), *w, dtype=np.float64)
    f32 = host.dense_conv(xc, idx.astype(np.int64), *w, dtype=np.float32)
    assert f32.dtype == F
    rows = np.ascontiguousarray(np.swapaxes(f64, 1, 2))
    rows.setflags(write=False)
    return rows, float(np.abs(f32.astype(np.float64) - f64).max())
