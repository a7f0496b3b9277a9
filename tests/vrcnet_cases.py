"""Shared inputs of the VRCNet tests (CPU and GPU) and of tests/golden/make_golden_vrcnet.py: the golden cases of
tests/golden/g27_vrcnet*.npz, their cfgs and seeded states, and the houv_sa_attn cases with their float64 expectations.
Everything is computed once and handed out read-only."""
import functools
import os
import sys

import numpy as np

import vrcnet_host as host

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import vrcnet_weights  # noqa: E402

F = np.float32
SA_C = (64, 128, 256, 512)
LAYER_K = (10, 16)
LAYER_N = 40
SK_KS = (10, 20)
# the encoder golden: the smallest hierarchy that halves three times and still leaves k = 16 points at the last level (the
# reference's knn cannot list 16 neighbours among fewer points)
ENC_PTS, ENC_K, ENC_PK = (128, 64, 32, 16), (16,), 10
# the three model cases, B = 2 (tests/golden/g27_vrcnet_<name>.npz)
MODEL_CASES = {
    "a": host.cfg(),                                                                       # the shipped cfg
    "b": host.cfg(layers=(2, 1, 1, 1), knn_list=(10, 20), points_label=False, local_folding=True, num_coarse_raw=512,
                  num_input=1024, num_fps=2048, num_coarse=1024, num_points=3072),
    "c": host.cfg(layers=(2, 1, 1, 1), knn_list=(10, 20), points_label=False, local_folding=False, num_coarse_raw=512,
                  num_input=1024, num_fps=2048, num_coarse=1024, num_points=3072),
}
# The largest share of a k-NN decision's entries that a `_safe` mask may exclude (an entry is excluded when the reference's
# choice is not the float64 ranking's or its float64 margin to a neighbour in that ranking is within what fp32 rounding and 4x
# the float32 spread of the rows can move: make_golden_vrcnet.safe_mask).  Measured by the generator for the reference on the
# CPU: 0.4 % .. 2.03 % on coordinates (the worst is knn1_0 of case a), 1.3 % .. 1.5 % on the 256-channel features of
# expansion1, 0.9 % on the 64-channel ones of expansion2.  The bound is 1.5x the worst of them; the generator and the GPU test
# both assert it.
MAX_UNSAFE_SHARE = 0.03


def tau(C):
    """ecg_cases.tau: the relative bound on a comparison of two fp32 squared distances over C channels."""
    return 4 * (C + 3) * 2.0 ** -24


def _frozen(st):
    for v in st.values():
        v.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def sa_state(C, k):
    return _frozen(vrcnet_weights.make_state(vrcnet_weights.sa_spec("", C, k), vrcnet_weights.SEED + C + k))


@functools.lru_cache(maxsize=None)
def sk_state(C=64, ks=SK_KS):
    return _frozen(vrcnet_weights.make_state(vrcnet_weights.sk_spec("", C, ks), vrcnet_weights.SEED + C + 1000))


@functools.lru_cache(maxsize=None)
def encoder_state():
    return _frozen(vrcnet_weights.make_state(vrcnet_weights.encoder_spec("", 3, ENC_K, (2, 2, 2, 2), 64), vrcnet_weights.SEED + 7))


@functools.lru_cache(maxsize=None)
def model_state(name):
    return _frozen(vrcnet_weights.make_state(vrcnet_weights.spec(MODEL_CASES[name]), vrcnet_weights.SEED + 11))


def reference_decisions(g, name):
    return {n: g[n].astype(np.int64) for n in host.decision_names(MODEL_CASES[name]) if n in g.files}


def safe_mask(g, decision):
    shape = g[decision].shape
    return np.unpackbits(g[f"{decision}_safe"])[:int(np.prod(shape))].reshape(shape).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- houv_sa_attn
@functools.lru_cache(maxsize=None)
def sa_case(B, N, C, k, kind="random"):
    """(x[B,N,C] rows, idx[B,N,k] int32) fp32 for sa_state(C, k).
    random   neighbour lists drawn at random (repeats happen)
    self     every neighbour is the point itself
    repeat   one neighbour repeated k times
    last     every neighbour is the point itself but the last, which is a far-away point (features 8x larger)
    wild     random lists with entries outside 0..N-1 (the kernel clamps them)"""
    rng = np.random.default_rng([B, N, C, k, sum(map(ord, kind))])
    x = rng.standard_normal((B, N, C)).astype(F)
    idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
    if kind == "self":
        idx[:] = np.arange(N, dtype=np.int32)[None, :, None]
    elif kind == "repeat":
        idx[:] = idx[:, :, :1]
    elif kind == "last":
        idx[:] = np.arange(N, dtype=np.int32)[None, :, None]
        idx[:, :, -1] = N - 1
        x[:, N - 1] *= 8
    elif kind == "wild":
        idx[:, ::3, 0], idx[:, 1::3, k - 1] = -5, N + 1000
    x.setflags(write=False)
    idx.setflags(write=False)
    return x, idx


def sa_host(state, x_rows, idx, dtype, prefix=""):
    """The restatement on rows: x[B,N,C] -> [B,N,C]."""
    xc = np.ascontiguousarray(np.swapaxes(x_rows, 1, 2))[:, :, None, :]
    out = host.sa_module(state, prefix, xc, np.clip(idx, 0, x_rows.shape[1] - 1).astype(np.int64), dtype)
    return np.ascontiguousarray(np.swapaxes(out[:, :, 0], 1, 2))


@functools.lru_cache(maxsize=None)
def sa_expected(B, N, C, k, kind="random"):
    """(float64 restatement [B,N,C] as rows, max |float32 restatement - float64|), out-of-range entries clamped."""
    x, idx = sa_case(B, N, C, k, kind)
    f64 = sa_host(sa_state(C, k), x, idx, np.float64)
    f32 = sa_host(sa_state(C, k), x, idx, np.float32)
    assert f32.dtype == F
    f64.setflags(write=False)
    return f64, float(np.abs(f32.astype(np.float64) - f64).max())
