"""Shared by tests/golden/make_golden_vrcnet_grad.py and the tests that read its fixtures: the file names
and the seeded inputs.  Weights, inputs, lists and the loss weights G are regenerated from the stored seed (NumPy's PCG64 streams
are stable), so the fixtures hold only the seed, the lists (as a check) and the sampled gradients."""
import numpy as np

import vrcnet_grad_host as gh

KEEP = 1024                                # stored entries per tensor, at most
A_C, A_K, N, B = (64, 128, 256, 512), (10, 16), 40, 2
UNIT = dict(cin=64, cout=64, ks=(10, 20), layers=2)
FILE_B = "g30_vrcnet_grad_b.npz"


def file_a(C):
    return f"g30_vrcnet_grad_a{C}.npz"


def inputs_a(C, k, seed):
    """-> (state of one SA_module, x[B,C,1,N], idx[B,N,k], G[B,C,1,N])."""
    rng = np.random.default_rng([30, C, k, seed])
    state = gh.sa_state(rng, "", C, k)
    x = rng.standard_normal((B, C, 1, N)).astype(np.float32)
    idx = rng.integers(0, N, (B, N, k))
    return state, x, idx, rng.standard_normal((B, C, 1, N)).astype(np.float32)


def inputs_b(seed):
    """-> (state of SKN_Res_unit(64, 64, [10, 20], 2), feat[B,64,1,N], [idx10, idx20], G[B,64,1,N])."""
    rng = np.random.default_rng([31, seed])
    state = gh.unit_state(rng, "", UNIT["cin"], UNIT["cout"], UNIT["ks"], UNIT["layers"])
    x = rng.standard_normal((B, UNIT["cin"], 1, N)).astype(np.float32)
    idxs = [rng.integers(0, N, (B, N, k)) for k in UNIT["ks"]]
    return state, x, idxs, rng.standard_normal((B, UNIT["cout"], 1, N)).astype(np.float32)


def load_a(g, key):
    C, k = (int(t) for t in key[2:].split("_"))
    state, x, idx, G = inputs_a(C, k, int(g[f"{key}_seed"]))
    assert np.array_equal(idx, g[f"{key}_idx"])
    return state, x, idx, G


def load_b(g):
    state, x, idxs, G = inputs_b(int(g["unit_seed"]))
    assert all(np.array_equal(idx, g[f"unit_idx{i}"]) for i, idx in enumerate(idxs))
    return state, x, idxs, G


def sample(name, size):
    """The flat entries of tensor `name` that a fixture stores: all of them up to KEEP, else KEEP seeded ones, ascending."""
    if size <= KEEP:
        return np.arange(size)
    rng = np.random.default_rng([32] + [ord(c) for c in name])
    return np.sort(rng.choice(size, KEEP, replace=False))
