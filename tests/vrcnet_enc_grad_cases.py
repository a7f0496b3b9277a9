"""Shared by tests/golden/make_golden_vrcnet_enc_grad.py and the tests that read its fixture: the file
name and the seeded inputs.  The encoder's case is the encoder golden's of vrcnet_cases.py (ENC_PTS, ENC_K, ENC_PK,
encoder_state()); inputs and the loss weights G are regenerated from the stored seed, so the fixture holds only the seed, the
decisions and the sampled gradients."""
import numpy as np

import vrcnet_cases as cases

FILE = "g31_vrcnet_enc_grad.npz"
KEEP = 1024                                # stored entries per tensor, at most
KEEP_ENCODER = 256                         # ... of the whole encoder's 148 tensors, which at 1024 would pass the 1 MiB of a fixture
OUT_SIZE = 64
NARROW = dict(B=2, N=128, S=64, C=64, pk=10)
# The input of the module-level gradient test (tests/test_gpu_vrcnet_enc_train.py).  No seed below 64 clears the generator's 4x
# margin for the whole encoder, so the test takes the (B, seed) of the generator's walk whose float64
# restatement stays furthest from its kinks in units of its own float32 spread: B = 1, seed 3, nearest non-zero ReLU input 7.4e-6
# = 2.2x the spread of 3.3e-6, every pooled lead and conv5 lead >= 2.4e-5 = 7x.  A float32 implementation whose error stays within
# the spread takes every mask and every maximum as float64 does; the test re-derives both figures and asserts >= 2x.
TRAIN_CASE = (1, 3)


def inputs_encoder(B, seed):
    """-> (x[B,3,N] in the unit cube, G[B,64,N])."""
    rng = np.random.default_rng([34, B, seed])
    x = rng.uniform(-0.5, 0.5, (B, 3, cases.ENC_PTS[0])).astype(np.float32)
    return x, rng.standard_normal((B, OUT_SIZE, cases.ENC_PTS[0])).astype(np.float32)


def inputs_narrow(seed):
    """-> (feat[B,C,N], pts[B,N,3], G[B,2C,N]) of the pooling followed by the up-sampling."""
    rng = np.random.default_rng([35, seed])
    n = NARROW
    feat = rng.standard_normal((n["B"], n["C"], n["N"])).astype(np.float32)
    pts = rng.uniform(-0.5, 0.5, (n["B"], n["N"], 3)).astype(np.float32)
    return feat, pts, rng.standard_normal((n["B"], 2 * n["C"], n["N"])).astype(np.float32)


def sample(name, size, keep=KEEP):
    """The flat entries of tensor `name` that the fixture stores: all of them up to `keep`, else `keep` seeded ones, ascending."""
    if size <= keep:
        return np.arange(size)
    rng = np.random.default_rng([36] + [ord(c) for c in name])
    return np.sort(rng.choice(size, keep, replace=False))
