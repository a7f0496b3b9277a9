"""Seeded inputs and shape lists of tests/test_gpu_pcn.py and tests/test_pcn_host.py.  Bounds are not
stored here: every test computes 4x the float32 restatement's own maximum error against float64 on the inputs it uses (the
kernel-level factor of idam_cases.py: it covers a different but equally careful summation order) and prints it."""
import numpy as np

T = 64                                    # houv_amd.ops.PCN_ROW_TILE, asserted equal by the tests
MLP_SHAPES = [(3, 128, 256), (256, 512, 1024)]          # the served (Cin, H, Cout)
MLP_B = [1, 3]
MLP_N = [1, T - 1, T, T + 1, 2 * T + 5]
FOLD_SCALES = [1, 2, 3, 4, 8, 16]
FOLD_NC = [1, T - 1, T + 1]
FOLD_B = [1, 3]
GOLDEN_CASES = {"p64c64": (64, 64), "p96c24": (96, 24), "p2048c1024": (2048, 1024)}


def mlp_case(B, N, Cin, H, Cout, per_cloud=True, seed=0):
    """-> (x[B,N,Cin], W1[H,Cin], shift1[B,H] or [H], W2[Cout,H], b2[Cout]): O(1) inputs, weights uniform * 2 / sqrt(fan_in), so
    that the hidden layer and y are O(1) and about half of the hidden units are cut by the ReLU."""
    rng = np.random.default_rng(100003 * seed + 1009 * N + 31 * B + Cin)
    x = rng.uniform(-1, 1, (B, N, Cin))
    W1 = rng.uniform(-1, 1, (H, Cin)) * 2 / np.sqrt(Cin)
    shift1 = rng.uniform(-0.3, 0.3, (B, H) if per_cloud else (H,))
    W2 = rng.uniform(-1, 1, (Cout, H)) * 2 / np.sqrt(H)
    b2 = rng.uniform(-0.1, 0.1, Cout)
    return tuple(a.astype(np.float32) for a in (x, W1, shift1, W2, b2))


def fold_case(B, nc, scale, seed=0):
    """-> (coarse[B,nc,3], cvec[B,512], grid[2,scale], Wgp[512,5], W2[512,512], b2[512], W3[3,512], b3[3])."""
    rng = np.random.default_rng(7919 * seed + 101 * nc + 7 * scale + B)
    coarse = rng.uniform(-0.5, 0.5, (B, nc, 3))
    cvec = rng.uniform(-1, 1, (B, 512))
    grid = rng.uniform(-0.05, 0.05, (2, scale))
    Wgp = rng.uniform(-1, 1, (512, 5)) * 4 / np.sqrt(5)
    W2 = rng.uniform(-1, 1, (512, 512)) * 2 / np.sqrt(512)
    b2 = rng.uniform(-0.1, 0.1, 512)
    W3 = rng.uniform(-1, 1, (3, 512)) * 2 / np.sqrt(512)
    b3 = rng.uniform(-0.1, 0.1, 3)
    return tuple(a.astype(np.float32) for a in (coarse, cvec, grid, Wgp, W2, b2, W3, b3))
