"""Inputs shared by tests/test_solve_seed_host.py (CPU) and tests/test_gpu_solve_seed.py (GPU): clouds on which the rule of
houv_solve_seed (csrc/solve_seed.hip; NumPy statement: scripts/sim_solve_seed.py `seed_records`) is exact in fp32, so that the
kernel's records can be compared with the float64 statement index for index.

Grid clouds.  Unit u = 2^-6; every coordinate is an integer number of units below 2^10, so every difference, square and sum of
three squares is an integer below 2^24 u^2: exact in fp32 whatever the order and whether or not an fma contracts it.  Under the
identity pose (V and c any axis, a = -0.5 in window 0: theta = 0, R = I exactly; s = -0.5 in trans_mode 0: sigma = 0, T = 0) a
moved point is its source point to the bit, as in tests/solve_select_cases.py.

Run t (32 consecutive points) of the source has x in {8t, 8t + 2} units and of the target x in {8t + 5, 8t + 7}; y and z are random
integers in [0, 16).  So along x a target point at 8t + 5 is 3 units from the source boxes t and t + 1 -- two equidistant boxes --
and a source point at 8t + 2 is 3 units from the target boxes t - 1 and t; in the view metric that drops x every box overlaps
the query or ties with others at a small integer distance.  Run 3 of the source and run 5 of the target are 32 copies of one
point (a tile of equal points: 32-fold ties inside the run), and the sizes leave the last run partly filled."""
import numpy as np

U = 2.0 ** -6
IDENTITY = np.array([0.0, 0.0, 1.0, -0.5, 0.0, 1.0, 0.0, -0.5])      # V, a, c, s: R = I and T = 0 in window 0, trans_mode 0

# (N, M, views): 300 = 9 runs + 12 points (256-thread solve variant, 512-thread seed kernel); 2500 = 78 runs + 4 points (the
# 1024-thread seed kernel, super-tile solve); N != M with the full metric alone
GRID_SHAPES = [(300, 300, True), (2500, 2500, True), (300, 270, False)]


def _grid_cloud(n, xs, equal_run, equal_point, rng):
    runs = -(-n // 32)
    pts = np.empty((runs * 32, 3), np.float64)
    pts[:, 0] = (8 * np.repeat(np.arange(runs), 32) + rng.choice(xs, runs * 32))
    pts[:, 1:] = rng.integers(0, 16, (runs * 32, 2))
    pts[equal_run * 32:(equal_run + 1) * 32] = equal_point
    assert pts.max() < 1024
    return (pts[:n] * U).astype(np.float32)


def grid_pair(N, M, seed=5):
    """src fp32 [N, 3], tgt fp32 [M, 3] of the construction above."""
    rng = np.random.default_rng(seed)
    return _grid_cloud(N, [0, 2], 3, (24, 5, 5), rng), _grid_cloud(M, [5, 7], 5, (45, 7, 7), rng)


def nan_grid_pair(N, M, seed=6):
    """The grid pair with: source point 5 and target point 40 all NaN (a NaN query; a NaN reference that must seed nobody); run 4
    of the target all NaN (its box is empty: at infinite distance from every query); run 6 of the target with x = NaN in its even
    points and y = NaN in its odd ones -- its box is finite on every axis but none of its points is at a finite distance in the
    full metric, nor in the view that drops z, so the queries next to it fall back to a finite reference elsewhere -- while the
    views that drop x or y still find finite points in it."""
    src, tgt = grid_pair(N, M, seed)
    src[5] = np.nan
    tgt[40] = np.nan
    tgt[4 * 32:5 * 32] = np.nan
    tgt[6 * 32:7 * 32:2, 0] = np.nan
    tgt[6 * 32 + 1:7 * 32:2, 1] = np.nan
    return src, tgt


def expected_records(src, tgt, nmet):
    """(direction B [M, nmet], direction A [N, nmet]) of the float64 statement under the identity pose."""
    from scripts.sim_solve_seed import seed_records
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    return seed_records(t, s, nmet), seed_records(s, t, nmet)
