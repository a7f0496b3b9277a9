"""NumPy restatement of houv_icp_refine's loop (houv_amd/csrc/icp.hip) with the arithmetic type as an argument, as in
tests/kabsch_host.py: float64 is the yardstick the kernel is held to, float32 shows what the formula itself loses.  Also the input
builders of tests/test_gpu_icp.py: clouds in which every decision of the loop (which target is nearest, inside or outside the
radius, stop or go on) is far from its threshold, so that float32 and float64 cannot legitimately disagree about any of them;
tests/test_icp_host.py checks that on the CPU for every case the GPU tests use."""
import collections
import functools
import os
import re

import numpy as np

import kabsch_host

EPS32 = kabsch_host.EPS32
ROWS = 256                         # nearest neighbours are searched this many source rows at a time
MAX_N = 8192                       # houv_icp_refine: Q <= 8 points per lane of a 1024-thread workgroup
LDS_BYTES = 160 * 1024             # what houv_icp_refine compares icp_smem_bytes(M, 1024) with
DEGENERATE_GAP = 0.05              # kabsch_host.make_case's floor on polar_gap

Case = collections.namedtuple("Case", "key src tgt init max_dist assign inlier")
Ref = collections.namedtuple("Ref", "T fitness rmse iterations trace count yard bound gap degenerate iterations32 same_trace deltas")


def _nearest(p, tgt, dtype):
    """Per row of p the lowest index of the nearest row of tgt and the squared distance to it, in dtype, ROWS rows at a time."""
    j = np.empty(len(p), np.int64)
    d2 = np.empty(len(p), dtype)
    tx, ty, tz = (np.ascontiguousarray(tgt[:, a]) for a in range(3))
    for r in range(0, len(p), ROWS):
        q = p[r:r + ROWS]
        dx, dy, dz = tx[None, :] - q[:, 0:1], ty[None, :] - q[:, 1:2], tz[None, :] - q[:, 2:3]
        d = dx * dx + dy * dy + dz * dz
        assert d.dtype == dtype
        jj = d.argmin(1)                                   # first = lowest index among equals
        j[r:r + ROWS] = jj
        d2[r:r + ROWS] = d[np.arange(len(q)), jj]
    return j, d2


def _kabsch_rotation(H, dtype):
    """H = U S V^T -> V diag(1, 1, det(V U^T)) U^T (kabsch_rotation, houv_math.h)."""
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        D = np.diag(np.array([1, 1, -1], dtype))
        R = Vt.T @ D @ U.T
    return R.astype(dtype)


def icp(src, tgt, init, max_dist, max_iter, rel_fit=1e-6, rel_rmse=1e-6, dtype=np.float64, deltas=None):
    """src[N,3], tgt[M,3], init[4,4] or None -> (T[4,4], fitness, rmse, iterations, trace), everything computed in dtype.
    The kernel's control flow: evaluate the correspondences under the current T; stop if it > 0 and both changes are < their
    thresholds, or it >= max_iter, or nothing corresponds; otherwise T = U T with U the Kabsch update from the centred sums.
    max_dist is rounded to float32 and squared (in float32 when dtype is float32, as the host entry does); the thresholds are the
    float32 values the entry receives.  trace: (inlier mask, target index) of every evaluation; `deltas`, a list, receives
    (|change of fitness|, |change of rmse|) of every evaluation after the first."""
    dtype = np.dtype(dtype).type
    s = np.asarray(src, dtype)
    g = np.asarray(tgt, dtype)
    N = len(s)
    md = np.float32(max_dist)
    md2 = md * md if dtype is np.float32 else dtype(md) * dtype(md)
    rel_fit, rel_rmse = dtype(np.float32(rel_fit)), dtype(np.float32(rel_rmse))
    R, t = np.eye(3, dtype=dtype), np.zeros(3, dtype)
    if init is not None:
        R, t = np.asarray(init, dtype)[:3, :3].copy(), np.asarray(init, dtype)[:3, 3].copy()
    prev_fit = prev_rmse = fit = rmse = dtype(0)
    trace = []
    it = 0
    while True:
        p = (s @ R.T + t).astype(dtype)
        j, d2 = _nearest(p, g, dtype)
        ok = d2 < md2                                      # strictly inside the radius
        trace.append((ok, j))
        cnt = int(ok.sum())
        fit = dtype(cnt) / dtype(N)
        rmse = np.sqrt(d2[ok].sum(dtype=dtype) / dtype(cnt)) if cnt else dtype(0)
        if it > 0 and deltas is not None:
            deltas.append((abs(float(prev_fit) - float(fit)), abs(float(prev_rmse) - float(rmse))))
        stop = it > 0 and abs(prev_fit - fit) < rel_fit and abs(prev_rmse - rmse) < rel_rmse
        if stop or it >= max_iter or cnt == 0:
            break
        prev_fit, prev_rmse = fit, rmse
        a, b = p[ok], g[j[ok]]
        mp, mn = a.sum(0, dtype=dtype) / dtype(cnt), b.sum(0, dtype=dtype) / dtype(cnt)
        H = ((a - mp).T @ (b - mn)).astype(dtype)
        Ru = _kabsch_rotation(H, dtype)
        tu = mn - Ru @ mp
        R, t = (Ru @ R).astype(dtype), (Ru @ t + tu).astype(dtype)
        it += 1
    T = np.eye(4, dtype=dtype)
    T[:3, :3], T[:3, 3] = R, t
    assert T.dtype == dtype
    return T, fit, rmse, it, trace


# ---------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    ax = axis / np.linalg.norm(axis)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _unit(rng, n=None):
    v = rng.standard_normal(3 if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frozen(key, src, tgt, init, max_dist, assign, inlier):
    for a in (src, tgt, init, assign, inlier):
        if a is not None:
            a.setflags(write=False)
    return Case(key, src, tgt, init, max_dist, assign, inlier)


@functools.lru_cache(maxsize=None)
def separated_case(N, M, seed):
    """-> Case(src[N,3], tgt[M,3], init[4,4], max_dist; assign[N], inlier[N]) in fp32, read-only.
    With g = ceil(M^(1/3)) and c = 1 / g the targets are M distinct cells of a g^3 lattice, at (cell + 0.5 + U(-0.2, 0.2)) c - 0.5:
    two targets are >= 0.6 c apart.  Every source point picks a random target (shared when N > M) and sits within 0.1 c of it;
    N // 5 of them (none when N < 5) are outliers on a shell of radius 0.9 + 3 max_dist + U(0, 0.2) about the origin instead,
    outside the targets' cube.  max_dist = 0.4 c.  src is that cloud moved back by a random rigid motion (0.3..2.5 rad,
    |t| <= 0.5 per axis); init is the motion composed with a perturbation in the targets' frame, a rotation of 0.05 c rad and a
    translation of length 0.05 c, which moves no point of the unit ball by more than 0.1 c: inliers stay within 0.2 c = half the
    radius of their target and at least 0.4 c = one radius farther from every other."""
    rng = np.random.default_rng([N, M, seed])
    g = 1
    while g ** 3 < M:
        g += 1
    c = 1.0 / g
    cells = rng.choice(g ** 3, size=M, replace=False)
    cells = np.stack([cells // (g * g), (cells // g) % g, cells % g], 1)
    tgt = (cells + 0.5 + rng.uniform(-0.2, 0.2, (M, 3))) * c - 0.5
    max_dist = float(np.float32(0.4 * c))
    assign = rng.integers(0, M, N)
    q = tgt[assign] + _unit(rng, N) * rng.uniform(0, 0.1 * c, (N, 1))
    inlier = np.ones(N, bool)
    if N >= 5:
        out = rng.permutation(N)[:N // 5]
        inlier[out] = False
        q[out] = _unit(rng, len(out)) * (0.9 + 3 * max_dist + rng.uniform(0, 0.2, (len(out), 1)))
    R0 = _rotation(rng.standard_normal(3), rng.uniform(0.3, 2.5))
    t0 = rng.uniform(-0.5, 0.5, 3)
    src = (q - t0) @ R0                                    # rows R0^T (q - t0): R0 src + t0 = q
    Pm = np.eye(4)
    Pm[:3, :3] = _rotation(rng.standard_normal(3), 0.05 * c)
    Pm[:3, 3] = _unit(rng) * 0.05 * c
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R0, t0
    return _frozen(("separated", N, M, seed), src.astype(np.float32), tgt.astype(np.float32), (Pm @ T0).astype(np.float32),
                   max_dist, assign, inlier)


def _lattice(M, step, nx=4, ny=4):
    j = np.arange(M)
    return np.stack([j % nx, (j // nx) % ny, j // (nx * ny)], 1) * step


TIE_M, TIE_N = 70, 13
_TIE_SITES = (0, 7, 13, 22, 27, 35, 44, 50, 57, 61, 66, 68, 1, 10)     # spread over the lattice, not coplanar


@functools.lru_cache(maxsize=None)
def tie_case(a, b, flip):
    """M = 70 targets on a dyadic lattice (4 x 4 x 5 integer sites: wide enough next to the far point that H stays well
    conditioned, polar_gap ~ 0.4), except targets a < b, which sit at (10 +- 1/8, 1/4, -1/2) (flip: b gets
    the +).  Twelve source points lie exactly on other targets, the thirteenth at (10, 1/4, -1/2), exactly 1/8 from a and from b:
    an exact tie, which the lowest index (a) must win.  init None, max_dist 0.5.  Every coordinate is a small dyadic number, so
    every difference, product and sum of the kernel's distance expression is exact in fp32, fused or not."""
    assert 0 <= a < b < TIE_M
    tgt = _lattice(TIE_M, 1.0).astype(np.float64)
    sa = -0.125 if flip else 0.125
    tgt[a] = (10 + sa, 0.25, -0.5)
    tgt[b] = (10 - sa, 0.25, -0.5)
    sites = [s for s in _TIE_SITES if s not in (a, b)][:TIE_N - 1]
    src = np.concatenate([tgt[sites], [[10, 0.25, -0.5]]])
    assign = np.array(sites + [a])
    return _frozen(("tie", a, b, bool(flip)), src.astype(np.float32), tgt.astype(np.float32), None, 0.5, assign,
                   np.ones(TIE_N, bool))


@functools.lru_cache(maxsize=None)
def threshold_case():
    """M = 45 targets on a lattice of multiples of 1/2 in [1, 2.5]^3, max_dist = 1/8, identity pose.  Seven source points each lie
    exactly 1/8 - 2^-10, 1/8 and 1/8 + 2^-10 from their target along one axis (either sign), four more on a target: only the first
    and the last group correspond (strict <).  Two more lie 1/16 and 1/32 from the origin, where no target is: they correspond to
    nothing unless the 19 pad slots of the target cloud act as points at the origin.  Coordinates, differences and squares are
    exact in fp32."""
    M = 45
    tgt = _lattice(M, 0.5).astype(np.float64) + 1.0
    src, assign, inlier = [], [], []
    k = 0
    for off, inside in ((0.125 - 2.0 ** -10, True), (0.125, False), (0.125 + 2.0 ** -10, False)):
        for i in range(7):
            j = (5 * k + 2) % M
            d = np.zeros(3)
            d[i % 3] = off if i % 2 == 0 else -off
            src.append(tgt[j] + d); assign.append(j); inlier.append(inside)
            k += 1
    for j in (0, 17, 31, 44):
        src.append(tgt[j]); assign.append(j); inlier.append(True)
    for near_origin in ((0.0625, 0, 0), (0, 0, -0.03125)):
        src.append(np.array(near_origin)); assign.append(0); inlier.append(False)
    order = np.random.default_rng(7).permutation(len(src))              # mix the groups over the lanes
    src, assign, inlier = np.array(src)[order], np.array(assign)[order], np.array(inlier)[order]
    assert np.array_equal(src.astype(np.float32).astype(np.float64), src)
    return _frozen(("threshold",), src.astype(np.float32), tgt.astype(np.float32), None, 0.125, assign, inlier)


@functools.lru_cache(maxsize=None)
def tail_case(N, M, seed):
    """separated_case(N, M, seed) with the source frame moved so that its ORIGIN maps onto a target under init: the same moved
    cloud, the same correspondences, but a lane past the end of the cloud, which carries the point (0, 0, 0), would sit on a target
    and be counted if the kernel did not mask it.  -> the Case, its key ending in the index of that target."""
    base = separated_case(N, M, seed)
    k = (7 * seed + 3) % M
    T = base.init.astype(np.float64)
    s0 = (base.tgt[k].astype(np.float64) - T[:3, 3]) @ T[:3, :3]          # R^T (tgt_k - t): T s0 = tgt_k
    init = base.init.copy()
    init[:3, 3] = (T[:3, :3] @ s0 + T[:3, 3]).astype(np.float32)
    return _frozen(("tail", N, M, seed), (base.src.astype(np.float64) - s0).astype(np.float32), base.tgt, init, base.max_dist,
                   base.assign, base.inlier)


def tail_target(N, M, seed):
    return (7 * seed + 3) % M


# ---------------------------------------------------------------------------------------------------------------
# reference and bounds
# ---------------------------------------------------------------------------------------------------------------
def inlier_gap(case):
    """kabsch_host.polar_gap of the built inlier pairs; 0 when there are too few pairs for H to have rank 2."""
    m = case.inlier
    if m.sum() < 3:
        return 0.0
    with np.errstate(all="ignore"):
        gap = kabsch_host.polar_gap(case.src[m].T[None], case.tgt[case.assign[m]].T[None])
    return gap if np.isfinite(gap) else 0.0


def mean_residual(T, case):
    """|T (mean of the built inlier source points) - mean of their targets|, max over the axes, in float64."""
    m = case.inlier
    T = np.asarray(T, np.float64)
    ms, mt = case.src[m].astype(np.float64).mean(0), case.tgt[case.assign[m]].astype(np.float64).mean(0)
    return float(np.abs(T[:3, :3] @ ms + T[:3, 3] - mt).max())


@functools.lru_cache(maxsize=None)
def _reference(case_fn, args, max_iter, rel_fit, rel_rmse):
    case = case_fn(*args)
    deltas = []
    T64, f64, r64, it64, trace = icp(case.src, case.tgt, case.init, case.max_dist, max_iter, rel_fit, rel_rmse, np.float64, deltas)
    T32, _, r32, it32, trace32 = icp(case.src, case.tgt, case.init, case.max_dist, max_iter, rel_fit, rel_rmse, np.float32)
    same = len(trace) == len(trace32) and all(np.array_equal(m, m32) and np.array_equal(j[m], j32[m])
                                              for (m, j), (m32, j32) in zip(trace, trace32))
    gap = inlier_gap(case)
    degenerate = gap < DEGENERATE_GAP
    if degenerate:
        # R is arbitrary; what T must still do is carry the inliers' mean onto their targets' mean: t = mt - R ms, formed from
        # operands as large as ms, mt and t itself
        m = case.inlier
        yR = float("nan")
        yt = mean_residual(T32, case) if m.any() else 0.0
        big = max(np.abs(T32[:3, 3]).max(), np.abs(case.src[m]).max(initial=0), np.abs(case.tgt).max())
        bound_R, bound_t = float("nan"), 4 * yt + 8 * EPS32 * float(big)
    else:
        yR = float(np.abs(T32[:3, :3].astype(np.float64) - T64[:3, :3]).max())
        yt = float(np.abs(T32[:3, 3].astype(np.float64) - T64[:3, 3]).max())
        bound_R = 4 * yR + 8 * EPS32 * float(np.abs(T64[:3, :3]).max())
        bound_t = 4 * yt + 8 * EPS32 * float(np.abs(T64[:3, 3]).max())
    yr = abs(float(r32) - float(r64))
    # a pose error shifts every residual by at most bound_t + 2 bound_R (the moved inliers lie within radius 2); 32 roundings cover
    # the longest summation chain: 8 per-lane terms, 6 butterfly steps, 16 waves, the division and the square root
    # (degenerate: the residuals do not depend on the arbitrary rotation, only on where the mean lands)
    bound_rmse = 4 * yr + 32 * EPS32 * float(r64) + (bound_t if degenerate else bound_t + 2 * bound_R)
    T64.setflags(write=False)
    return Ref(T64, float(f64), float(r64), it64, trace, int(trace[-1][0].sum()), (yR, yt, yr), (bound_R, bound_t, bound_rmse),
               gap, degenerate, it32, same, tuple(deltas))


_BUILDERS = {"separated": separated_case, "tail": tail_case, "tie": tie_case, "threshold": threshold_case}


def reference_and_bounds(case, max_iter=30, rel_fit=1e-6, rel_rmse=1e-6):
    """-> Ref for a Case of one of the builders: the float64 restatement's (T, fitness, rmse, iterations, trace, final inlier
    count; deltas = its |change of fitness|, |change of rmse| per evaluation; same_trace = the float32 restatement took the same
    inliers and the same target for each of them in every evaluation), yard = the float32 restatement's error against it (R, t, rmse), and bound:
        R and t separately   4 x yard + 8 x 2^-24 x max |value|
        rmse                 4 x yard + 32 x 2^-24 x rmse + bound_t + 2 bound_R
    The x4 is the project's margin for a different summation order.  A case whose built inlier pairs have
    polar_gap < 0.05 (M = 1 and M = 2 always) is degenerate: its rotation is arbitrary in any arithmetic, bound_R is NaN and bound_t
    bounds mean_residual() instead, with the float32 run's mean_residual as the yardstick."""
    return _reference(_BUILDERS[case.key[0]], case.key[1:], int(max_iter), float(rel_fit), float(rel_rmse))


def errors(T, ref):
    """(max |R - R64|, max |t - t64|)."""
    T = np.asarray(T, np.float64)
    return float(np.abs(T[:3, :3] - ref.T[:3, :3]).max()), float(np.abs(T[:3, 3] - ref.T[:3, 3]).max())


# ---------------------------------------------------------------------------------------------------------------
# the LDS the kernel asks for, as the host entry computes it
# ---------------------------------------------------------------------------------------------------------------
def _constant(name):
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "houv_amd", "csrc")
    for header in ("houv_common.h", "houv_math.h"):
        with open(os.path.join(csrc, header)) as f:
            m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
        if m:
            return int(m.group(1))
    raise AssertionError(f"{name} not found in the kernel headers")


def smem_bytes(M, block):
    """icp_smem_bytes (icp.hip): the padded target cloud, one reduction row per wave, the result row, the pose and a flag."""
    k_sub, acc = _constant("kSub"), _constant("kAccStride")
    mpad = (M + k_sub - 1) // k_sub * k_sub
    return mpad * 16 + (block // 64) * acc * 4 + acc * 4 + 16 * 4 + 64


def largest_m():
    """The largest M houv_icp_refine accepts: icp_smem_bytes(M, 1024) <= 160 KiB, whatever block the launch then takes."""
    k_sub = _constant("kSub")
    M = (LDS_BYTES - smem_bytes(0, 1024)) // (16 * k_sub) * k_sub
    assert smem_bytes(M, 1024) <= LDS_BYTES < smem_bytes(M + 1, 1024)
    return M


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_icp.py (tests/test_icp_host.py checks the builders' guarantees for every one of them)
# ---------------------------------------------------------------------------------------------------------------
# kernel path -> (N, M): the first N of a path and a tail (N no multiple of the block), the last N of a path; M below 16, one
# past a tracking unit, one short of a sub-tile, a whole sub-tile, one past it, odd and even numbers of sub-tiles
PATH_CASES = (("<256,1>", 63, 15), ("<256,1>", 256, 17), ("<256,2>", 257, 31), ("<256,2>", 512, 32),
              ("<256,4>", 513, 33), ("<256,4>", 1024, 48), ("<512,4>", 1025, 100), ("<512,4>", 2048, 257),
              ("<1024,4>", 2049, 1000), ("<1024,4>", 4096, 70), ("<1024,8>", 4097, 33), ("<1024,8>", 8192, 1000))
TAIL_CASES = tuple((p, N, M) for p, N, M in PATH_CASES[0::2])      # the first N of every path: all but one lane of a chunk idle
STOP_CASES = ((513, 33), (2049, 1000))
DEGENERATE_CASES = ((1, 1), (5, 1), (2, 2))
TIE_PAIRS = ((3, 9), (5, 20), (14, 40), (15, 16), (31, 32), (2, 69))
NO_CORRESPONDENCE_CASE = (300, 5)
PLUMBING_CASE = (300, 40)


def pairs_of(N):
    return 3 if N <= 2048 else 2


def lds_cases():
    return ((64, largest_m()), (2049, largest_m()))


def separated_cases_in_use():
    """Every (N, M, seed) the GPU tests build."""
    out = [(N, M, s) for _, N, M in PATH_CASES for s in range(pairs_of(N))]
    out += [(N, M, 0) for N, M in lds_cases()]
    out += [(N, M, s) for N, M in DEGENERATE_CASES + (NO_CORRESPONDENCE_CASE, PLUMBING_CASE) for s in range(3)]
    return sorted(set(out + [(N, M, 0) for N, M in STOP_CASES]))


def pushed_away(case, radii=10.0):
    """-> (src', clearance): the case's source moved so that, under init, the whole cloud lands `radii` search radii farther along
    the coordinate direction that leaves it farthest from every target; clearance = the smallest point-to-target distance then, in
    radii (float64).  Nothing corresponds when it is well above 1."""
    T = case.init.astype(np.float64)
    p = case.src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    g = case.tgt.astype(np.float64)
    best = None
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = np.zeros(3)
            d[axis] = sign * radii * case.max_dist
            near = np.sqrt((((p + d)[:, None, :] - g[None]) ** 2).sum(-1).min())
            if best is None or near > best[1]:
                best = (d, near)
    src = (case.src.astype(np.float64) + best[0] @ T[:3, :3]).astype(np.float32)      # rows R^T d: T src' = T src + d
    near = np.sqrt((((src.astype(np.float64) @ T[:3, :3].T + T[:3, 3])[:, None, :] - g[None]) ** 2).sum(-1).min())
    return src, float(near / case.max_dist)
