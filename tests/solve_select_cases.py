"""Inputs, expected values and bounds shared by tests/test_solve_select_host.py (CPU) and tests/test_gpu_solve_select.py (GPU):
the top-k selection of the fused solve loop (select_smallest / repair_direction_a in solve.hip, select_threshold and its tie
rank in solve_large.hip, the radix passes of houv_solve.h) at every k, tie pattern and launch path.

Tier A -- selection made exact by construction.  Unit u = 2^-12; sites on a cubic grid of spacing 2^14 u; target i sits on site
pi(i), source i on site i plus (m_i, 0, 0) u; the surplus points of the larger cloud sit next to a used site (a target at
site - D u, a source at site + (m_site + D) u).  Under the identity pose (a = -0.5, base 0; s = -0.5 / trans_mode 0 or s = 0 /
trans_mode 1) every nearest neighbour lies along x, d = m^2 u^2, sqrtf(d) = m u and every fp32 partial sum of a direction
(total <= 2^24 units) are exact, so cd = fl32(S u) / fl32(k) is ONE rounding of integers known from the construction and
score / loss follow bit for bit.  tests/test_solve_select_host.py re-establishes each of these claims with a float32 model of
the kernel's distance expression and a NumPy model of the radix select.

Tier B -- generic poses and synthetic.make_pairs clouds, k swept.  Reference: `cd_reference` below, a float64 restatement that
takes the fp32 R and T the kernel reports.  Bound per case: 4x what the same restatement run in float32 loses against float64
(max over hypotheses and terms), capped at half the float64 gap to the neighbouring selections k-1 and k+1, so that no
tolerance can hide an off-by-one selection.  Measured on an MI355X with the kernels' own R and T, over the k of `k_values`
(absolute figures on terms of 0.01 .. 0.1; three hypotheses per case):

    case (N, M, views, k_view, kernel)       bound, smallest .. largest over k     min half gap     largest error   worst error/bound
    (200, 200, no views, in-LDS)            2.37e-08 (k=200) .. 7.52e-08 (k=100)  1.12e-04 (k=1)   2.50e-08 (k=63)   0.65 (k=64)
    (300, 512, no views, in-LDS)            7.67e-09 (k=64)  .. 6.88e-08 (k=2)    3.08e-05 (k=1)   1.44e-08 (k=2)    0.68 (k=64)
    (2048, 2048, no views, in-LDS)          8.67e-09 (k=63)  .. 1.29e-07 (k=2048) 1.31e-05 (k=1024) 2.12e-08 (k=1)   0.32 (k=63)
    (4500, 4500, no views, large kernel)    1.68e-08 (k=64)  .. 5.96e-08 (k=2)    1.02e-05 (k=2250) 2.75e-08 (k=2250) 0.62 (k=2250)
    (40, 64, views, k_view=40, in-LDS)      4.27e-08 (k=1)   .. 7.39e-08 (k=39)   2.37e-04 (k=1)   1.59e-08 (k=39)   0.25 (k=1)
    (300, 512, views, k_view=200, in-LDS)   1.71e-08 (k=150) .. 6.88e-08 (k=2)    1.36e-05 (all k) 1.44e-08 (k=2)    0.36 (k=300)

Every bound is below 1 % of its half gap.  Where error/bound is exactly 0.25 the kernel returned the float32 restatement's bits.
Tier A with the view terms (NMET = 4): the worst error is 0.151 of the bound (k+1) 2^-24 at every size.
"""
import numpy as np

U = 2.0 ** -12             # Tier A's unit
SPACING = 1 << 14          # grid spacing in units
MAX_OFFSET = SPACING // 4  # every m, and m + D of a surplus point, stays at or below a quarter of the spacing
SUM_LIMIT = 1 << 24        # a direction's sum of all m: every fp32 partial sum is then an exact integer of units

# (full, partial) Tier A size per row of houv_solve_variant, in the table's order
INLDS_ROWS = [(64, 40), (128, 100), (256, 200), (512, 300), (768, 700), (1024, 900), (1536, 1100), (2048, 1800), (3072, 2500),
              (4096, 3500)]
LARGE_SHAPES = [(64, 64), (1024, 1024), (1025, 1025), (4096, 4096), (4097, 4097), (6000, 5000), (5000, 6000), (16384, 16384)]
LARGE_BLOCK = 1024         # solve_large_kernel ranks ties in (thread, chunk slot) order of 1024 threads
LOW_BYTE_MAX_COUNT = SUM_LIMIT // 4095   # m up to 4095 is allowed while count * 4095 <= 2^24 (the in-LDS sizes)


def inlds_shapes():
    """(N, M) of Tier A's in-LDS cases: every size as N == M, the full size of a row with a smaller target (N > M: direction 1
    wins, the repair path under solve_predict 1), the partial size with a smaller source (M > N); the pair stays in the row."""
    out = []
    for full, part in INLDS_ROWS:
        out += [(full, full), (full, full - max(3, full // 8)), (part, part), (part - max(3, part // 8), part)]
    return out


# ---- distance multisets by name ----------------------------------------------------------------------------------------------
def _spread(n, vals, rng):
    """m[n]: class vals[i % len] at index i, so every class has members in every wave and slot; then each block of len(vals)
    consecutive indices is shuffled."""
    m = np.array([vals[i % len(vals)] for i in range(n)], np.int64)
    L = len(vals)
    for s in range(0, n - L + 1, L):
        m[s:s + L] = rng.permutation(m[s:s + L])
    return m


def _class_cuts(m, pick):
    """k values around class `pick` (index into the sorted distinct values, clipped) of the multiset m: the cut one past the
    class start (remaining 1), mid-class, one before its end (remaining neq-1) and exactly at its end (neq == remaining)."""
    vals, counts = np.unique(m, return_counts=True)
    c = min(pick, len(vals) - 1)
    lo, neq = int(counts[:c].sum()), int(counts[c])
    return sorted({lo + 1, lo + max(1, neq // 2), lo + max(1, neq - 1), lo + neq})


def _ms_distinct(n, rng):
    if n <= MAX_OFFSET - 1:
        return rng.permutation(n).astype(np.int64) + 1, [], False
    m = rng.permutation(np.arange(n, dtype=np.int64) % 1000 + 1)      # the count does not allow distinct m: a ramp of 1000 classes
    return m, _class_cuts(m, 500), False


def _ms_classes(n, rng):
    m = _spread(n, [9, 10, 12, 15], rng)
    return m, sorted(set(_class_cuts(m, 1) + _class_cuts(m, 0))), False


def _ms_one_class(n, rng):
    return np.full(n, 37, np.int64), [], False


def _ms_top_byte(n, rng):          # d = 4^(2j) u^2: the keys differ in exponent bits 30..24 only
    m = _spread(n, [1, 4, 16, 64, 256, 1024], rng)
    return m, _class_cuts(m, 3), False


def _ms_mid_byte(n, rng):          # m^2 = q^2 2^12, q^2 in [128, 256): the keys differ in bits 22..16 only
    m = _spread(n, [768, 832, 896, 960], rng)
    return m, _class_cuts(m, 2), False


def _ms_low_byte(n, rng):          # m^2 in [2^23, 2^24) shares its upper 16 bits: the keys differ in the two low bytes only
    m = _spread(n, list(range(4000, 4008)), rng)
    return m, _class_cuts(m, 5), False


def _ties_clustered(n, rng, first):
    c = max(2, (3 * n) // 5)       # more than half: the cluster spans two slots of every lane even at two points per lane
    nl = (n - c) // 2
    rest = np.concatenate([1 + np.arange(nl) % 97, 101 + np.arange(n - c - nl) % 97]).astype(np.int64)
    rest = rng.permutation(rest)
    tie = np.full(c, 100, np.int64)
    m = np.concatenate([tie, rest] if first else [rest, tie])
    ks = {nl + 1, nl + max(1, c // 2), nl + c - 1}
    ks |= {nl + j for j in (63, 64, 65) if j < c}
    return m, sorted(ks), True


MULTISETS = {
    "distinct": _ms_distinct,
    "classes": _ms_classes,
    "one_class": _ms_one_class,
    "top_byte": _ms_top_byte,
    "mid_byte": _ms_mid_byte,
    "low_byte": _ms_low_byte,
    "ties_first": lambda n, rng: _ties_clustered(n, rng, True),
    "ties_last": lambda n, rng: _ties_clustered(n, rng, False),
}


def multiset_names(N, M):
    """The named multisets a shape carries: all of them; low_byte only where its m of up to 4095 keeps the sum exact."""
    return [n for n in MULTISETS if n != "low_byte" or max(N, M) <= LOW_BYTE_MAX_COUNT]


_cache = {}


def tier_a_case(N, M, name):
    """One Tier A pair.  dict(src fp32 [N,3], tgt fp32 [M,3], d0 / d1 = int64 distances in units of the queries of direction 0
    (target points, M of them) / direction 1 (moved points, N), in point order, ks = the k this multiset targets)."""
    key = (N, M, name)
    if key in _cache:
        return _cache[key]
    n, E = min(N, M), abs(N - M)
    rng = np.random.default_rng([N, M, sorted(MULTISETS).index(name)])
    m, ks, identity = MULTISETS[name](n, rng)
    side = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    idx = np.arange(n, dtype=np.int64)
    site = np.stack([idx % side, (idx // side) % side, idx // (side * side)], 1) * SPACING
    pi = idx if identity else rng.permutation(n)
    src = site.copy()
    src[:, 0] += m
    tgt = site[pi]
    # surplus points on sites 0 .. E-1: the next larger distance class of the multiset, or one past the largest
    vals = np.unique(m)
    nxt = np.searchsorted(vals, m[:E], side="right")
    v = np.where(nxt < len(vals), vals[np.minimum(nxt, len(vals) - 1)], vals[-1] + 1)
    extra = site[:E].copy()
    d0, d1 = m[pi], m
    if M > N:
        extra[:, 0] -= v - m[:E]
        tgt = np.concatenate([tgt, extra])
        d0 = np.concatenate([d0, v])
    elif N > M:
        extra[:, 0] += v
        src = np.concatenate([src, extra])
        d1 = np.concatenate([d1, v])
    assert max(int(d0.max()), int(d1.max())) <= MAX_OFFSET and max(int(d0.sum()), int(d1.sum())) <= SUM_LIMIT, key
    out = dict(src=(src * U).astype(np.float32), tgt=(tgt * U).astype(np.float32), d0=d0, d1=d1,
               ks=[k for k in ks if 1 <= k <= n], src_units=src, tgt_units=tgt)
    assert np.array_equal(out["src"].astype(np.float64) / U, src) and np.array_equal(out["tgt"].astype(np.float64) / U, tgt)
    _cache[key] = out
    return out


def k_values(N, M, targeted=()):
    """The k of a case: 1, 2, the wave edge, half, count-1 and count of EACH direction's count, clipped to [1, min(N, M)], plus
    the k its multisets target."""
    ks = {1, 2, 63, 64, 65, N // 2, N - 1, N, M // 2, M - 1, M} | set(targeted)
    return sorted(k for k in ks if 1 <= k <= min(N, M))


def tier_a_batch(N, M):
    """Every named multiset of a shape as one batch of pairs: (names, src [P,N,3], tgt [P,M,3], ks)."""
    names = multiset_names(N, M)
    cases = [tier_a_case(N, M, n) for n in names]
    ks = k_values(N, M, [k for c in cases for k in c["ks"]])
    return names, np.stack([c["src"] for c in cases]), np.stack([c["tgt"] for c in cases]), ks


def tier_a_params(n, trans_mode, seed=0):
    """[n,8] float64 parameters of the identity pose: V and c arbitrary and positive, a = -0.5 so that theta =
    sin(-pi/2) pi/8 + pi/8 = 0, and s = -0.5 (trans_mode 0: sigma = sin(-pi/2)/8 + 1/8 = 0) or 0 (mode 1).  Positive, because
    the zeros of R = I + 0 A + 0 A^2 and T = chat * 0 carry the signs of A, A^2 and chat: the device keeps a -0 where both
    products are -0 (measured: V = (0.3, -0.7, 0.9) gives R[0][1] = R[1][2] = -0), which moves no point but is not bitwise I;
    with every component of u positive each off-diagonal entry has a +0 product, and T = +0."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.25, 1.0, (n, 8))
    p[:, 3] = -0.5
    p[:, 7] = -0.5 if trans_mode == 0 else 0.0
    return p.astype(np.float32).astype(np.float64)


def expected_cd(d, k):
    """fl32(S u) / fl32(k) of the k smallest of the integer distances d: the one rounding the kernel performs."""
    S = int(np.sort(d, kind="stable")[:k].sum())
    assert S <= SUM_LIMIT
    return np.float32(S * U) / np.float32(k)


def tier_a_expected(case, k):
    """(cd0, cd1, score, loss) as float32 scalars: min with first-wins, loss = fl32(6 * score)."""
    cd0, cd1 = expected_cd(case["d0"], k), expected_cd(case["d1"], k)
    score = cd0 if cd0 <= cd1 else cd1
    return cd0, cd1, score, np.float32(score * np.float32(6.0))


def tier_a_expected_batch(N, M, ks):
    """float32 [len(ks), P, 4] = (cd0, cd1, score, loss) of tier_a_batch(N, M)'s pairs."""
    key = ("exp", N, M, tuple(ks))
    if key not in _cache:
        cases = [tier_a_case(N, M, n) for n in multiset_names(N, M)]
        _cache[key] = np.array([[tier_a_expected(c, k) for c in cases] for k in ks], np.float32)
    return _cache[key]


# ---- NumPy models of the kernels' arithmetic and selection --------------------------------------------------------------------
def sqdist_f32(q_units, r_units):
    """metric_sqdist<0> in fp32 on coordinates given in units: fma(dz, dz, fma(dy, dy, dx * dx)) of the fp32 differences, [Q,R].
    The differences of the fp32 coordinates are formed in fp32; the products and the fused sums are formed exactly in float64
    (integers of units^2 below 2^53) and rounded once, which is what an fma does."""
    q, r = (q_units * U).astype(np.float32), (r_units * U).astype(np.float32)
    d = (r[None, :, :] - q[:, None, :])
    assert d.dtype == np.float32
    d = d.astype(np.float64)
    t = (d[..., 0] * d[..., 0]).astype(np.float32).astype(np.float64)
    t = (d[..., 1] * d[..., 1] + t).astype(np.float32).astype(np.float64)
    return (d[..., 2] * d[..., 2] + t).astype(np.float32)


def keys_of(d_units):
    """fp32 bit patterns of d = m^2 u^2, the radix select's keys."""
    return ((d_units.astype(np.float64) * U) ** 2).astype(np.float32).view(np.uint32)


def radix_model(keys, ksel):
    """houv_solve.h's four passes on the valid keys: (prefix, remaining, neq, distinct digits seen by each pass)."""
    prefix = mask = 0
    remaining, neq, digits = int(ksel), 0, []
    for p in range(4):
        shift = 24 - 8 * p
        live = keys[(keys & np.uint32(mask)) == np.uint32(prefix)]
        hist = np.bincount((live >> np.uint32(shift)) & np.uint32(255), minlength=256)
        c = np.cumsum(hist)
        b = int(np.searchsorted(c, remaining, side="left"))
        remaining -= int(c[b] - hist[b])
        neq = int(hist[b])
        prefix |= b << shift
        mask |= 255 << shift
        digits.append(int(np.count_nonzero(hist)))
    return prefix, remaining, neq, digits


def select_model(keys, ksel, block, mutate=None):
    """How often each key enters the sum under the kernels' selection (0 / 1): everything below the threshold, and the first
    `remaining` of the tied keys in (thread, slot) order, thread = index % block.  `mutate` plants one of the faults the suite
    has to see: "plus_one" / "minus_one" (select k+-1), "wave_local_rank" (the tie rank ignores the other waves' counts),
    "take_all_ties" (the neq == remaining shortcut taken unconditionally), "doubled" (one selected key summed twice)."""
    n = len(keys)
    if mutate == "plus_one":
        ksel = min(n, ksel + 1)
    if mutate == "minus_one":
        ksel = max(1, ksel - 1)
    if ksel >= n:
        take = np.ones(n, np.int64)
    else:
        prefix, remaining, neq, _ = radix_model(keys, ksel)
        take = (keys < prefix).astype(np.int64)
        tied = np.flatnonzero(keys == prefix)
        tied = tied[np.lexsort((tied // block, tied % block))]            # thread-major, then the thread's slots
        if mutate == "take_all_ties" or neq == remaining:
            take[tied] = 1
        elif mutate == "wave_local_rank":
            wave = (tied % block) // 64
            for w in np.unique(wave):
                take[tied[wave == w][:remaining]] = 1
        else:
            take[tied[:remaining]] = 1
    if mutate == "doubled":
        take[np.flatnonzero(take)[0]] += 1
    return take


MUTATIONS = ("plus_one", "minus_one", "wave_local_rank", "take_all_ties", "doubled")


def model_cd(d_units, ksel, block, mutate=None):
    S = int((select_model(keys_of(d_units), ksel, block, mutate) * d_units).sum())
    return np.float32(S * U) / np.float32(ksel)


# ---- Tier A with the view terms (NMET = 4): N == M, offsets (m, m, m) u, m a power of 8 --------------------------------------
VIEW_CLASSES = [1, 8, 64, 512]
# One size per row of the variant table up to <1024,3>.  <1024,4> (3073..4096 points) has no size: the comparison's bound grows
# as k while the cheapest swap across a cut inside a class that holds a share f of the points moves the sum by about 1 / (f k),
# and four times (k+1) 2^-24 overtakes that near k = 2000 f^-1/2; its selection is Tier A's without views, bit for bit.
VIEW_SIZES = [40, 64, 200, 300, 700, 1024, 1100, 2048, 2500]
VIEW_PATTERNS = ("classes", "one_class", "ties_first", "ties_last")


def tier_a_view_case(N, pattern):
    """dict(src, tgt fp32 [N,3], m int64 [N] in point order (both directions: pi is the identity), ks)."""
    key = ("view", N, pattern)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([N, VIEW_PATTERNS.index(pattern)])
    if pattern == "classes":
        m = _spread(N, VIEW_CLASSES, rng)
        ks = sorted(set(_class_cuts(m, 1) + _class_cuts(m, 2)))
    elif pattern == "one_class":
        m, ks = np.full(N, 8, np.int64), []
    else:
        c = max(2, (3 * N) // 5)
        nl = (N - c) // 2
        rest = rng.permutation(np.concatenate([np.full(nl, 1), np.full(N - c - nl, 512)]).astype(np.int64))
        tie = np.full(c, 64, np.int64)
        m = np.concatenate([tie, rest] if pattern == "ties_first" else [rest, tie])
        ks = sorted({nl + 1, nl + max(1, c // 2), nl + c - 1} | {nl + j for j in (63, 64, 65) if j < c})
    side = int(np.ceil(N ** (1.0 / 3.0) - 1e-9))
    idx = np.arange(N, dtype=np.int64)
    site = np.stack([idx % side, (idx // side) % side, idx // (side * side)], 1) * SPACING
    src = site + m[:, None]
    out = dict(src=(src * U).astype(np.float32), tgt=(site * U).astype(np.float32), m=m, ks=[k for k in ks if 1 <= k <= N],
               src_units=src, tgt_units=site)
    _cache[key] = out
    return out


def view_expected64(case, k_full, k_view):
    """float64 [4,2] = cd of every metric and direction (0 over the target points, 1 over the moved points).  Full metric:
    sqrt(3) m u of the point's own site either way.  A view drops one axis, which projects every site of a grid line along that
    axis onto one point: a moved point still finds sqrt(2) m u (its own m: the targets of its line coincide), a target point
    finds the smallest m of its line."""
    m, site = case["m"], case["tgt_units"] // SPACING
    out = np.empty((4, 2))
    full = np.sort(m.astype(np.float64)) * U
    out[0, :] = np.sqrt(3.0) * full[:k_full].sum() / k_full
    for ax in range(3):
        keep = [a for a in range(3) if a != ax]
        line = site[:, keep[0]] * (site.max() + 1) + site[:, keep[1]]
        lo = np.full(line.max() + 1, np.iinfo(np.int64).max)
        np.minimum.at(lo, line, m)
        out[1 + ax, 0] = np.sqrt(2.0) * (np.sort(lo[line].astype(np.float64)) * U)[:k_view].sum() / k_view
        out[1 + ax, 1] = np.sqrt(2.0) * full[:k_view].sum() / k_view
    return out


def view_bound(k):
    """Relative bound of a term: k-1 additions, one root and one division of non-negative terms, half an ulp each."""
    return (k + 1) * 2.0 ** -24


def view_swap_margin(m, k):
    """Smallest non-zero relative change of the float64 sum when one point is swapped across the cut at k (inf when no swap
    changes it: k == count, or one class)."""
    s = np.sort(m.astype(np.float64))
    if k >= len(s):
        return np.inf
    S, thr, nxt = s[:k].sum(), s[k - 1], s[k]
    cands = []
    above = s[k:][s[k:] > thr]
    if len(above):
        cands.append(above.min() - s[:k][s[:k] < above.min()].max())     # the cheapest exchange with a higher class
    if nxt == thr:                                                        # tied points outside: swap one in for a lower one
        below = s[:k][s[:k] < thr]
        if len(below):
            cands.append(thr - below.max())
    return min(cands) / S if cands else np.inf


# ---- Tier B: generic poses and clouds ------------------------------------------------------------------------------------------
# (N, M, use_views, k_view or None, path): path "lds" = houv_solve_iterate, "large" = houv_solve_iterate_large
TIER_B_CASES = [(200, 200, False, None, "lds"), (300, 512, False, None, "lds"), (2048, 2048, False, None, "lds"),
                (4500, 4500, False, None, "large")]
VIEW_CORNER_CASES = [(40, 64, 40), (300, 512, 200)]        # (N, M, k_view): use_views with N != M and k_view < max(N, M)
TIER_B_HYPOTHESES = 3


def tier_b_inputs(N, M, seed=77):
    """(src fp32 [P,N,3], tgt fp32 [P,M,3], params float64 [P,8] of fp32 values) as test_single_forward_backward_vs_oracle
    draws them."""
    from houv_amd import synthetic
    P = TIER_B_HYPOTHESES
    src, tgt, _ = synthetic.make_pairs(P, max(N, M), seed=seed)
    src, tgt = src[:, :N].contiguous().numpy(), tgt[:, :M].contiguous().numpy()
    params = np.random.default_rng(N + M).standard_normal((P, 8)).astype(np.float32).astype(np.float64)
    return src, tgt, params


def nn_sqdists(src, tgt, R, T, dtype, views):
    """The restatement: moved = src R^T + T, then the brute-force squared nearest-neighbour distance of every query, per metric
    (0 full; 1..3 with x / y / z dropped) and direction (0 over the target points, 1 over the moved points), all in `dtype`.
    Returns list over metrics of (d_dir0 [M], d_dir1 [N])."""
    s, t = src.astype(dtype), tgt.astype(dtype)
    Rd, Td = R.astype(dtype), T.astype(dtype)
    # written out (no BLAS call): every rounding is an IEEE operation of `dtype` in a fixed order, the same on every host
    mv = (s[:, 0:1] * Rd[:, 0] + s[:, 1:2] * Rd[:, 1]) + s[:, 2:3] * Rd[:, 2] + Td
    out = []
    for met in range(4 if views else 1):
        keep = [a for a in range(3) if a != met - 1]
        d0 = np.full(len(t), np.inf, dtype)
        d1 = np.empty(len(mv), dtype)
        for a0 in range(0, len(mv), 512):                      # chunks of moved points keep the temporaries small
            diff = mv[a0:a0 + 512, None, keep] - t[None, :, keep]
            d = (diff * diff).sum(-1, dtype=dtype)
            d1[a0:a0 + 512] = d.min(1)
            d0 = np.minimum(d0, d.min(0))
        out.append((d0, d1))
    return out


def cd_of(dists, ks):
    """[len(dists), 2]: mean root of the ks[m] smallest (a stable sort) squared distances of each metric and direction."""
    return np.array([[np.sqrt(np.sort(d, kind="stable")[:k]).sum(dtype=d.dtype) / d.dtype.type(k) for d in pair]
                     for pair, k in zip(dists, ks)])


def cd_reference(src, tgt, R, T, views):
    """The squared-distance lists of one hypothesis in float64 and float32: (d64, d32) for cd_of."""
    return nn_sqdists(src, tgt, R, T, np.float64, views), nn_sqdists(src, tgt, R, T, np.float32, views)


def tier_b_bound_and_gap(d64, d32, k_full, k_view, count_min):
    """(reference cd [nmet,2] float64, 4 x |f32 - f64| maximum, the smallest half gap to the selections k-1 / k+1)."""
    nmet = len(d64)
    ks = [k_full] + [k_view] * (nmet - 1)
    ref = cd_of(d64, ks)
    loss32 = np.abs(cd_of(d32, ks).astype(np.float64) - ref).max()
    gap = np.inf
    for dk in (-1, 1):
        for m in range(nmet):
            k2 = list(ks)
            k2[m] += dk
            if 1 <= k2[m] <= count_min:
                gap = min(gap, np.abs(cd_of(d64, k2)[m] - ref[m]).min())
    return ref, 4.0 * loss32, 0.5 * gap


def oracle_nn(src, tgt, params, base, trans_mode, views):
    """The oracle's float64 search, once per case (it does not depend on k): per metric (idx_gt [P,M] into the moved cloud,
    idx_out [P,N] into the target), as calc_cd_percent / loss_view call the Chamfer op: (gt, output)."""
    import torch
    from oracle import houv_ref_cpu as orc
    T_ = torch.tensor
    tv = [T_(params[:, a:b].astype(np.float32)) for a, b in ((0, 3), (3, 4), (4, 7), (7, 8))]
    with torch.no_grad():
        moved, _, _ = orc.houv_forward(T_(src), *tv, base, "houv" if trans_mode == 0 else "solve")
        out = []
        for met in range(4 if views else 1):
            keep = torch.ones(3)
            if met:
                keep[met - 1] = 0
            _, _, i_gt, i_out = orc.chamfer_nn_chunked(T_(tgt) * keep, moved * keep, chunk=1)
            out.append((i_gt.long(), i_out.long()))
    return out


def oracle_terms(src, tgt, params, base, trans_mode, views, k_full, k_view, nn):
    """The autograd oracle of tests/test_gpu_solve.py's `_oracle_terms` with the top-k sizes as arguments: the eight (or two)
    terms, loss and the parameter gradient of loss.mean() for P hypotheses (K = 1).  `nn` = oracle_nn of the same inputs: the
    distances are re-formed from the float64 search's neighbours (as the Chamfer op's backward does), so a sweep over k pays for
    one search."""
    import torch
    from oracle import houv_ref_cpu as orc
    T_ = torch.tensor
    tv = [T_(params[:, 0:3].astype(np.float32), requires_grad=True), T_(params[:, 3:4].astype(np.float32), requires_grad=True),
          T_(params[:, 4:7].astype(np.float32), requires_grad=True), T_(params[:, 7:8].astype(np.float32), requires_grad=True)]
    moved, R, Tt = orc.houv_forward(T_(src), *tv, base, "houv" if trans_mode == 0 else "solve")
    tg = T_(tgt)
    cds, loss = [], 0
    for met, (i_gt, i_out) in enumerate(nn):
        keep = torch.ones(3)
        if met:
            keep[met - 1] = 0
        a, b = (moved * keep).double(), (tg * keep).double()
        k = k_full if met == 0 else k_view
        d_gt = ((b - torch.gather(a, 1, i_gt.unsqueeze(2).expand(-1, -1, 3))) ** 2).sum(2).float()
        d_out = ((a - torch.gather(b, 1, i_out.unsqueeze(2).expand(-1, -1, 3))) ** 2).sum(2).float()
        d_gt, _ = d_gt.topk(k, dim=1, largest=False, sorted=True)
        d_out, _ = d_out.topk(k, dim=1, largest=False, sorted=True)
        cds.append((torch.sqrt(d_gt).mean(1), torch.sqrt(d_out).mean(1)))
        loss = loss + torch.minimum(*cds[-1]) * (6 if met == 0 else 1)
    loss.mean().backward()
    return dict(cd=np.stack([np.stack([c[0].detach().numpy(), c[1].detach().numpy()], 1) for c in cds], 1),
                loss=loss.detach().numpy(), grads=np.concatenate([t.grad.numpy() for t in tv], 1))
