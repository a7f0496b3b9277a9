"""CPU proof of tests/solve_select_cases.py: the Tier A construction is exact, every named multiset reaches the branch of the
radix select it names, the expected values see the faults a selection can have, and Tier B's bounds cannot hide an off-by-one
selection.  tests/test_gpu_solve_select.py then holds the kernels to these values."""
import numpy as np
import pytest

import solve_select_cases as sc

# the shapes of the prototype plus the smallest in-LDS ones: brute force in the fp32 model of the kernel's distance expression
BRUTE_SHAPES = [(300, 300), (300, 340), (340, 300), (1100, 1100), (900, 1024), (40, 40), (35, 40), (64, 56)]
ALL_SHAPES = sc.inlds_shapes() + sc.LARGE_SHAPES


def _names(N, M):
    return sc.multiset_names(N, M)


@pytest.mark.parametrize("N,M", BRUTE_SHAPES)
def test_tier_a_minima_roots_and_sums_are_exact(N, M):
    """Per direction: the fp32 minimum of metric_sqdist<0> over all references equals m^2 u^2 of the construction (its float64
    value), is attained by one reference only, its fp32 root is m u, and the fp32 sum of the roots is the integer sum of m in
    any order."""
    rng = np.random.default_rng(N * 7 + M)
    for name in _names(N, M):
        c = sc.tier_a_case(N, M, name)
        for q, r, d in ((c["tgt_units"], c["src_units"], c["d0"]), (c["src_units"], c["tgt_units"], c["d1"])):
            sq = sc.sqdist_f32(q, r)
            mn = sq.min(1)
            want = (d.astype(np.float64) * sc.U) ** 2
            assert np.array_equal(mn.astype(np.float64), want), name
            assert ((sq == mn[:, None]).sum(1) == 1).all(), name                      # unique nearest neighbours
            root = np.sqrt(mn)
            assert root.dtype == np.float32 and np.array_equal(root.astype(np.float64), d * sc.U), name
            total = float(d.sum()) * sc.U
            assert root.astype(np.float64).sum() == total
            for _ in range(5):
                o = rng.permutation(len(root))
                assert float(np.cumsum(root[o], dtype=np.float32)[-1]) == total, name       # sequential fp32 sum in a random order
            assert float(root.sum(dtype=np.float32)) == total                                # pairwise


@pytest.mark.parametrize("N,M", ALL_SHAPES)
def test_tier_a_keys_and_limits(N, M):
    """At every shape, the large ones included: the coordinates are fp32-exact multiples of u (asserted by the builder), the
    offsets stay below a quarter of the spacing, each direction's sum stays at or below 2^24 units, m^2 < 2^24 so that d is
    exact, and the fp32 root of every key is m u."""
    for name in _names(N, M):
        c = sc.tier_a_case(N, M, name)
        assert c["src"].shape == (N, 3) and c["tgt"].shape == (M, 3) and len(c["d0"]) == M and len(c["d1"]) == N
        for d in (c["d0"], c["d1"]):
            assert d.min() >= 1 and d.max() <= sc.MAX_OFFSET and d.sum() <= sc.SUM_LIMIT
            key = sc.keys_of(d)
            assert np.array_equal(np.sqrt(key.view(np.float32)).astype(np.float64), d * sc.U)
        # both clouds are sets: no two points coincide
        assert len(np.unique(c["src_units"], axis=0)) == N and len(np.unique(c["tgt_units"], axis=0)) == M


@pytest.mark.parametrize("N,M", ALL_SHAPES)
def test_every_multiset_hits_the_branch_it_names(N, M):
    """The radix model (four 8-bit passes on the keys) agrees with a sort about the threshold, `remaining` and `neq` at every
    k of the case, and each named multiset shows the digit pattern and the cut it is there for."""
    from houv_amd import _lib
    names, _, _, ks = sc.tier_a_batch(N, M)
    n = min(N, M)
    for name in names:
        c = sc.tier_a_case(N, M, name)
        seen = set()
        for dname, count in (("d0", M), ("d1", N)):
            d = c[dname]
            keys, srt = sc.keys_of(d), np.sort(d)
            for k in ks:
                prefix, remaining, neq, digits = sc.radix_model(keys, k)
                thr = srt[k - 1]
                assert prefix == int(sc.keys_of(np.array([thr]))[0])
                assert neq == int((d == thr).sum()) and remaining == k - int((d < thr).sum()) and 1 <= remaining <= neq
                if k in c["ks"] and count == n:
                    seen.add("end" if remaining == neq else "first" if remaining == 1 else "last" if remaining == neq - 1 else "mid")
            if count != n:
                continue          # the digit patterns are those of the direction without surplus points
            _, _, _, digits = sc.radix_model(keys, max(1, n // 2))
            if name == "one_class":
                assert digits == [1, 1, 1, 1]
            if name == "top_byte":
                assert digits[0] == min(6, n) and digits[1:] == [1, 1, 1]
                assert len(np.unique(keys & np.uint32(0x00FFFFFF))) == 1
            if name == "mid_byte":
                assert digits[0] == 1 and digits[1] == 4 and digits[2:] == [1, 1]
                assert len(np.unique(keys & np.uint32(0xFF00FFFF))) == 1
            if name == "low_byte":
                assert digits[:2] == [1, 1] and digits[2] > 1
                assert len(np.unique(keys >> np.uint32(16))) == 1 and len(np.unique(keys & np.uint32(255))) > 1
            if name == "distinct" and n < sc.MAX_OFFSET:
                assert len(np.unique(d)) == n
        if name == "classes":
            assert {"end", "first", "mid"} <= seen and ("last" in seen or n < 16)
        if name in ("ties_first", "ties_last"):
            d = c["d1"][:n]
            tied = np.flatnonzero(d == 100)
            assert np.array_equal(tied, np.arange(len(tied)) + (0 if name == "ties_first" else n - len(tied)))
            assert np.array_equal(c["d0"][:n], d)                                     # both directions see the cluster in place
            assert "end" not in seen and len(seen) >= 2
            # the rank of the tied keys crosses waves and, with more than one point per lane, slots (chunks in the large kernel)
            block, q = _lib.solve_variant(N, M) if max(N, M) <= 4096 else (sc.LARGE_BLOCK, 4)
            thread = tied % block
            if len(tied) > 64:
                assert len(np.unique(thread // 64)) >= 2
            if q > 1 and n == block * q:
                assert len(np.unique(tied // block)) >= 2 and (np.bincount(thread) >= 2).any()


@pytest.mark.parametrize("N,M", ALL_SHAPES)
def test_winner_direction(N, M):
    """M > N: direction 0 (over the target) wins or ties; N > M: direction 1 wins or ties, strictly somewhere; N == M: a tie,
    which the tail's first-wins rule gives to direction 0."""
    names, _, _, ks = sc.tier_a_batch(N, M)
    exp = sc.tier_a_expected_batch(N, M, ks)
    cd0, cd1, score, loss = exp[..., 0], exp[..., 1], exp[..., 2], exp[..., 3]
    assert np.array_equal(score, np.where(cd0 <= cd1, cd0, cd1)) and np.array_equal(loss, score * np.float32(6))
    if M > N:
        assert (cd0 <= cd1).all()
    elif N > M:
        assert (cd1 <= cd0).all() and (cd1 < cd0).any()
        assert (cd1 < cd0).any(0).sum() >= len(names) - 1      # strictly for every multiset whose surplus enters some selection
    else:
        assert np.array_equal(cd0, cd1)


def test_every_variant_row_has_a_full_and_a_partial_size():
    from houv_amd import _lib
    rows = {}
    for full, part in sc.INLDS_ROWS:
        b, q = _lib.solve_variant(full, full)
        assert _lib.solve_variant(part, part) == (b, q) and full == b * q and part < full and part % 64 != 0
        assert _lib.solve_variant(full + 1, full + 1) != (b, q) if full < 4096 else True
        rows[(b, q)] = (full, part)
    table = {_lib.solve_variant(n, n) for n in range(1, 4097)}
    assert table == set(rows)
    for N, M in sc.inlds_shapes():                              # the N != M pairs stay inside their row
        assert _lib.solve_variant(N, M) == _lib.solve_variant(max(N, M), max(N, M))
        assert _lib.solve_variant(N, M) in rows


@pytest.mark.parametrize("N,M", [(40, 40), (300, 300), (340, 300), (1100, 1100), (2048, 1792), (4097, 4097), (5000, 6000)])
def test_expected_values_see_planted_faults(N, M):
    """The NumPy model of the selection reproduces the constructed value, and each planted fault -- a select that is off by
    one, a tie rank that ignores the other waves, the shortcut for `neq == remaining` taken always, a doubled point -- changes
    the expected value wherever it changes the selection."""
    from houv_amd import _lib
    block = _lib.solve_variant(N, M)[0] if max(N, M) <= 4096 else sc.LARGE_BLOCK
    names, _, _, ks = sc.tier_a_batch(N, M)
    hits = {m: 0 for m in sc.MUTATIONS}
    for name in names:
        c = sc.tier_a_case(N, M, name)
        for d, count in ((c["d0"], M), (c["d1"], N)):
            for k in ks:
                want = sc.expected_cd(d, k)
                assert sc.model_cd(d, k, block) == want
                assert sc.select_model(sc.keys_of(d), k, block).sum() == k
                for mut in sc.MUTATIONS:
                    same = np.array_equal(sc.select_model(sc.keys_of(d), k, block, mut), sc.select_model(sc.keys_of(d), k, block))
                    got = sc.model_cd(d, k, block, mut)
                    if not same and got != want:
                        hits[mut] += 1
                    if mut in ("plus_one", "doubled") and not same:
                        # one more point of at least one unit: S grows, and S u / k moves unless it rounds away
                        assert got >= want
                if 1 < k < count:
                    # the off-by-one selections are seen at EVERY k: they move S by at least one unit of <= 2^24
                    assert sc.model_cd(d, k, block, "plus_one") != want or sc.model_cd(d, k, block, "minus_one") != want
    assert all(v > 0 for m, v in hits.items() if m != "wave_local_rank" or block > 64), hits


@pytest.mark.parametrize("N", sc.VIEW_SIZES)
def test_view_cases_margins(N):
    """NMET = 4 under ties: d = 3 m^2 u^2 and 2 m^2 u^2 are exact in fp32 (checked in the distance model at the small sizes),
    and swapping any one point across the cut moves the float64 value by at least four times the bound of the comparison."""
    for pattern in sc.VIEW_PATTERNS:
        c = sc.tier_a_view_case(N, pattern)
        m = c["m"]
        assert set(np.unique(m)) <= set(sc.VIEW_CLASSES) and m.sum() <= sc.SUM_LIMIT
        if N <= 1100:
            for q, r in ((c["tgt_units"], c["src_units"]), (c["src_units"], c["tgt_units"])):
                mn = sc.sqdist_f32(q, r).min(1)
                assert np.array_equal(mn.astype(np.float64), 3.0 * (m * sc.U) ** 2)
            # the eight expected terms against a brute-force float64 search on the integer coordinates (all points in a view)
            want = sc.view_expected64(c, max(1, N // 2), N)
            for ax in range(3):
                keep = [a for a in range(3) if a != ax]
                d = ((c["tgt_units"][:, None, keep] - c["src_units"][None, :, keep]) ** 2).sum(-1)        # [target, moved], exact
                assert d.max() < 2 ** 53 and set(np.unique(d.min(0))) <= {2 * v * v for v in sc.VIEW_CLASSES}
                got = [np.sqrt(d.min(1).astype(np.float64)).mean() * sc.U, np.sqrt(d.min(0).astype(np.float64)).mean() * sc.U]
                np.testing.assert_allclose(want[1 + ax], got, rtol=1e-13)
        for k in sc.k_values(N, N, c["ks"]):
            assert sc.view_swap_margin(m, k) >= 4 * sc.view_bound(k), (pattern, k)
        assert sc.view_swap_margin(m, N) == np.inf
        # the margin function itself: brute force over all single swaps at one cut
        k = max(1, N // 2)
        s = np.sort(m.astype(np.float64))
        S = s[:k].sum()
        deltas = {abs(b - a) for a in np.unique(s[:k]) for b in np.unique(s[k:])} - {0.0}
        assert sc.view_swap_margin(m, k) == (min(deltas) / S if deltas else np.inf)


_tier_b = {}


def _tier_b_lists(N, M, views):
    """Squared-distance lists of every hypothesis under the oracle's fp32 R, T (the kernels' own differ in the last bit)."""
    key = (N, M, views)
    if key not in _tier_b:
        import torch
        from oracle import houv_ref_cpu as orc
        src, tgt, params = sc.tier_b_inputs(N, M)
        tv = [torch.tensor(params[:, a:b].astype(np.float32)) for a, b in ((0, 3), (3, 4), (4, 7), (7, 8))]
        _, R, T = orc.houv_forward(torch.tensor(src), *tv, 1, "houv")
        _tier_b[key] = [sc.cd_reference(src[h], tgt[h], R[h].numpy(), T[h, 0].numpy(), views) for h in range(len(src))]
    return _tier_b[key]


@pytest.mark.parametrize("N,M,views,k_view,path", sc.TIER_B_CASES + [(n, m, True, kv, "lds") for n, m, kv in sc.VIEW_CORNER_CASES])
def test_tier_b_bound_is_below_half_the_gap_to_the_neighbouring_selections(N, M, views, k_view, path):
    """For every k of the sweep: 4x the float32 restatement's loss against float64 is at most half of
    min(|cd(k) - cd(k-1)|, |cd(k) - cd(k+1)|) of the float64 reference, for every hypothesis and term."""
    lists = _tier_b_lists(N, M, views)
    ks = sc.k_values(N, M) if not views else [N // 2]
    worst = (0.0, None)
    for k in ks:
        bound, gap = 0.0, np.inf
        for d64, d32 in lists:
            _, b, g = sc.tier_b_bound_and_gap(d64, d32, k, k_view if views else k, min(N, M))
            bound, gap = max(bound, b), min(gap, g)
        print(f"tier B ({N},{M},views={views}) k={k}: bound {bound:.3e} half gap {gap:.3e}")
        assert bound <= gap, (k, bound, gap)
        worst = max(worst, (bound / gap, k))
    print("worst bound / half gap:", worst)
