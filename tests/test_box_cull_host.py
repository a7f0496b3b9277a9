"""CPU: the group cull of the pruned solve's box tests (houv::box_test_group, houv_amd/csrc/houv_math.h) against the per-query
test it stands in front of (houv::box_test_query, the host restatement of prune_masks' test), host-compiled (tests/boxcull).
The property the kernel relies on, in fp32 and with ZERO exceptions: a box that fails the group test fails the test of every
query of the group.  Draws that straddle the threshold are constructed with exactly representable geometry, so that the
expected verdicts come from integer arithmetic; elsewhere both tests must agree with a float64 restatement wherever the margin
is clear (relative 1e-5: fp32 rounds each of the five operations of a distance to 6e-8)."""
import numpy as np

from tests import boxcull

MSETS = [15, 13, 11, 6, 12, 1, 8]


def _f64_dist(off):
    """[..., 3] non-negative offsets -> [..., 4] squared distances per metric (0: 3-D, 1 / 2 / 3: x / y / z dropped)."""
    sq = off.astype(np.float64) ** 2
    return np.stack([sq.sum(-1), sq[..., 1] + sq[..., 2], sq[..., 0] + sq[..., 2], sq[..., 0] + sq[..., 1]], -1)


def _f64_verdicts(c):
    """float64 restatement -> (query pass [n, 64], clear [n, 64], group pass [n], clear [n]); finite inputs only."""
    q, ub = c["q"].astype(np.float64), c["ub"].astype(np.float64)
    L = np.minimum(c["lo"], c["hi"]).astype(np.float64)[:, None, :]
    H = np.maximum(c["lo"], c["hi"]).astype(np.float64)[:, None, :]
    lanes = np.arange(64)[None, :] < c["count"][:, None]
    ub = np.where(lanes[..., None], ub, -1.0)
    use = ((c["mset"][:, None] >> np.arange(4)[None, :]) & 1).astype(bool)
    use &= np.arange(4)[None, :] < c["nmet"][:, None]

    def verdict(s, b):
        margin = 1e-5 * (np.abs(s) + np.abs(b)) + 1e-30
        ok = (s <= b) & use[:, None, :]
        clear = (np.abs(s - b) > margin) | ~use[:, None, :]
        return ok.any(-1), clear.all(-1)

    qp, qc = verdict(_f64_dist(np.maximum(np.maximum(L - q, q - H), 0.0)), ub)
    qv = np.where(lanes[..., None], q, np.nan)
    glo, ghi = np.nanmin(qv, 1, keepdims=True), np.nanmax(qv, 1, keepdims=True)
    gp, gc = verdict(_f64_dist(np.maximum(np.maximum(L - ghi, glo - H), 0.0)), ub.max(1, keepdims=True))
    return qp, qc, gp[:, 0], gc[:, 0]


def _lanes(v):
    return ((v["lanes"][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def _assert_cull_is_exact(c, v, what):
    bad = (v["group"] == 0) & (v["lanes"] != 0)
    print(f"{what}: {len(c)} cases, group fails {int((v['group'] == 0).sum())}, group passes with no lane passing "
          f"{int(((v['group'] == 1) & (v['lanes'] == 0)).sum())}, violations {int(bad.sum())}")
    assert not bad.any(), f"{what}: case {int(np.flatnonzero(bad)[0])}: the group test fails a box that a query passes"


def _random_cases(rng, n, nmet, mset, spread):
    """Groups of 64 queries in a cube of side `spread` somewhere in the unit cube, a box nearby, bounds about the true distance."""
    c = boxcull.cases(n, nmet=nmet, mset=mset)
    centre = rng.uniform(-1, 1, (n, 1, 3))
    c["q"] = (centre + rng.uniform(-0.5, 0.5, (n, 64, 3)) * spread).astype(np.float32)
    bc = centre[:, 0] + rng.normal(0, 1, (n, 3)) * rng.choice([0.05, 0.3, 1.0], (n, 1))
    half = rng.uniform(0, 0.2, (n, 3)) * rng.choice([0.0, 1.0], (n, 1), p=[0.1, 0.9])
    c["lo"], c["hi"] = (bc - half).astype(np.float32), (bc + half).astype(np.float32)
    swap = rng.random((n, 3)) < 0.05                      # v_med3 takes a box's bounds in either order
    c["lo"], c["hi"] = np.where(swap, c["hi"], c["lo"]), np.where(swap, c["lo"], c["hi"])
    L, H = np.minimum(c["lo"], c["hi"])[:, None], np.maximum(c["lo"], c["hi"])[:, None]
    d = _f64_dist(np.maximum(np.maximum(L - c["q"], c["q"] - H), 0.0))
    # bounds: the true distances of the group scaled around 1, so that group and query verdicts both mix
    c["ub"] = (d.min(1, keepdims=True) * rng.choice([0.25, 0.9, 0.99999, 1.0, 1.00001, 1.1, 4.0], (n, 1, 1)) *
               rng.uniform(0.5, 1.0, (n, 64, 4))).astype(np.float32)
    return c


def test_a_box_the_group_test_fails_is_failed_by_every_query_random_groups_in_fp32():
    rng = np.random.default_rng(20251)
    seen_fail = seen_pass = 0
    for nmet, mset in [(4, m) for m in MSETS] + [(1, 1)]:
        for spread in (0.02, 0.2, 1.0):
            c = _random_cases(rng, 4000, nmet, mset, spread)
            c["count"] = rng.choice([64, 64, 64, 1, 17, 33, 63], len(c))
            v = boxcull.verdicts(c)
            _assert_cull_is_exact(c, v, f"nmet {nmet} mset {mset} spread {spread}")
            seen_fail += int((v["group"] == 0).sum())
            seen_pass += int((v["lanes"] != 0).sum())
            assert not (_lanes(v) & (np.arange(64)[None, :] >= c["count"][:, None])).any(), "a lane past the cloud's end passes"
    assert seen_fail > 10000 and seen_pass > 10000, (seen_fail, seen_pass)


def test_both_tests_agree_with_float64_where_the_margin_is_clear():
    rng = np.random.default_rng(20252)
    for nmet, mset in [(4, 15), (4, 13), (4, 6), (1, 1)]:
        c = _random_cases(rng, 6000, nmet, mset, 0.2)
        c["count"] = rng.choice([64, 40], len(c))
        v = boxcull.verdicts(c)
        qp, qc, gp, gc = _f64_verdicts(c)
        got = _lanes(v)
        print(f"nmet {nmet} mset {mset}: clear query verdicts {int(qc.sum())} of {qc.size}, clear group verdicts {int(gc.sum())} of {gc.size}")
        assert qc.mean() > 0.5 and gc.mean() > 0.5, "the draws are meant to leave most verdicts clear of the threshold"
        assert (got == qp)[qc].all(), "per-query test against float64"
        assert ((v["group"] == 1) == gp)[gc].all(), "group test against float64"
        # the group the program formed is the float64 one: min / max select, they do not round
        qv = np.where((np.arange(64)[None, :] < c["count"][:, None])[..., None], c["q"], np.nan)
        assert np.array_equal(v["glo"], np.nanmin(qv, 1)) and np.array_equal(v["ghi"], np.nanmax(qv, 1))


def _ulp_neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def test_bounds_at_the_distance_to_the_last_bit_and_its_one_ulp_neighbours():
    """Integer coordinates: every difference, square and sum is exact in fp32, so the distances are known integers.  The box is
    [10, 12]^3; the group's corner nearest to it is (7, 6, 8): gaps (3, 4, 2), group distances 29 / 20 / 13 / 25."""
    lo, hi = (10, 10, 10), (12, 12, 12)
    pts = [(7, 6, 8), (5, 6, 8), (7, 2, 8), (7, 6, 1), (1, 1, 1), (7, 6, 8)]
    gd = [29.0, 20.0, 13.0, 25.0]
    for nmet, msets in ((4, [1, 2, 4, 8]), (1, [1])):
        for mset in msets:
            m = mset.bit_length() - 1
            bounds = _ulp_neighbours(gd[m])
            c = boxcull.cases(len(bounds), nmet=nmet, mset=mset, count=len(pts))
            c["q"][:, :len(pts)] = np.array(pts, dtype=np.float32)
            c["lo"], c["hi"] = lo, hi
            c["ub"][:] = 1e30                                     # the other metrics are not in the set: never looked at
            for i, b in enumerate(bounds):
                c["ub"][i, :, m] = b
            v = boxcull.verdicts(c)
            assert list(v["group"]) == [0, 1, 1], (mset, v["group"])
            # the queries' own distances, in integers: 0 and 5 sit on the group's corner, the others are farther on one axis
            off = np.maximum(np.array(lo) - np.array(pts), 0) ** 2
            dist = [off.sum(1), off[:, 1] + off[:, 2], off[:, 0] + off[:, 2], off[:, 0] + off[:, 1]][m]
            want = [sum(1 << i for i, d in enumerate(dist) if float(d) <= float(b)) for b in bounds]
            assert want[0] == 0 and want[1] & 0b100001 == 0b100001
            assert list(v["lanes"]) == want, (mset, v["lanes"], want)
    # the bound that decides is the LARGEST of the group: lower every lane's but one below the distance -> that lane's survives
    c = boxcull.cases(2, mset=1, count=len(pts))
    c["q"][:, :len(pts)] = np.array(pts, dtype=np.float32)
    c["lo"], c["hi"] = lo, hi
    c["ub"][:, :, 0] = 28.0
    c["ub"][1, 4, 0] = 29.0                                       # lane 4 is far away: passes nothing, but lifts the group's bound
    v = boxcull.verdicts(c)
    assert list(v["group"]) == [0, 1] and list(v["lanes"]) == [0, 0]


def test_queries_on_a_box_face_and_degenerate_boxes():
    # a query ON a face has offset 0 on that axis; inside the box all three are 0: passes with bound 0, not with bound -1
    c = boxcull.cases(4, mset=15, count=3)
    c["q"][:, :3] = np.array([(10, 11, 11), (12, 10, 12), (11, 11, 11)], dtype=np.float32)
    c["lo"], c["hi"] = (10, 10, 10), (12, 12, 12)
    c["ub"][0], c["ub"][1] = 0.0, -1.0
    c["lo"][2], c["hi"][2], c["ub"][2] = (12, 10, 10), (12, 12, 12), 0.0        # a flat box: the group touches it
    c["lo"][3], c["hi"][3], c["ub"][3] = (13, 10, 10), (13, 12, 12), 0.0        # a flat box one away: only the views without x reach it
    c["mset"][2:] = 1                                                           # the 3-D distance alone
    v = boxcull.verdicts(c)
    assert list(v["group"]) == [1, 0, 1, 0] and list(v["lanes"]) == [0b111, 0, 0b010, 0], (v["group"], v["lanes"])
    c["mset"][3] = 15
    v = boxcull.verdicts(c)
    assert v["group"][3] == 1 and v["lanes"][3] == 0b111
    # all points equal: the group box and the reference box are points
    c = boxcull.cases(3, mset=15, count=64)
    c["q"][:] = np.float32(0.3)
    c["lo"][:] = c["hi"][:] = np.float32(0.3)
    c["lo"][1:] = c["hi"][1:] = np.float32(0.5)
    d = np.float32(0.5) - np.float32(0.3)
    s1 = np.float32(d * d) + np.float32(d * d)                     # a view's distance (one rounding of the fma: d*d is exact in float64)
    c["ub"][0], c["ub"][1], c["ub"][2] = 0.0, np.float32(np.float64(d) ** 2 * 2), np.nextafter(np.float32(np.float64(d) ** 2 * 2), np.float32(0))
    v = boxcull.verdicts(c)
    full = (1 << 64) - 1
    assert list(v["group"]) == [1, 1, 0] and list(v["lanes"]) == [full, full, 0], (v["group"], v["lanes"], s1)
    _assert_cull_is_exact(c, v, "degenerate boxes")


def test_nan_and_inf_coordinates_and_bounds_and_partly_filled_groups():
    rng = np.random.default_rng(20253)
    c = _random_cases(rng, 12000, 4, 15, 0.2)
    n = len(c)
    kind = rng.integers(0, 8, n)
    lane = rng.integers(0, 64, n)
    idx = np.arange(n)
    sel = kind == 0; c["q"][idx[sel], lane[sel], rng.integers(0, 3, sel.sum())] = np.nan
    sel = kind == 1; c["q"][idx[sel], lane[sel], rng.integers(0, 3, sel.sum())] = rng.choice([np.inf, -np.inf], sel.sum())
    sel = kind == 2; c["ub"][idx[sel], lane[sel], rng.integers(0, 4, sel.sum())] = np.nan
    sel = kind == 3; c["ub"][idx[sel], lane[sel], rng.integers(0, 4, sel.sum())] = np.inf
    sel = kind == 4; c["ub"][sel] = np.nan                                     # every bound NaN: nothing passes
    sel = kind == 5; c["q"][sel] = np.nan                                      # every query NaN: an empty group box
    sel = kind == 6; c["hi"][idx[sel], rng.integers(0, 3, sel.sum())] = np.inf  # an unbounded box
    sel = kind == 7; c["ub"][sel] = -1.0                                       # no term needed
    c["count"] = rng.choice([64, 64, 5, 31, 32, 33], n)
    v = boxcull.verdicts(c)
    _assert_cull_is_exact(c, v, "NaN / Inf draws")
    got = _lanes(v)
    # a NaN coordinate fails every metric that reads its axis (a view that drops the axis still passes on the other two, and the
    # group box holds those two: the property above covers it)
    assert not got[np.isnan(c["q"]).all(-1)].any(), "a query that is NaN on every axis has an empty list"
    c3 = c.copy()
    c3["mset"] = 1
    assert not _lanes(boxcull.verdicts(c3))[np.isnan(c["q"]).any(-1)].any(), "the 3-D metric fails a query with a NaN coordinate"
    for k in (4, 5, 7):
        assert (v["group"][kind == k] == 0).all() and (v["lanes"][kind == k] == 0).all(), k
    assert (v["group"][kind == 3] == 1)[(lane < c["count"])[kind == 3]].all(), "an infinite bound lets every box survive"
    # partly filled: what the lanes past the end hold -- wild coordinates, huge bounds -- changes nothing
    part = c[c["count"] < 64].copy()
    wild = part.copy()
    past = np.arange(64)[None, :] >= wild["count"][:, None]
    wild["q"][past] = rng.choice([0.0, 1e30, -1e30, np.nan, np.inf], (int(past.sum()), 3)).astype(np.float32)
    wild["ub"][past] = np.float32(1e30)
    a, b = boxcull.verdicts(part), boxcull.verdicts(wild)
    assert np.array_equal(a["group"], b["group"]) and np.array_equal(a["lanes"], b["lanes"])
    assert np.array_equal(a["glo"], b["glo"], equal_nan=True) and np.array_equal(a["gub"], b["gub"], equal_nan=True)
