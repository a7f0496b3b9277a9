"""CPU: the rule of houv_solve_seed as scripts/sim_solve_seed.py states it in NumPy (`seed_records`, what
tests/test_gpu_solve_seed.py holds the kernel's records against), checked against a brute-force float64 search, and the replay's
headline: seeded first-iteration visit lists stay within twice the exact-neighbour lists."""
import numpy as np
import pytest

from scripts.sim_solve_seed import (LEAF, box_sq, exact_records, list_lengths, mean_lists, metric_sq, run_boxes, seed_records,
                                    sorted_pair)
from solve_seed_cases import GRID_SHAPES, grid_pair, nan_grid_pair


def _check_against_brute_force(q, refs, nmet):
    """Every record is in range; it is a reference at a finite distance whenever the cloud has one for that query and metric,
    0 otherwise; and it is what a plain loop over boxes and points gives (lowest run, lowest index, strict < from +inf)."""
    rec = seed_records(q, refs, nmet)
    assert rec.shape == (len(q), nmet) and rec.min() >= 0 and rec.max() < len(refs)
    with np.errstate(invalid="ignore"):
        d = metric_sq(q[:, None, :] - refs[None])[..., :nmet]                     # [nq, count, nmet]
    finite = d < np.inf                                                           # False for NaN
    got = np.take_along_axis(d, rec[:, None, :], 1)[:, 0, :]
    has = finite.any(1)
    assert np.all((got < np.inf) == has), "a seed at infinite or NaN distance although a finite reference exists"
    assert np.all(rec[~has] == 0)
    lo, hi = run_boxes(refs)
    bs = box_sq(q, lo, hi)
    for i in range(0, len(q), max(1, len(q) // 40)):                              # a plain restatement on a sample of the queries
        for m in range(nmet):
            bd, bt = np.inf, 0
            for t in range(len(lo)):
                if bs[i, t, m] < bd:
                    bd, bt = bs[i, t, m], t
            best, bi = np.inf, None
            for j in range(bt * LEAF, min((bt + 1) * LEAF, len(refs))):
                if d[i, j, m] < best:
                    best, bi = d[i, j, m], j
            if bi is None:
                fin = np.nonzero(finite[i, :, m])[0]
                bi = fin[0] if len(fin) else 0
            assert rec[i, m] == bi, (i, m)
    return rec


@pytest.mark.parametrize("n,count", [(300, 300), (257, 500), (700, 333)])
def test_seed_rule_on_random_clouds_never_seeds_a_non_finite_reference(n, count):
    rng = np.random.default_rng(n + count)
    q, refs = rng.standard_normal((n, 3)), rng.standard_normal((count, 3))
    refs = refs[np.argsort(refs[:, 0], kind="stable")]                            # runs = slabs along x: boxes that mean something
    _check_against_brute_force(q, refs, 4)
    # NaN and Inf points among the queries and the references, a run of NaN points, a run with no finite full-metric distance
    q[3] = np.nan
    q[7, 1] = np.inf
    refs[10] = np.nan
    refs[45, 2] = np.inf
    refs[64:96] = np.nan
    refs[128:160:2, 0] = np.nan
    refs[129:160:2, 1] = np.nan
    rec = _check_against_brute_force(q, refs, 4)
    assert np.all(rec[3] == 0) and np.all(rec[7, [0, 1, 3]] == 0)                # the view that drops y does not see q[7]'s Inf
    assert not (rec == 10).any() and not (rec[:, :3] == 45).any() and not ((rec >= 64) & (rec < 96)).any()
    _check_against_brute_force(q, refs, 1)


@pytest.mark.parametrize("N,M,views", GRID_SHAPES)
def test_seed_rule_on_the_grid_clouds_meets_the_ties_they_are_built_for(N, M, views):
    """The grid pairs do contain what the GPU test relies on them for: equidistant boxes, a run of equal points, a partly filled
    last run -- and the statement resolves them to the lowest run and index."""
    nmet = 4 if views else 1
    for make in (grid_pair, nan_grid_pair):
        src, tgt = (c.astype(np.float64) for c in make(N, M))
        for q, refs, equal_run in ((tgt, src, 3), (src, tgt, 5)):
            rec = _check_against_brute_force(q, refs, nmet)
            assert len(refs) % LEAF != 0
            bs = box_sq(q, *run_boxes(refs))[..., 0]
            with np.errstate(invalid="ignore"):
                two_nearest = np.sort(np.where(np.isnan(bs), np.inf, bs), 1)[:, :2]
            ties = (two_nearest[:, 0] == two_nearest[:, 1]) & (two_nearest[:, 0] < np.inf)
            assert ties.sum() >= len(q) // 8, "queries with two equidistant nearest boxes"
            if make is grid_pair:
                hit = (rec[:, 0] >= equal_run * LEAF) & (rec[:, 0] < (equal_run + 1) * LEAF)
                assert hit.any() and np.all(rec[hit, 0] == equal_run * LEAF), "a run of equal points seeds its first point"
                if refs is src:   # the last target points lie beyond the last source run; the other way round box 8 wins the tie
                    assert (rec[:, 0] >= len(refs) // LEAF * LEAF).any(), "the partly filled last run seeds its neighbours"


def test_seeded_first_iteration_lists_stay_within_twice_the_exact_neighbour_lists():
    """scripts/sim_solve_seed.py's headline at 512 points, pairs 0 and 1, two hypotheses, angle windows 0 and 2: 6.0 sub-tiles per
    query against 5.3 with exact neighbours (1.14 x; 1.48 x at 2048 points: 8.5 against 5.7 of 64)."""
    from houv_amd import solver
    params = solver.houv_init_params(64)[[0, 26]]
    for pid in (0, 1):
        src, tgt = sorted_pair(pid, 512)
        for base in (0, 2):
            r = mean_lists(src, tgt, params, base, rules=("exact", "metric"))
            assert r["exact"] <= r["metric"] < 2.0 * r["exact"], (pid, base, r)
            assert r["metric"] < 0.5 * (512 // LEAF), "well below the brute-force sweep's every sub-tile"


def test_exact_records_give_the_shortest_lists():
    src, tgt = sorted_pair(0, 512)
    la = list_lengths(src, tgt, exact_records(src, tgt)).mean()
    lb = list_lengths(src, tgt, seed_records(src, tgt)).mean()
    assert 1.0 <= la <= lb
