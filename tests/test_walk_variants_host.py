"""CPU: the table of walk variants of the pruned solve (houv::walk_variant, houv_amd/csrc/houv_math.h), host-compiled
(tests/walkvariants): every term mask of a direction runs on a compiled metric set that contains it, and the standing-still
cases of tests/test_gpu_walk_variants.py produce -- by the term rule restated on the CPU -- masks that together reach EVERY
compiled set, so that no variant ships without a GPU case that runs it."""
from tests import walk_variant_cases as wc
from tests import walkvariants


def _popcount(x):
    return bin(x).count("1")


def test_every_mask_runs_on_a_compiled_superset():
    variant, instantiated, cost, packed = walkvariants.table()
    sets = [m for m in range(16) if instantiated[m]]
    print("compiled metric sets:", sets, "table:", variant)
    assert 15 in sets and variant[15] == 15
    assert 0 not in sets, "a sweep none of whose terms is needed is skipped, not walked"
    for need in range(16):
        v = variant[need]
        assert v & need == need, f"mask {need} runs on {v}, which lacks a metric it needs"
        assert instantiated[v], f"mask {need} runs on {v}, which is not compiled"
        assert (packed >> (4 * need)) & 15 == v, "the packed table the kernel shifts is the same table"
    for s in sets:
        assert variant[s] == s, f"compiled set {s} runs on {variant[s]}"


def test_a_mask_runs_on_the_cheapest_compiled_superset():
    variant, instantiated, cost, _ = walkvariants.table()
    sets = [m for m in range(16) if instantiated[m]]
    # the cost model: per pair of references 2 fma per metric (metric 0 also pays metric 3's), 2 mul for metric 1, 1 min3 per
    # metric, 16 pairs a step; 5 instructions of unit bookkeeping per metric and step
    assert cost[15] == 16 * 14 + 20 and cost[15] - cost[14] == 53 and cost[15] - cost[13] == 85
    assert cost[15] - cost[11] == 53 and cost[15] - cost[7] == 21 and cost[15] - cost[6] == 53 + 21 + 32
    for a in range(16):
        for b in range(16):
            if a & b == a:
                assert cost[a] <= cost[b], f"a subset costs no more: {a} within {b}"
    for need in range(1, 16):
        assert cost[variant[need]] == min(cost[s] for s in sets if s & need == need), need


def test_the_standing_still_cases_reach_every_compiled_variant():
    variant, instantiated, _, _ = walkvariants.table()
    sets = {m for m in range(16) if instantiated[m]}
    reached = {}
    for name in wc.STILL_CASES:
        masks = wc.standing_still_masks(name) - {0}
        print(f"{name}: masks produced for sure {sorted(masks)}")
        for m in masks:
            reached.setdefault(variant[m], set()).add(m)
    print("compiled set <- masks that run on it:", {s: sorted(v) for s, v in sorted(reached.items())})
    assert set(reached) == sets, f"no constructed case reaches the compiled sets {sorted(sets - set(reached))}"
