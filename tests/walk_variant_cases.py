"""The clouds and launch patterns of tests/test_gpu_walk_variants.py, and -- for the standing-still cases -- the CPU prediction of the
term masks (`need`, four bits per direction) that the pruned solve's rule (houv::term_anchor_masks, houv_amd/csrc/houv_math.h)
produces on them.  tests/test_walk_variants_host.py checks on the CPU that the predicted masks reach every compiled walk variant
(houv::walk_variant); the GPU file checks that the walks saw each predicted mask.  Not a test module."""
import numpy as np
import torch

K = 26
LAUNCHES = (1, 7, 50, 3)
STILL = (1, 6)              # lr 1e-9: iterations 1..4 of the second launch apply the rule to the records of its iteration 0
REL, ABS, MOVE = 1e-3, 1e-6, 1e-6                # kTermRel, kTermAbs, kTermMoveErr, houv_math.h
BAND = 0.05                 # a gap within 5 % of the rule's margin is "unsure": CPU and GPU sums differ in rounding (~1e-6 relative)

# name: (points, lr, kind, pairs, launches, expected (block, points per lane, prune mode), parameter precisions)
CASES = {
    "320_plain": (320, 0.01, "plain", 2, LAUNCHES, (256, 2, 2), (False,)),
    "512_plain": (512, 0.01, "plain", 2, LAUNCHES, (256, 2, 2), (False, True)),
    "512_crop": (512, 0.01, "crop", 2, LAUNCHES, (256, 2, 2), (False,)),
    "320_axis_x": (320, 0.01, "axis0", 2, LAUNCHES, (256, 2, 2), (False,)),
    "512_axis_z": (512, 0.01, "axis2", 2, LAUNCHES, (256, 2, 2), (False,)),
    "512_one_nan_point": (512, 0.01, "nan", 2, LAUNCHES, (256, 2, 2), (False,)),
    "512_standing_still": (512, 1e-9, "plain", 2, STILL, (256, 2, 2), (False,)),
    "768_plain": (768, 0.01, "plain", 2, LAUNCHES, (256, 3, 2), (False,)),
    "2048_bench_kernel": (2048, 0.01, "plain", 1, LAUNCHES, (512, 4, 2), (False, True)),
    "2500_super_tiles": (2500, 0.01, "plain", 1, (1, 7), (1024, 3, 3), (False,)),
}
STILL_CASES = sorted(n for n, c in CASES.items() if c[4] == STILL)


def cpu_clouds(name):
    """src, tgt [pairs, N, 3] on the CPU, before the spatial sort (which permutes the points of a cloud: no term depends on it)."""
    from houv_amd import synthetic
    N, _, kind, pairs, _, _, _ = CASES[name]
    src, tgt, _ = synthetic.make_pairs(pairs, N, seed=91)
    if kind == "crop":
        # the target is one half-space of the source, padded by duplicates to N points: every target point has its twin in the
        # source, half of the source points have none -- the terms over the moved points lose every metric near the true pose
        rows = []
        for p in range(pairs):
            keep = src[p][src[p][:, 0] > src[p][:, 0].median()]
            rows.append(keep.repeat((N + keep.shape[0] - 1) // keep.shape[0], 1)[:N])
        tgt = torch.stack(rows)
    elif kind.startswith("axis"):
        # the source is the target with a quarter of its points displaced along one axis: the view that drops that axis does not
        # see them, the 3-D term trims them (k = N / 2), the other two views' terms over the moved points lose
        src = tgt.clone()
        src[:, : N // 4, int(kind[-1])] += 1.5
    return src.contiguous(), tgt.contiguous()


def gpu_clouds(name, dev):
    from houv_amd import solver
    N, _, kind, _, _, _, _ = CASES[name]
    src, tgt = cpu_clouds(name)
    leaf = solver.sort_leaf(N, N)
    src, tgt = solver.spatial_sort(src.to(dev), leaf), solver.spatial_sort(tgt.to(dev), leaf)
    if kind == "nan":
        src[0, 5, 0] = float("nan")
    return src, tgt


def standing_still_masks(name):
    """The masks of a standing-still case that the rule produces for SURE: a set of `need` values (0..15; 0 = the sweep is
    skipped).  With lr = 1e-9 the pose does not move, so the rule's slack is its margin alone (tests/test_gpu_term_anchors.py):
    term (metric, dir) is dropped where the other direction's cd is lower by more than the margin.  A (hypothesis, direction)
    counts only when each of its four metrics is outside the BAND around the margin."""
    from oracle import houv_ref_cpu as orc
    from scripts.sim_term_masks import eight_terms
    N, _, _, pairs, _, _, _ = CASES[name]
    src, tgt = cpu_clouds(name)
    s, t = orc._replicate(src, K), orc._replicate(tgt, K)
    V, ang, tc, ts = [torch.from_numpy(p) for p in orc.houv_init_params(pairs * K)]
    moved, _, T = orc.houv_forward(s, V, ang, tc, ts, 0, "houv")
    cd = eight_terms(moved, t).double().numpy()                       # [n, metric, dir]; dir 0 over the target points
    radius = np.sqrt((s.double().numpy() ** 2).sum(2).max(1))
    tn = np.sqrt((T.double().numpy()[:, 0] ** 2).sum(1))
    margin = REL * np.abs(cd).sum(2) + (ABS + MOVE * (2.0 * radius + 2.0 * tn))[:, None]
    sure = set()
    for d in (0, 1):
        gap = cd[:, :, d] - cd[:, :, 1 - d]                           # > margin: term (metric, d) loses and is dropped
        dropped, kept = gap > (1.0 + BAND) * margin, gap < (1.0 - BAND) * margin
        ok = (dropped | kept).all(1)
        need = (kept * (1 << np.arange(4))[None, :]).sum(1)
        sure |= {int(m) for m in need[ok]}
    return sure
