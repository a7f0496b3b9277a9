"""CPU replay of the seeded first iteration of a pruned solve stage (houv_solve_seed, houv_amd/csrc/solve_seed.hip):
how long the visit lists of a stage's FIRST iteration are when the workspace starts from first-guess neighbour records instead of
nothing (64 of 64 sub-tiles: the brute-force sweep), for several ways of guessing.

Synthetic pairs, both clouds in k-d leaf order (solver.kd_sort), the source moved by the poses solver.houv_init_params gives the
hypotheses --hyps of a K = 64 stage, in the angle windows --bases.  A query's bound per metric is its distance to the guessed
reference (x 1.00001, as prune_masks takes it); its list is every 32-point run whose box passes for some metric.  Both sweep
directions are replayed and averaged.  Rules:

  exact     the true nearest neighbour per metric (what the brute-force first iteration leaves behind: the steady state's lists)
  metric    THE KERNEL'S RULE (seed_records below): per metric, the run whose box is nearest in that metric's projection, then the
            point of that run nearest in that metric
  box3d     the run whose box is nearest in 3-D, its best point per metric
  two3d     the two runs nearest in 3-D, their best point per metric
  first     the first point of the run nearest in 3-D, for all metrics

seed_records is the NumPy statement of the kernel's rule that tests/test_solve_seed_host.py and tests/test_gpu_solve_seed.py compare
the kernel's records with.

  python scripts/sim_solve_seed.py [--pairs 0 1] [--points 2048] [--hyps 0 13 26 39 52] [--bases 0 2]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEAF = 32
DROP = [(), (0,), (1,), (2,)]                      # metric m leaves out these axes (0: 3-D, 1 / 2 / 3: x / y / z dropped)


def metric_sq(off):
    """[..., 3] offsets -> [..., 4] squared distances per metric, each summed from its own axes only (a NaN on a dropped axis does
    not reach the metric, as in the kernels)."""
    sq = off ** 2
    return np.stack([sum(sq[..., a] for a in range(3) if a not in drop) for drop in DROP], -1)


def run_boxes(pts, leaf=LEAF):
    """(lo, hi) [runs, 3] of the runs of ``leaf`` consecutive points; a last, partly filled run from its existing points; a NaN
    coordinate is left out, and a run without a number on an axis keeps lo = +inf, hi = -inf there."""
    n = len(pts)
    pad = -(-n // leaf) * leaf
    t = np.full((pad, 3), np.nan, pts.dtype)
    t[:n] = pts
    t = t.reshape(-1, leaf, 3)
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmin.reduce(t, 1), np.inf), np.fmax(np.fmax.reduce(t, 1), -np.inf)


def box_sq(q, lo, hi):
    """[nq, runs, 4] squared distance per metric from each query to each box: the query clamped into the box (a NaN query
    coordinate clamps to lo, as fmaxf / fminf do, and its distance is NaN)."""
    with np.errstate(invalid="ignore"):
        c = np.fmin(np.fmax(q[:, None, :], lo[None]), hi[None])
        return metric_sq(q[:, None, :] - c)


def _first_min(d, axis):
    """index of the first strict minimum from +inf along ``axis`` (NaN never wins; nothing below +inf: 0), and that minimum."""
    d = np.where(np.isnan(d), np.inf, d)
    i = d.argmin(axis)
    return i, np.take_along_axis(d, np.expand_dims(i, axis), axis).squeeze(axis)


def seed_records(q, refs, nmet=4, leaf=LEAF):
    """The kernel's rule.  q [nq, 3], refs [count, 3] -> int [nq, nmet]: for every query and metric the run whose box is nearest in
    that metric (lowest run among equals), then the point of that run nearest in that metric (lowest index among equals, strict <
    from +inf); no point of the run at a finite distance: the first reference of the cloud that is; none: 0."""
    count = len(refs)
    lo, hi = run_boxes(refs, leaf)
    bt, _ = _first_min(box_sq(q, lo, hi)[..., :nmet], 1)                         # [nq, nmet]
    pad = np.full((len(lo) * leaf, 3), np.nan, refs.dtype)
    pad[:count] = refs
    out = np.zeros((len(q), nmet), np.int64)
    for m in range(nmet):
        idx = bt[:, m, None] * leaf + np.arange(leaf)[None]                      # [nq, leaf]
        with np.errstate(invalid="ignore"):
            d = metric_sq(q[:, None, :] - pad[idx])[..., m]
        j, best = _first_min(d, 1)
        out[:, m] = bt[:, m] * leaf + j
        for i in np.nonzero(~(best < np.inf))[0]:                                # rare: scan the whole cloud
            with np.errstate(invalid="ignore"):
                fin = np.nonzero(metric_sq(q[i][None] - refs)[:, m] < np.inf)[0]
            out[i, m] = fin[0] if len(fin) else 0
    return out


def list_lengths(q, refs, rec, leaf=LEAF):
    """[nq] runs on each query's visit list when its bounds come from the records ``rec`` [nq, 4] (prune_masks' test)."""
    ub = np.stack([metric_sq(q - refs[rec[:, m]])[:, m] for m in range(4)], 1) * 1.00001 + 1e-30
    lo, hi = run_boxes(refs, leaf)
    return (box_sq(q, lo, hi) <= ub[:, None, :]).any(-1).sum(1)


def exact_records(q, refs):
    return metric_sq(q[:, None, :] - refs[None]).argmin(1)


def _best_in_runs(q, refs, runs, leaf=LEAF):
    """records [nq, 4]: per metric the best point among the runs ``runs`` [nq, r] of each query."""
    idx = (runs[:, :, None] * leaf + np.arange(leaf)[None, None]).reshape(len(q), -1)
    d = metric_sq(q[:, None, :] - refs[idx])                                     # [nq, r * leaf, 4]
    return np.take_along_axis(idx, d.argmin(1), 1)


def rule_records(rule, q, refs):
    if rule == "exact":
        return exact_records(q, refs)
    if rule == "metric":
        return seed_records(q, refs)
    d3 = box_sq(q, *run_boxes(refs))[..., 0]                                     # [nq, runs]
    if rule == "box3d":
        return _best_in_runs(q, refs, d3.argmin(1)[:, None])
    if rule == "two3d":
        return _best_in_runs(q, refs, np.argsort(d3, 1, kind="stable")[:, :2])
    if rule == "first":
        return np.repeat((d3.argmin(1) * LEAF)[:, None], 4, 1)
    raise ValueError(rule)


RULES = ["exact", "metric", "box3d", "two3d", "first"]


def pose(p, base, trans_mode=0):
    """R [3, 3], T [3] of the parameters p [8] in the angle window ``base`` (pose_forward, houv_math.h), in float64."""
    u = p[0:3] / np.linalg.norm(p[0:3])
    theta = np.sin(p[3] * np.pi) * np.pi / 8 + np.pi / 8 + base * np.pi / 4
    A = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    R = np.eye(3) + np.sin(theta) * A + (1 - np.cos(theta)) * A @ A
    sp = np.sin(p[7] * np.pi)
    sigma = sp * 0.125 + 0.125 if trans_mode == 0 else sp
    return R, p[4:7] / np.linalg.norm(p[4:7]) * sigma


def mean_lists(src, tgt, params, base, rules=RULES):
    """{rule: mean list length of the first iteration} over the hypotheses ``params`` [h, 8], both directions."""
    out = {r: [] for r in rules}
    for p in params:
        R, T = pose(p, base)
        mov = src @ R.T + T
        for r in rules:
            la = list_lengths(mov, tgt, rule_records(r, mov, tgt))               # direction A: moved -> target
            lb = list_lengths(tgt, mov, rule_records(r, tgt, mov))               # direction B: target -> moved
            out[r].append(0.5 * (la.mean() + lb.mean()))
    return {r: float(np.mean(v)) for r, v in out.items()}


def sorted_pair(pid, points):
    from houv_amd import solver, synthetic
    src, tgt, _ = synthetic.make_pairs(1, points, first_id=pid)
    return solver.kd_sort(src, LEAF)[0].double().numpy(), solver.kd_sort(tgt, LEAF)[0].double().numpy()


def main():
    from houv_amd import solver
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--hyps", type=int, nargs="+", default=[0, 13, 26, 39, 52], help="hypotheses of a K = 64 stage")
    ap.add_argument("--bases", type=int, nargs="+", default=[0, 2])
    a = ap.parse_args()
    params = solver.houv_init_params(64)[a.hyps]
    print(f"{a.points} points, {-(-a.points // LEAF)} runs of {LEAF}; pairs {a.pairs}, hypotheses {a.hyps}: mean visit-list length "
          "of a stage's first iteration")
    print("rule     " + "".join(f"  base {b}" for b in a.bases))
    res = {b: [mean_lists(*sorted_pair(pid, a.points), params, b) for pid in a.pairs] for b in a.bases}
    for r in RULES:
        print(f"{r:8s} " + "".join(f"  {np.mean([x[r] for x in res[b]]):6.2f}" for b in a.bases))


if __name__ == "__main__":
    main()
