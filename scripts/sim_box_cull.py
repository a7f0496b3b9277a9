"""CPU simulation of the group cull of the pruned solve's box tests (prune_masks, houv_amd/csrc/houv_sweep.h):
how many of a cloud's reference boxes survive a conservative test of a GROUP of consecutive queries -- the group's box against
the reference box, with the group's largest bound per metric -- and how that compares with the union of the queries' own lists.

Synthetic pairs, both clouds in k-d leaf order (solver.kd_sort), the source moved by a pose --angles degrees from the true one.
The bound of a query and metric is its distance to the point that was its nearest neighbour one step earlier (a pose 5 % farther
from the truth), as the kernel's remembered neighbours give it.  Both sweep directions are simulated and averaged.  Prints per
angle: the mean list length per query, and per group size the boxes surviving the group test and the true union of the lists;
for the kernel's present ownership (a wave owns --points-per-lane strided groups of 64) also the union over the wave's groups,
which is what a cull per wave rather than per k would have to test.

  python scripts/sim_box_cull.py [--pairs 0 1] [--points 2048] [--block 512] [--angles 0.2 0.5 1 2 5]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from houv_amd import solver, synthetic             # noqa: E402

LEAF = 32
DROP = [(), (0,), (1,), (2,)]                      # metric m leaves out these axes (0: 3-D, 1 / 2 / 3: x / y / z dropped)


def metric_sq(off):
    """[..., 3] offsets -> [..., 4] squared distances per metric."""
    sq = off ** 2
    return np.stack([sq.sum(-1) - sum(sq[..., a] for a in drop) for drop in DROP], -1)


def rotation(axis, deg):
    a = np.radians(deg)
    x, y, z = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def nearest(q, r):
    """index [nq, 4] of each query's nearest reference per metric."""
    return metric_sq(q[:, None, :] - r[None, :, :]).argmin(1)


def boxes_of(pts, size):
    t = pts.reshape(-1, size, 3)
    return t.min(1), t.max(1)


def sweep(q_now, q_prev, refs_now, refs_prev, block, ppl):
    """One direction: queries against the boxes of the references' leaves.  -> dict of means."""
    n = len(q_now)
    prev_nn = nearest(q_prev, refs_prev)                                            # [n, 4] remembered neighbours
    ub = np.stack([metric_sq(q_now - refs_now[prev_nn[:, m]])[:, m] for m in range(4)], 1) * 1.00001 + 1e-30
    lo, hi = boxes_of(refs_now, LEAF)                                               # [nt, 3]
    off = np.maximum(np.maximum(lo[None] - q_now[:, None], q_now[:, None] - hi[None]), 0.0)
    lists = (metric_sq(off) <= ub[:, None, :]).any(-1)                              # [n, nt] the queries' own lists
    out = {"list": lists.sum(1).mean(), "boxes": len(lo)}
    for g in (64, 128, 256):
        glo, ghi = boxes_of(q_now, g)
        gub = ub.reshape(-1, g, 4).max(1)
        gap = np.maximum(np.maximum(lo[None] - ghi[:, None], glo[:, None] - hi[None]), 0.0)
        surv = (metric_sq(gap) <= gub[:, None, :]).any(-1)                          # [n / g, nt]
        union = lists.reshape(-1, g, len(lo)).any(1)
        assert not (union & ~surv).any(), "a culled box is on a query's list: the group test is not conservative"
        out[f"surv{g}"], out[f"union{g}"] = surv.sum(1).mean(), union.sum(1).mean()
        if g == 64 and n % (block * ppl) == 0:
            # present ownership: wave w of a workgroup owns the groups k * block / 64 + w, k = 0 .. ppl - 1
            waves = surv.reshape(ppl, block // 64, len(lo)).any(0)
            out["wave_union"] = waves.sum(1).mean()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--block", type=int, default=512, help="threads per workgroup of the kernel that serves --points")
    ap.add_argument("--angles", type=float, nargs="+", default=[0.2, 0.5, 1.0, 2.0, 5.0])
    a = ap.parse_args()
    ppl = a.points // a.block
    rng = np.random.default_rng(13)
    print(f"{a.points} points, {a.points // LEAF} boxes, workgroup of {a.block} threads x {ppl} points per lane")
    print("pair angle   list   | 64: surviving  union | 128: surviving  union | 256: surviving  union | wave's strided groups")
    for pid in a.pairs:
        src, tgt, tf = synthetic.make_pairs(1, a.points, first_id=pid)
        src = solver.kd_sort(src, LEAF)[0].double().numpy()
        tgt = solver.kd_sort(tgt, LEAF)[0].double().numpy()
        R, t = tf[0, :3, :3].double().numpy(), tf[0, :3, 3].double().numpy()
        centre = src.mean(0)
        for deg in a.angles:
            axis = rng.standard_normal(3)

            def moved(d):
                Rp = rotation(axis, d)
                return ((src - centre) @ Rp.T + centre) @ R.T + t

            now, prev = moved(deg), moved(deg * 1.05)
            ra = sweep(now, prev, tgt, tgt, a.block, ppl)                            # direction A: moved -> target
            rb = sweep(tgt, tgt, now, prev, a.block, ppl)                            # direction B: target -> moved
            m = {k: 0.5 * (ra[k] + rb[k]) for k in ra}
            print(f"{pid:4d} {deg:5.1f}  {m['list']:6.2f}  |     {m['surv64']:6.2f}  {m['union64']:6.2f}  |      {m['surv128']:6.2f}  "
                  f"{m['union128']:6.2f}  |      {m['surv256']:6.2f}  {m['union256']:6.2f}  | {m.get('wave_union', float('nan')):6.2f}")


if __name__ == "__main__":
    main()
