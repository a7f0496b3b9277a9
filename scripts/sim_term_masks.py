"""CPU simulation of the pruned solve's term masks (houv::term_anchor_masks and houv::term_masks, houv_amd/csrc/houv_math.h;
DESIGN.md 3.1b).

Runs the oracle's predict_model formulation (fp32, autograd + Adam) on synthetic pairs, logs the eight Chamfer terms and the
pose of every hypothesis at every iteration, then replays a dropping policy on the log.  Every policy computes all eight terms
on the first and the last iteration of a launch (--launch iterations each).  --policy:
  shared            term_masks: one anchor, renewed by the iterations that compute every term, which every REFRESH-th is made to
  perterm           term_anchor_masks: every term has its own record (value and pose when last computed); still all terms on
                    every REFRESH-th iteration
  perterm-noforce   the same without the forced all-term iterations (what solve.hip runs)
--no-sqrt2 takes the Frobenius norm for the rotation part of the per-term rule (term_masks' bound) instead of Frobenius /
sqrt(2) + defects; --max-age A forces a term back after A dropped iterations in a row (0: never, which is solve.hip's kTermMaxAge; the
ladder of --policy all ends with A = 12).
Prints the share of (direction, metric) terms proved unnecessary, by quarter of the run as well, how many per direction sweep by
kind, and the number of UNSOUND decisions (a dropped term that would have won or tied), which must be 0.

  python scripts/sim_term_masks.py [--pairs 0 1 2 3] [--points 512] [--kernel 26] [--iters 200] [--launch 50]
                                   [--policy all] [--refresh 4] [--max-age 12]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from houv_amd import synthetic                     # noqa: E402
from oracle import houv_ref_cpu as orc             # noqa: E402

REL, ABS, MOVE = np.float32(1e-3), np.float32(1e-6), np.float32(1e-6)      # kTermRel, kTermAbs, kTermMoveErr


def eight_terms(moved, target):
    """cd[n, metric, dir] as Predict_loss takes them: dir 0 over the target points, 1 over the moved points."""
    rows = [orc.calc_cd_percent(moved, target, percent=0.5)] + [orc.loss_view(moved, target, dim=d) for d in range(3)]
    return torch.stack([torch.stack([over_gt, over_out], 1) for over_gt, over_out in rows], 1)


def rule(cd_a, R_a, T_a, R, T, radius):
    """term_masks in fp32 numpy: need[n, metric, dir]."""
    f = np.float32
    delta2 = f(2) * (np.sqrt(((R - R_a) ** 2).sum((1, 2), dtype=f)) * radius + np.sqrt(((T - T_a) ** 2).sum(1, dtype=f)))
    abs_m = ABS + MOVE * (f(2) * radius + np.sqrt((T ** 2).sum(1, dtype=f)) + np.sqrt((T_a ** 2).sum(1, dtype=f)))
    c0, c1 = cd_a[:, :, 0], cd_a[:, :, 1]
    slack = (delta2 + abs_m)[:, None] + REL * (np.abs(c0) + np.abs(c1) + delta2[:, None])
    need = np.ones(cd_a.shape, bool)
    need[:, :, 1] = ~(c0 + slack < c1)
    need[:, :, 0] = ~(c1 + slack < c0)
    return need


def defect(M):
    """term_rot_defect in fp32 numpy: ||M^T M - I||_F + kTermDefectErr."""
    f = np.float32
    G = (np.swapaxes(M, -1, -2) @ M).astype(f) - np.eye(3, dtype=f)
    return np.sqrt((G ** 2).sum((-1, -2), dtype=f)) + f(1e-6)


def travel(Rz, Tz, R, T, radius, sqrt2):
    """term_travel in fp32 numpy over records [n, 4, 2, ...]: (d, |T_Z|)."""
    f = np.float32
    fr = ((R[:, None, None] - Rz) ** 2).sum((-1, -2), dtype=f)
    fro = np.sqrt(fr)
    rho = fro
    if sqrt2:
        dft = defect(R)[:, None, None] + defect(Rz)
        tight = fro * f(0.70710683) + f(2) * dft
        rho = np.where((fr <= 2) & (dft <= f(1e-3)) & (tight < fro), tight, fro)
    d = rho * radius[:, None, None] + np.sqrt(((T[:, None, None] - Tz) ** 2).sum(-1, dtype=f))
    return d, np.sqrt((Tz ** 2).sum(-1, dtype=f))


def rule_perterm(cd_r, R_r, T_r, R, T, radius, sqrt2):
    """term_anchor_masks in fp32 numpy with one record per term: cd_r [n,4,2], R_r [n,4,2,3,3], T_r [n,4,2,3] -> need[n,4,2]."""
    f = np.float32
    d, tz = travel(R_r, T_r, R, T, radius, sqrt2)
    dd = d[:, :, 0] + d[:, :, 1]
    tn = np.sqrt((T ** 2).sum(1, dtype=f))
    c0, c1 = cd_r[:, :, 0], cd_r[:, :, 1]
    slack = dd + REL * (np.abs(c0) + np.abs(c1) + dd) + ABS + MOVE * ((f(2) * radius + tn)[:, None] + f(0.5) * (tz[:, :, 0] + tz[:, :, 1]))
    need = np.ones(cd_r.shape, bool)
    need[:, :, 1] = ~(c0 + slack < c1)
    need[:, :, 0] = ~(c1 + slack < c0)
    return need


def replay(log, radius, policy, refresh, launch, max_age, sqrt2):
    """(terms, dropped, unsound, dropped per sweep kind [3-D, views], dropped share by quarter of the run)."""
    iters = len(log)
    terms = dropped = unsound = 0
    per_sweep = np.zeros(2)
    by_quarter = np.zeros((4, 2))
    anchor = rec = age = None
    for it, (cd, R, T) in enumerate(log):
        edge = it % launch == 0 or it % launch == launch - 1 or it == iters - 1
        forced = edge or (policy != "perterm-noforce" and it % refresh == 0)
        if forced:
            need = np.ones(cd.shape, bool)
        elif policy == "shared":
            need = rule(anchor[0], anchor[1], anchor[2], R, T, radius)
        else:
            need = rule_perterm(rec[0], rec[1], rec[2], R, T, radius, sqrt2)
            if max_age > 0:
                back = age >= max_age                            # dropped max_age times in a row: computed now
                need[back] = True
        if policy == "shared":
            if need.all():
                anchor = (cd, R, T)
        else:
            if rec is None:
                n = cd.shape[0]
                rec = [cd.copy(), np.broadcast_to(R[:, None, None], (n, 4, 2, 3, 3)).copy(),
                       np.broadcast_to(T[:, None, None], (n, 4, 2, 3)).copy()]
                age = np.zeros((n, 4), int)
            rec[0][need] = cd[need]
            rec[1][need] = np.broadcast_to(R[:, None, None], rec[1].shape)[need]
            rec[2][need] = np.broadcast_to(T[:, None, None], rec[2].shape)[need]
            age = np.where(need.all(2), 0, age + 1)
        terms += need.size
        dropped += int((~need).sum())
        by_quarter[min(3, 4 * it // iters)] += [(~need).sum(), need.size]
        per_sweep += [(~need[:, 0]).sum(), (~need[:, 1:]).sum()]
        loses = np.stack([cd[:, :, 0] > cd[:, :, 1], cd[:, :, 1] > cd[:, :, 0]], 2)       # dir d strictly loses now
        unsound += int((~need & ~loses).sum())
    return terms, dropped, unsound, per_sweep, by_quarter[:, 0] / by_quarter[:, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--points", type=int, default=512)
    ap.add_argument("--kernel", type=int, default=26)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--refresh", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2021)
    ap.add_argument("--launch", type=int, default=50, help="iterations per launch: its first and last compute every term")
    ap.add_argument("--policy", default="all", choices=["all", "shared", "perterm", "perterm-noforce"])
    ap.add_argument("--max-age", type=int, default=12, help="perterm-noforce: 0 = a dropped term is never forced back (solve.hip); --policy all: the ladder's last row")
    ap.add_argument("--no-sqrt2", action="store_true")
    a = ap.parse_args()
    src, tgt, _ = synthetic.make_pairs(max(a.pairs) + 1, a.points, seed=a.seed)
    src, tgt = src[a.pairs].contiguous(), tgt[a.pairs].contiguous()
    B, K = src.shape[0], a.kernel
    s, t = orc._replicate(src, K), orc._replicate(tgt, K)
    radius = np.sqrt((s.numpy() ** 2).sum(2).max(1)).astype(np.float32)
    V, ang, tc, ts = [torch.nn.Parameter(torch.from_numpy(p)) for p in orc.houv_init_params(B * K, a.seed)]
    opt = torch.optim.Adam([V, ang, tc, ts], lr=0.01)
    log = []
    for it in range(a.iters):
        opt.zero_grad()
        moved, R, T = orc.houv_forward(s, V, ang, tc, ts, 0, "houv")
        cd = eight_terms(moved, t)
        loss = (6 * cd[:, 0].min(1)[0] + cd[:, 1:].min(2)[0].sum(1))
        loss.mean().backward()
        opt.step()
        log.append((cd.detach().numpy().copy(), R.detach().numpy().copy(), T.detach().numpy()[:, 0].copy()))
        if (it + 1) % 50 == 0:
            print(f"iteration {it + 1}: mean loss {float(loss.detach().mean()):.5f}", flush=True)
    print(f"{a.points} points, pairs {a.pairs}, {K} restarts x {a.iters} iterations in launches of {a.launch}")
    if a.policy == "all":      # the ladder of DESIGN.md 3.1b
        runs = [("shared", a.refresh, 0, False), ("perterm", a.refresh, 0, False), ("perterm-noforce", a.refresh, 0, False),
                ("perterm-noforce", a.refresh, 0, True), ("perterm-noforce", a.refresh, a.max_age, True)]
    else:
        runs = [(a.policy, a.refresh, a.max_age if a.policy == "perterm-noforce" else 0, not a.no_sqrt2)]
    unsound = 0
    sweeps = 2.0 * len(log) * B * K
    for policy, refresh, max_age, sqrt2 in runs:
        terms, dropped, bad, per_sweep, quarters = replay(log, radius, policy, refresh, a.launch, max_age, sqrt2)
        what = policy + ("" if policy == "perterm-noforce" else f", all terms every {refresh}th iteration")
        if policy != "shared":
            what += (", rotation part / sqrt(2)" if sqrt2 else ", Frobenius rotation part") + (f", max age {max_age}" if max_age else "")
        print(f"{what}: {dropped} of {terms} terms proved unnecessary = {100.0 * dropped / terms:.1f} %; by quarter "
              + " / ".join(f"{100.0 * q:.0f}" for q in quarters)
              + f" %; per direction sweep 3-D {per_sweep[0] / sweeps:.2f}, views {per_sweep[1] / sweeps:.2f}; unsound {bad}")
        unsound += bad
    print(f"unsound decisions over {len(log) * B * K} hypothesis-iterations, all policies: {unsound}")
    return 1 if unsound else 0


if __name__ == "__main__":
    sys.exit(main())
