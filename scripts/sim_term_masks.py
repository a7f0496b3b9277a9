"""CPU simulation of the pruned solve's term masks (houv::term_masks, houv_amd/csrc/houv_math.h).

Runs the oracle's predict_model formulation (fp32, autograd + Adam) on synthetic pairs, logs the eight Chamfer terms and the
pose of every hypothesis at every iteration, then replays the rule: anchors are the iterations that compute every term (every
REFRESH-th, the first and the last), in between a term is dropped when the anchor proves that it loses.  Prints the share of
(direction, metric) terms proved unnecessary, how many per direction sweep by kind, and the number of UNSOUND decisions (a dropped
term that would have won or tied), which must be 0.

  python scripts/sim_term_masks.py [--pairs 2 3 4 5] [--points 1024] [--kernel 26] [--iters 200] [--refresh 4]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[2, 3, 4, 5])
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--kernel", type=int, default=26)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--refresh", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2021)
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
    terms = dropped = unsound = 0
    per_sweep = np.zeros(2)                        # dropped 3-D terms, dropped view terms
    anchor = None
    for it, (cd, R, T) in enumerate(log):
        if it % a.refresh == 0 or it == a.iters - 1:
            anchor = (cd, R, T)
            need = np.ones(cd.shape, bool)
        else:
            need = rule(anchor[0], anchor[1], anchor[2], R, T, radius)
        terms += need.size
        dropped += int((~need).sum())
        per_sweep += [(~need[:, 0]).sum(), (~need[:, 1:]).sum()]
        loses = np.stack([cd[:, :, 0] > cd[:, :, 1], cd[:, :, 1] > cd[:, :, 0]], 2)       # dir d strictly loses now
        unsound += int((~need & ~loses).sum())
    sweeps = 2.0 * len(log) * B * K
    print(f"{a.points} points, pairs {a.pairs}, {K} restarts x {a.iters} iterations, anchor every {a.refresh}th iteration")
    print(f"terms proved unnecessary: {dropped} of {terms} = {100.0 * dropped / terms:.1f} %")
    print(f"dropped per direction sweep: 3-D {per_sweep[0] / sweeps:.2f}, views {per_sweep[1] / sweeps:.2f}")
    print(f"unsound decisions over {len(log) * B * K} hypothesis-iterations: {unsound}")
    return 1 if unsound else 0


if __name__ == "__main__":
    sys.exit(main())
