"""Time per call of the mm3d_pn2 point ops added with houv_ball_query / houv_scatter_points_grad, each next to what the same
device does with the torch composition a user had before them: cdist + mask + sort for the ball query, index_add_ for the three
backward passes (float atomics: not deterministic), and the helper losses written with those.  HIP events after a warm-up
call; the median of the repeats.

    python scripts/perf_pointops.py [--reps 5] [--out profiles/r06_perf_pointops.txt]"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from houv_amd import _lib, model_utils_completion as muc  # noqa: E402
from houv_amd.mm3d_pn2 import (ball_query, furthest_point_sample, gather_points, grouping_operation,  # noqa: E402
                               three_interpolate)


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_ball_query(r, nsample, xyz, ctr):
    """cdist + mask + sort: the first nsample indices inside the ball in index order, padded with the first."""
    N = xyz.shape[1]
    d2 = torch.cdist(ctr, xyz) ** 2
    key = torch.where(d2 < r * r, torch.arange(N, device=xyz.device).expand_as(d2), torch.full_like(d2, N, dtype=torch.long))
    key = key.sort(dim=-1).values[:, :, :nsample]
    first = torch.where(key[:, :, :1] == N, torch.zeros_like(key[:, :, :1]), key[:, :, :1])
    return torch.where(key == N, first.expand_as(key), key).int()


def torch_scatter(grad_out, idx, weight, N, S):
    B, C, _ = grad_out.shape
    terms = grad_out if S == 1 else grad_out.repeat_interleave(S, dim=2)
    if weight is not None:
        terms = terms * weight.unsqueeze(1)
    out = torch.zeros(B, C, N, device=grad_out.device)
    return out.scatter_add_(2, idx.long().unsqueeze(1).expand(-1, C, -1), terms)


def torch_repulsion(pred, nsample=20, radius=0.07):
    d2 = torch.cdist(pred, pred) ** 2
    d2 = -torch.topk(-d2, 5).values[:, :, 1:]
    d2 = d2.clamp_min(1e-12)
    return torch.mean(radius - torch.sqrt(d2) * torch.exp(-d2 / 0.03 ** 2))


def torch_uniform(pcd, percentages=(0.004, 0.006, 0.008, 0.010, 0.012), radius=1.0):
    """The reference's loss with every custom op replaced by its torch composition, except FPS (no torch form; common to both)."""
    B, N, _ = pcd.shape
    npoint = int(N * 0.05)
    loss = 0
    for p in percentages:
        nsample = int(N * p)
        expect = math.sqrt(math.pi * radius ** 2 * p / nsample)
        fps = furthest_point_sample(pcd, npoint).long()
        new_xyz = torch.gather(pcd, 1, fps.unsqueeze(2).expand(-1, -1, 3))
        idx = torch_ball_query(math.sqrt(p * radius), nsample, pcd.detach(), new_xyz.detach()).long()
        g = torch.gather(pcd, 1, idx.view(B, -1, 1).expand(-1, -1, 3)).view(-1, nsample, 3)
        d2 = (torch.cdist(g, g) ** 2)
        var = torch.topk(-d2, 2, dim=-1).values
        d = torch.sqrt(torch.abs(-var[:, :, 1:] + 1e-8)).mean(-1)
        loss = loss + torch.mean((d - expect) ** 2 / (expect + 1e-8)) * (p * 100) ** 2
    return loss / len(percentages)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_pointops.py needs an MI355X")
    dev = torch.device("cuda:0")
    lines = [f"# scripts/perf_pointops.py  library build {_lib.build_id()}  {torch.cuda.get_device_name(0)}  reps={args.reps}",
             "# case | houv ms (median [min, max]) | torch composition ms (median [min, max]) | torch / houv"]

    def row(label, ours, theirs):
        a, b = _time(ours, args.reps), _time(theirs, args.reps)
        lines.append(f"{label} | {a[0]:.3f} [{a[1]:.3f}, {a[2]:.3f}] | {b[0]:.3f} [{b[1]:.3f}, {b[2]:.3f}] | {b[0] / a[0]:.2f}")
        print(lines[-1], flush=True)

    g = torch.Generator().manual_seed(6)
    B, N = 32, 2048
    pcd = torch.rand((B, N, 3), generator=g).to(dev)
    flipped = pcd.transpose(1, 2).contiguous()
    new_xyz = gather_points(flipped, furthest_point_sample(pcd, int(N * 0.05))).transpose(1, 2).contiguous()
    for p in (0.004, 0.006, 0.008, 0.010, 0.012):
        r, ns = math.sqrt(p), int(N * p)
        same = torch.equal(ball_query(0, r, ns, pcd, new_xyz), torch_ball_query(r, ns, pcd, new_xyz))
        row(f"ball_query B {B} N {N} centres {new_xyz.shape[1]} r {r:.4f} nsample {ns} (same idx as torch: {same})",
            lambda: ball_query(0, r, ns, pcd, new_xyz), lambda: torch_ball_query(r, ns, pcd, new_xyz))
    row(f"ball_query B {B} N {N} centres {N} r 0.1 nsample 32", lambda: ball_query(0, 0.1, 32, pcd, pcd),
        lambda: torch_ball_query(0.1, 32, pcd, pcd))

    C, ns = 64, 20
    feats = torch.randn((B, C, N), generator=g).to(dev)
    idx = muc.knn(flipped, ns).int()                                        # B x N x 20 neighbour lists
    flat = idx.view(B, N * ns)
    go = torch.randn((B, C, N * ns), generator=g).to(dev)
    from houv_amd.mm3d_pn2 import _scatter_grad
    row(f"gather_points backward B {B} C {C} N {N} M {N * ns}", lambda: _scatter_grad(go, flat, None, N, 1),
        lambda: torch_scatter(go, flat, None, N, 1))
    go4 = go.view(B, C, N, ns)
    row(f"grouping_operation backward B {B} C {C} N {N} npoint {N} nsample {ns}",
        lambda: _scatter_grad(go4.view(B, C, -1), flat, None, N, 1), lambda: torch_scatter(go4.view(B, C, -1), flat, None, N, 1))
    m = 512
    src = pcd[:, :m].contiguous()
    i3, w3 = muc.three_nn_upsampling(pcd, src)
    go3 = torch.randn((B, C, N), generator=g).to(dev)
    row(f"three_interpolate backward B {B} C {C} n {N} from m {m}",
        lambda: _scatter_grad(go3, i3.view(B, N * 3), w3.view(B, N * 3), m, 3),
        lambda: torch_scatter(go3, i3.view(B, N * 3), w3.view(B, N * 3), m, 3))
    fm = torch.randn((B, C, m), generator=g).to(dev)
    row(f"three_interpolate forward B {B} C {C} n {N} from m {m}", lambda: three_interpolate(fm, i3, w3),
        lambda: (torch.gather(fm, 2, i3.view(B, 1, -1).long().expand(-1, C, -1)).view(B, C, N, 3) * w3.unsqueeze(1)).sum(-1))
    one = torch.zeros((B, N * ns), dtype=torch.int32, device=dev)
    row(f"scatter, all {N * ns} indices equal, B {B} C {C}", lambda: _scatter_grad(go, one, None, N, 1),
        lambda: torch_scatter(go, one, None, N, 1))

    def with_grad(fn, x):
        def run():
            y = x.detach().requires_grad_()
            fn(y).backward()
        return run
    row(f"get_uniform_loss forward + backward B {B} N {N}", with_grad(muc.get_uniform_loss, pcd), with_grad(torch_uniform, pcd))
    small = pcd * 0.5
    row(f"get_repulsion_loss forward + backward B {B} N {N}", with_grad(muc.get_repulsion_loss, small),
        with_grad(torch_repulsion, small))
    lines.append("# wave-per-centre against a lane-per-centre ball query: not measured (no lane-per-centre variant was built)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
