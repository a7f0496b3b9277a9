#!/usr/bin/env python3
"""EF_expansion(trainable=True) at the shapes VRCNet's decoder gives it: the forward that keeps its graph,
the backward of L = <G, out>, and the peak memory of forward + backward, two ways -- the graph path (two per-point
_LinearRowsFunction products and one _EFExpandFunction node over houv_ef_expand / houv_ef_expand_backward) and the torch
composition of tests/ef_expand_cases.py (composed_rows: _RowGather, three _LinearRowsFunction products over every edge,
torch.max), on the same device in the same run.  The baseline of every row is that composition, never an earlier build of these
kernels.

Shapes: with num_coarse_raw = 1024, 2048 input points, num_fps = num_coarse = 2048 (cfgs/vrcnet_mi355x.yaml), expansion1
(256 -> 64) sees N = 3072 points with r = up_scale = ceil(num_points / 3072), and expansion2 (64 -> 256, local_folding off) sees
N = 2048 with r = num_points // 2048: num_points 4096 gives r = 2 and 2; 8192 gives r = 3 and 4.  B = 24, k = 4.

Median of RUNS timed runs after WARM warm-up runs, device events, one device; peak memory is torch's allocator peak over one
forward + backward, above what is allocated before it.  Each shape runs in a child process of its own under a time limit.

    python scripts/perf_ef_expand.py [--out profiles/perf_ef_expand.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# (label, C, O, N, r)
SHAPES = (("num_points 4096 expansion1", 256, 64, 3072, 2), ("num_points 4096 expansion2", 64, 256, 2048, 2),
          ("num_points 8192 expansion1", 256, 64, 3072, 3), ("num_points 8192 expansion2", 64, 256, 2048, 4))
K = 4
LIMIT = 240                                      # seconds per shape


def one(i, B):
    import torch
    from ef_expand_cases import composed_rows
    from perf_vrcnet_train import measure
    from houv_amd import model_utils_completion as muc, ops
    label, C, O, N, r = SHAPES[i]
    dev = torch.device("cuda:0")
    if i == 0:
        from perf_vrcnet import RUNS, WARM
        from houv_amd import _lib
        print(f"build {_lib.build_id()}  B={B} k={K}  median of {RUNS} after {WARM} warm-up runs, device events; "
              "this = EF_expansion(trainable=True), torch = composed_rows with autograd")
    torch.manual_seed(31)
    net = muc.EF_expansion(C, O, step_ratio=r, k=K, trainable=True).to(dev)
    gen = torch.Generator().manual_seed(32)
    rows = torch.randn(B, N, C, generator=gen).to(dev).requires_grad_(True)
    idx = ops.knn_feat(rows.detach(), K)
    G = torch.randn(B, N * r, O, generator=gen).to(dev)
    params = list(net.parameters()) + [rows]
    a = measure(lambda: net.forward_rows(rows, idx=idx), params, G)
    b = measure(lambda: composed_rows(net, rows, idx), params, G)
    (net.forward_rows(rows, idx=idx) * G).sum().backward()
    mine, rows.grad = rows.grad.clone(), None
    (composed_rows(net, rows, idx) * G).sum().backward()
    rel = float((mine - rows.grad).norm() / rows.grad.norm())
    slower = [n for n, x, y in (("forward", a[0], b[0]), ("backward", a[1], b[1])) if x > y]
    note = f"   <- the node's {' and '.join(slower)} is SLOWER here" if slower else ""
    print(f"{label} ({C:3d} -> {O:3d}, N={N}, r={r}): forward {a[0]:8.3f} / {b[0]:8.3f} ms ({b[0] / a[0]:4.2f}x)   backward {a[1]:8.3f} / "
          f"{b[1]:8.3f} ms ({b[1] / a[1]:4.2f}x)   peak {a[2]:7.1f} / {b[2]:7.1f} MiB ({b[2] / a[2]:4.1f}x)   this / torch{note}")
    print(f"    relative L2 difference of the input gradient between the two {rel:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--shape", type=int, default=None, help="run one shape in this process (used by the parent)")
    args = ap.parse_args()
    if args.shape is not None:
        return one(args.shape, args.batch)
    lines = []                                   # the parent never touches the device: every shape is a fresh child
    for i in range(len(SHAPES)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(i), "--batch", str(args.batch)],
                               capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            lines.append(f"{SHAPES[i][0]}: no result within {LIMIT} s")
            break
        if p.returncode != 0:                    # nothing more is started on the device after a failure
            lines.append(f"{SHAPES[i][0]}: exit status {p.returncode}\n{p.stderr[-2000:]}")
            break
        lines.append(p.stdout.rstrip())
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
