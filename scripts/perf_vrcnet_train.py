#!/usr/bin/env python3
"""SA_module(trainable=True) at the four levels of the shipped VRCNet config (B = 24, k = 16; C x N = 64 x 3072, 128 x 1536,
256 x 768, 512 x 384): the forward that keeps its graph, the backward of L = <G, out>, and the peak memory of forward + backward,
two ways -- the fused node (houv_gemm_f32 + houv_sa_attn forward, houv_sa_attn_backward backward) and the reference's
materialising form composed from torch ops with autograd (perf_vrcnet.torch_sa) on the same device in the same run.  The
baseline of every row is the torch form, never an earlier build of these kernels.  Median of RUNS timed runs after WARM warm-up
runs, device events; peak memory is torch's allocator peak over one forward + backward, above what is allocated before it.

    python scripts/perf_vrcnet_train.py [--out profiles/perf_vrcnet_train.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import vrcnet_cases as cases  # noqa: E402
from perf_vrcnet import LEVELS, RUNS, WARM, timed, torch_sa  # noqa: E402
from houv_amd import _lib, ops  # noqa: E402
from houv_amd.models import vrcnet  # noqa: E402


def measure(forward, params, G):
    """-> (forward ms, backward ms, peak MiB of forward + backward) of L = <G, forward()>."""
    def clear():
        for p in params:
            p.grad = None
    fw, bw = [], []
    for run in range(WARM + RUNS):
        clear()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        out = forward()
        e[1].record()
        (out * G).sum().backward()
        e[2].record()
        torch.cuda.synchronize()
        if run >= WARM:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
        del out
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = forward()
    (out * G).sum().backward()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    del out
    clear()
    return statistics.median(fw), statistics.median(bw), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=24)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, k = args.batch, 16
    g = torch.Generator().manual_seed(28)
    lines = [f"build {_lib.build_id()}  B={B} k={k}  median of {RUNS} after {WARM} warm-up runs, device events; "
             "this = SA_module(trainable=True), torch = the materialising form with autograd"]
    for C, N in LEVELS:
        sa = vrcnet.SA_module(C, C // 16, C // 4, C, 8, k, trainable=True)
        sa.load_state_dict({n: torch.tensor(v) for n, v in cases.sa_state(C, k).items()}, strict=True)
        sa = sa.to(dev)
        params = list(sa.parameters())
        rows = torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True)
        idx = ops.knn(torch.rand(B, N, 3, generator=g).to(dev), k)
        G = torch.randn(B, N, C, generator=g).to(dev)
        cm = rows.detach().transpose(1, 2).unsqueeze(2).contiguous().requires_grad_(True)
        Gc, idx64 = G.transpose(1, 2).unsqueeze(2).contiguous(), idx.long()
        a = measure(lambda: sa.forward_rows(rows, idx), params + [rows], G)
        b = measure(lambda: torch_sa(sa, cm, idx64), params + [cm], Gc)
        # the same gradients, to float32 rounding
        sa.forward_rows(rows, idx).mul(G).sum().backward()
        mine = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        torch_sa(sa, cm, idx64).mul(Gc).sum().backward()
        rel = max(float((m - p.grad).norm() / p.grad.norm()) for m, p in zip(mine, params))
        for p in params + [rows, cm]:
            p.grad = None
        P = torch.randn(B, N, 3 * C // 8, generator=g).to(dev)
        Gm = torch.randn(B, N, C // 4, generator=g).to(dev)
        w = (sa.conv_w[1].matrix().detach(), sa.conv_w[3].matrix().detach(), sa.conv_w[3].bias.detach())
        kern = timed(lambda: ops.sa_attn_backward(P, idx, *w, Gm))
        ws = _lib.load().houv_sa_attn_backward_workspace_bytes(B, N, C, k) / 2 ** 20
        slower = [n for n, x, y in (("forward", a[0], b[0]), ("backward", a[1], b[1])) if x > y]
        note = f"   <- the fused {' and '.join(slower)} is SLOWER here" if slower else ""
        lines.append(f"SA_module C={C:3d} N={N:4d}: forward {a[0]:7.3f} / {b[0]:7.3f} ms ({b[0] / a[0]:4.2f}x)   backward {a[1]:7.3f} / "
                     f"{b[1]:7.3f} ms ({b[1] / a[1]:4.2f}x)   peak {a[2]:7.1f} / {b[2]:7.1f} MiB ({b[2] / a[2]:4.1f}x)   this / torch{note}")
        lines.append(f"    houv_sa_attn_backward alone {kern:.3f} ms (workspace {ws:.1f} MiB); largest relative L2 difference of a "
                     f"parameter gradient between the two {rel:.1e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
