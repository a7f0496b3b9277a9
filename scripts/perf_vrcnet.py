#!/usr/bin/env python3
"""VRCNet at the shipped config's shape (B = 24, 1024 + 2048 encoder points, k = 16): SA_module at the encoder's four levels
(C x N = 64 x 3072, 128 x 1536, 256 x 768, 512 x 384) two ways -- houv_gemm_f32 + houv_sa_attn (SA_module.forward_rows), and the
reference's materialising form restated in torch below (the [B, C, k, N] edge tensor, its two projections, the repeated weight
tensor) on the same device -- and the whole "test" forward of models.vrcnet.Model.  The baseline of every row is the torch
form, never an earlier run of the kernel.  Median of RUNS timed runs after WARM warm-up calls, device events.

    python scripts/perf_vrcnet.py [--out profiles/perf_vrcnet.txt]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vrcnet_cases as cases  # noqa: E402
from vrcnet_cases import vrcnet_weights as W  # noqa: E402
from houv_amd import _lib, ops  # noqa: E402
from houv_amd.models import vrcnet  # noqa: E402

RUNS, WARM = 7, 3
LEVELS = ((64, 3072), (128, 1536), (256, 768), (512, 384))


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def torch_sa(sa, x, idx):
    """SA_module.forward as the reference writes it: x[B,C,1,N], idx[B,N,k] int64 -> [B,C,1,N]."""
    B, C, _, N = x.shape
    k = idx.shape[2]
    identity = x
    x = F.relu(x)
    flat = (idx + torch.arange(B, device=x.device).view(-1, 1, 1) * N).view(-1)
    xn = x.squeeze(2).transpose(2, 1).contiguous().view(B * N, C)[flat].view(B, N, k, C).permute(0, 3, 2, 1)      # B C K N
    c = lambda m, t: F.conv2d(t, m.weight, getattr(m, "bias", None))
    x1, x2, x3 = c(sa.conv1, x), c(sa.conv2, xn), c(sa.conv3, xn)
    x2 = x2.reshape(B, -1, 1, N).contiguous()
    w = c(sa.conv_w[3], F.relu(c(sa.conv_w[1], F.relu(torch.cat([x1, x2], 1))))).view(B, -1, k, N)
    w = w.repeat(1, sa.share_planes, 1, 1)
    out = torch.sum(w * x3, dim=2, keepdim=True)
    return c(sa.conv_out, F.relu(out)) + identity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=24)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, k = args.batch, 16
    g = torch.Generator().manual_seed(27)
    lines = [f"build {_lib.build_id()}  B={B} k={k}  median of {RUNS} after {WARM} warm-up calls, device events"]
    with torch.no_grad():
        for C, N in LEVELS:
            sa = vrcnet.SA_module(C, C // 16, C // 4, C, 8, k)
            sa.load_state_dict({n: torch.tensor(v) for n, v in cases.sa_state(C, k).items()}, strict=True)
            sa = sa.to(dev).eval()
            rows = torch.randn(B, N, C, generator=g).to(dev)
            idx = ops.knn(torch.rand(B, N, 3, generator=g).to(dev), k)
            cm, idx64 = rows.transpose(1, 2).unsqueeze(2).contiguous(), idx.long()
            a = timed(lambda: sa.forward_rows(rows, idx))
            b = timed(lambda: torch_sa(sa, cm, idx64))
            err = float((sa.forward_rows(rows, idx) - torch_sa(sa, cm, idx64).squeeze(2).transpose(1, 2)).abs().max())
            note = "" if a <= b else "   <- the fused path is SLOWER here"
            lines.append(f"SA_module C={C:3d} N={N:4d} k={k}  gemm + sa_attn {a:8.3f} ms   torch materialising {b:8.3f} ms   ratio "
                         f"{b / a:5.2f}x   max |difference| {err:.2e}{note}")
        c = cases.MODEL_CASES["a"]
        net = vrcnet.Model(W.args(c))
        net.load_state_dict({n: torch.tensor(v) for n, v in cases.model_state("a").items()}, strict=True)
        net = net.to(dev).eval()
        x = (torch.rand(B, 3, c.num_input, generator=g) - 0.5).to(dev)
        z = torch.randn(B, net.size_z, generator=g).to(dev)
        a = timed(lambda: net(x, prefix="test", z=z))
        lines.append(f'Model forward ("test", the shipped cfg)  {a:8.3f} ms   {B / a * 1e3:.0f} clouds/s   result '
                     f'{tuple(net(x, prefix="test", z=z)["result"].shape)}')
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
