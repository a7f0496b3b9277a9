#!/usr/bin/env python3
"""IDAM head at the config's shape (B = 32, N = 2048, M = 341): houv_idam_simmat per call, a Propagate stack per cloud and the
Model forward, each beside the same formulas composed from torch ops on the same device (the reference's own formulation, the
concatenated [B, 2E+4, M, M] tensor included, chunked over the batch).  Median of RUNS timed runs after WARM warm-up calls, device events.  The similarity timing uses
standard-normal embeddings, not the model's (which span about +-100): the kernel's time does not depend on the values.

    python scripts/perf_idam.py [--out profiles/r08_perf_idam.txt]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import idam_weights  # noqa: E402
from houv_amd import _lib, ops  # noqa: E402
from houv_amd.models import idam  # noqa: E402


RUNS, WARM = 5, 2


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


def torch_simmat(src, tgt, es, et, par, chunk=4):
    """idam.py:267-320 as written: repeat + cat, four 1x1 Conv2d layers (BatchNorm folded), row max and row arg-max."""
    W1, s1, t1, W2, b2, W3, s3, t3, w4, b4 = par
    outs = []
    for c in range(0, src.shape[0], chunk):
        s, t = src[c:c + chunk].transpose(1, 2), tgt[c:c + chunk].transpose(1, 2)
        a, b = es[c:c + chunk].transpose(1, 2), et[c:c + chunk].transpose(1, 2)
        M = s.shape[2]
        x = torch.cat([a.unsqueeze(-1).repeat(1, 1, 1, M), b.unsqueeze(-2).repeat(1, 1, M, 1)], 1)
        diff = s.unsqueeze(-1) - t.unsqueeze(-2)
        dist = torch.sqrt((diff ** 2).sum(1, keepdim=True))
        x = torch.cat([x, dist, diff / (dist + 1e-8)], 1)
        h = F.relu(F.conv2d(x, W1[:, :, None, None]) * s1[None, :, None, None] + t1[None, :, None, None])
        h = F.conv2d(h, W2[:, :, None, None], b2)
        rowmax = h.max(-1)[0]
        h = F.relu(F.conv2d(h, W3[:, :, None, None]) * s3[None, :, None, None] + t3[None, :, None, None])
        sc = F.conv2d(h, w4[None, :, None, None], b4).squeeze(1).clamp(min=-20, max=20)
        outs.append((rowmax, sc.max(-1)[1]))
    return outs


def torch_propagate(p, x, idx):
    """idam.py:121-128 as written, on [B,C,N]."""
    bi = torch.arange(x.size(0), device=x.device).view(-1, 1, 1)
    d = x[bi, :, idx.long()].permute(0, 3, 1, 2) - x.unsqueeze(-1)
    first, second = p.conv2d.conv
    s, h = first.bn.folded()
    a = F.relu(F.conv2d(d, first.conv.weight) * s[None, :, None, None] + h[None, :, None, None])
    a = F.conv2d(a, second.weight, second.bias).max(-1)[0]
    last = p.conv1d.conv[0]
    return F.conv1d(a, last.weight, last.bias)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N = args.batch, args.points
    M = N // 6
    net = idam.Model(idam_weights.Args)
    net.load_state_dict({k: torch.tensor(v) for k, v in idam_weights.make_state().items()}, strict=False)
    net = net.to(dev)
    g = torch.Generator().manual_seed(3)
    src = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev)
    tgt = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev)
    ks, kt = src[:, :M].contiguous(), tgt[:, :M].contiguous()
    es, et = torch.randn(B, M, 64, generator=g).to(dev), torch.randn(B, M, 64, generator=g).to(dev)
    par = net.simmat_params(0)
    lines = [f"build {_lib.build_id()}  B={B} N={N} M={M}  median of {RUNS} after {WARM} warm-up calls, device events"]
    with torch.no_grad():
        a = timed(lambda: ops.idam_simmat(ks, kt, es, et, *par))
        b = timed(lambda: torch_simmat(ks, kt, es, et, par))
        lines.append(f"idam_simmat           {a:9.3f} ms   torch composition {b:9.3f} ms   ratio {b / a:7.1f}x")
        idx = idam.knn_idx(src)
        a = timed(lambda: net.emb_nn(src, idx))
        xt = src.transpose(1, 2).contiguous()

        def stack():
            x = xt
            for p in (net.emb_nn.propogate1, net.emb_nn.propogate2, net.emb_nn.propogate3, net.emb_nn.propogate4, net.emb_nn.propogate5):
                x = torch_propagate(p, x, idx)
            return x
        b = timed(stack)
        lines.append(f"Propagate x5 / cloud  {a:9.3f} ms   torch composition {b:9.3f} ms   ratio {b / a:7.1f}x")
        a = timed(lambda: net(src, tgt, prefix="test"))
        lines.append(f"Model forward         {a:9.3f} ms   {B / a * 1e3:9.1f} pairs/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
