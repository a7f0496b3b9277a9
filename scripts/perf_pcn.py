#!/usr/bin/env python3
"""PCN completion network at the config's shape (B = 32, N = 2048 input points, num_points = 2048, num_coarse = 1024): each
houv_mlp2_max stage, houv_pcn_fold and the whole Model forward, each beside the reference's own formulation composed from torch
ops on the same device (the repeated + concatenated [B, 512, N] and [B, 1029, 2048] features and the materialised [B, 1024, N]
activations included).  Median of RUNS timed runs after WARM warm-up calls, device events.

    python scripts/perf_pcn.py [--out profiles/r09_perf_pcn.txt]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import pcn_weights  # noqa: E402
from houv_amd import _lib, ops  # noqa: E402
from houv_amd.models import pcn  # noqa: E402

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


def torch_block1(enc, x):
    """pcn.py:22-24 on x[B,3,N]."""
    y = F.conv1d(F.relu(F.conv1d(x, enc.conv1.weight, enc.conv1.bias)), enc.conv2.weight, enc.conv2.bias)
    return y.max(2)[0], y


def torch_block2(enc, y, g):
    """pcn.py:25-29."""
    B, _, N = y.shape
    x = torch.cat((y, g.view(B, -1, 1).repeat(1, 1, N).contiguous()), 1)
    x = F.conv1d(F.relu(F.conv1d(x, enc.conv3.weight, enc.conv3.bias)), enc.conv4.weight, enc.conv4.bias)
    return x.max(2)[0]


def torch_fold(dec, coarse, feat):
    """pcn.py:108-125 on coarse[B,3,nc], feat[B,1024]."""
    B = feat.shape[0]
    grid_feat = dec.grid.unsqueeze(0).repeat(B, 1, dec.num_coarse).contiguous()
    point_feat = coarse.transpose(1, 2).contiguous().unsqueeze(2).repeat(1, 1, dec.scale, 1).view(-1, dec.num_fine, 3).transpose(1, 2).contiguous()
    global_feat = feat.unsqueeze(2).repeat(1, 1, dec.num_fine)
    cat = torch.cat((grid_feat, point_feat, global_feat), 1)
    h = F.relu(F.conv1d(F.relu(F.conv1d(cat, dec.conv1.weight, dec.conv1.bias)), dec.conv2.weight, dec.conv2.bias))
    return F.conv1d(h, dec.conv3.weight, dec.conv3.bias) + point_feat


def torch_model(net, x):
    g, y = torch_block1(net.encoder, x)
    feat = torch_block2(net.encoder, y, g)
    d = net.decoder
    c = F.linear(F.relu(F.linear(F.relu(F.linear(feat, d.fc1.weight, d.fc1.bias)), d.fc2.weight, d.fc2.bias)), d.fc3.weight, d.fc3.bias)
    coarse = c.view(-1, 3, d.num_coarse)
    return coarse.transpose(1, 2).contiguous(), torch_fold(d, coarse, feat).transpose(1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N = args.batch, args.points
    num_points, num_coarse = 2048, 1024
    net = pcn.Model(pcn_weights.args(num_points), num_coarse=num_coarse)
    net.load_state_dict({k: torch.tensor(v) for k, v in pcn_weights.make_state(num_coarse).items()}, strict=True)
    net = net.to(dev)
    enc, dec = net.encoder, net.decoder
    dec.grid = dec.grid.to(dev)
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(B, 3, N, generator=g) - 0.5).to(dev)
    rows = x.transpose(1, 2).contiguous()
    lines = [f"build {_lib.build_id()}  B={B} N={N} num_points={num_points} num_coarse={num_coarse}  median of {RUNS} after {WARM} "
             f"warm-up calls, device events"]

    def line(what, a, b):
        lines.append(f"{what:28s}{a:9.3f} ms   torch composition {b:9.3f} ms   ratio {b / a:6.2f}x")
    with torch.no_grad():
        a = timed(lambda: ops.mlp2_max(rows, enc.conv1.matrix(), enc.conv1.bias, enc.conv2.matrix(), enc.conv2.bias, want_y=True))
        b = timed(lambda: torch_block1(enc, x))
        line("mlp2_max 3-128-256 (+y)", a, b)
        g1, y = ops.mlp2_max(rows, enc.conv1.matrix(), enc.conv1.bias, enc.conv2.matrix(), enc.conv2.bias, want_y=True)
        W3 = enc.conv3.matrix()
        y_cm = y.transpose(1, 2).contiguous()

        def second():
            shift1 = ops.gemm(g1, W3[:, 256:], shift=enc.conv3.bias)
            return ops.mlp2_max(y, enc.conv3.columns(0, 256), shift1, enc.conv4.matrix(), enc.conv4.bias)
        a = timed(second)
        b = timed(lambda: torch_block2(enc, y_cm, g1))
        line("mlp2_max 256-512-1024", a, b)
        feat = second()[0]
        coarse, _ = dec(feat)
        coarse_cm = coarse.transpose(1, 2).contiguous()
        W1 = dec.conv1.matrix()

        def fold():
            cvec = ops.gemm(feat, W1[:, 5:], shift=dec.conv1.bias)
            return ops.pcn_fold(coarse, cvec, dec.grid, dec.conv1.columns(0, 5), dec.conv2.matrix(), dec.conv2.bias, dec.conv3.matrix(),
                                dec.conv3.bias)
        a = timed(fold)
        b = timed(lambda: torch_fold(dec, coarse_cm, feat))
        line("pcn_fold (+cvec gemm)", a, b)
        a = timed(lambda: net(x, prefix="test"))
        b = timed(lambda: torch_model(net, x))
        line("Model forward", a, b)
        own, ref = net(x, prefix="test")["result"], torch_model(net, x)[1]
        lines.append(f"Model forward: {B / a * 1e3:.0f} clouds/s; out2 against the torch composition: max abs difference "
                     f"{float((own - ref).abs().max()):.3g} (|out2| up to {float(ref.abs().max()):.3g})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
