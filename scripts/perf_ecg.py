#!/usr/bin/env python3
"""ECG completion network at the config's shape (B = 32, num_input = 2048, num_coarse = 1024, num_points = 2048: 3072 encoder
points, scale 1): houv_knn_feat and houv_dense_conv at the two shapes the encoder runs them at (C = 24 / N = 3072 and C = 48 /
N = 1024, k = 16) and the whole Model forward, each beside the reference's own formulation composed from torch ops on the same
device (the [B, N, N] expanded-form distance matrix + topk; the [B, 2C, N, 16] edge tensor and its three growing concatenations).
The point ops both sides need (FPS, gather, three_nn, three_interpolate) are this library's in both.  Median of RUNS timed runs
after WARM warm-up calls, device events.

    python scripts/perf_ecg.py [--out profiles/r10_perf_ecg.txt]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ecg_weights  # noqa: E402
from houv_amd import _lib, ops  # noqa: E402
from houv_amd import model_utils_completion as muc  # noqa: E402
from houv_amd.mm3d_pn2 import three_interpolate  # noqa: E402
from houv_amd.models import ecg  # noqa: E402

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


def torch_knn(x, k):
    """The reference's ranking: the expanded form on x[B,C,N], the [B,N,N] matrix materialised, topk."""
    inner = -2 * torch.matmul(x.transpose(2, 1).contiguous(), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    return (-xx - inner - xx.transpose(2, 1).contiguous()).topk(k=k, dim=-1)[1]


def torch_graph_feature(x, idx):
    B, C, N = x.shape
    k = idx.shape[2]
    rows = x.transpose(2, 1).contiguous()
    flat = (idx + torch.arange(B, device=x.device).view(-1, 1, 1) * N).view(-1)
    feature = rows.view(B * N, C)[flat].view(B, N, k, C)
    centre = rows.view(B, N, 1, C).repeat(1, 1, k, 1)
    return torch.cat((centre, feature - centre), dim=3).permute(0, 3, 1, 2)


def torch_dense(dc, x, idx=None):
    """Dense_conv.forward as the reference writes it: x[B,C,N] -> [B,C+72,N]."""
    k = dc.k
    idx = torch_knn(x, k) if idx is None else idx
    c1, c2 = dc.model.stack_conv_1.model.conv, dc.model.stack_conv_2.model.conv
    y = F.relu(F.conv2d(torch_graph_feature(x, idx), dc.first_conv.weight, dc.first_conv.bias))
    y = torch.cat((y, x.unsqueeze(3).repeat(1, 1, 1, k)), 1)
    y = torch.cat((y, F.relu(F.conv2d(y, c1.weight, c1.bias))), 1)
    y = torch.cat((y, F.conv2d(y, c2.weight, c2.bias)), 1)
    return y.max(3)[0]


def torch_model(net, x):
    """Model.forward ("test") in the reference's formulation, channel-major, scale 1."""
    pe, d = net.encoder, net.decoder
    e = d.encoder
    c = lambda m, t: F.conv1d(t, m.weight, m.bias)
    B, _, N = x.shape
    y = c(pe.conv2, F.relu(c(pe.conv1, x)))
    g = y.max(2)[0]
    y = torch.cat((y, g.view(B, -1, 1).repeat(1, 1, N)), 1)
    feat = c(pe.conv4, F.relu(c(pe.conv3, y))).max(2)[0]
    coarse = F.linear(F.relu(F.linear(F.relu(F.linear(feat, d.fc1.weight, d.fc1.bias)), d.fc2.weight, d.fc2.bias)), d.fc3.weight,
                      d.fc3.bias).view(B, 3, d.num_coarse)
    pts = torch.cat((coarse, x), 2)
    pc1 = pts.transpose(1, 2).contiguous()
    x0 = F.relu(c(e.conv1, pts))
    x1 = torch.cat((F.relu(torch_dense(e.dense_conv1, x0)), x0), 1)
    x1d, _, _, pc2 = muc.edge_preserve_sampling(x1, pc1, e.hierarchy[0], e.k)
    x2 = torch.cat((F.relu(torch_dense(e.dense_conv2, F.relu(c(e.conv2, x1d)))), x1d), 1)
    x2d, _, _, pc3 = muc.edge_preserve_sampling(x2, pc2, e.hierarchy[1], e.k)
    x3 = torch.cat((F.relu(torch_dense(e.dense_conv3, F.relu(c(e.conv3, x2d)))), x2d), 1)
    x3d, _, _, pc4 = muc.edge_preserve_sampling(x3, pc3, e.hierarchy[2], e.k)
    x4 = torch.cat((F.relu(torch_dense(e.dense_conv4, F.relu(c(e.conv4, x3d)))), x3d), 1)
    gf = c(e.gf_conv, x4).max(-1)[0]
    gf = F.relu(F.linear(F.relu(F.linear(gf, e.fc1.weight, e.fc1.bias)), e.fc2.weight, e.fc2.bias))
    x4 = F.relu(c(e.conv5, torch.cat((gf.unsqueeze(2).repeat(1, 1, e.hierarchy[2]), x4), 1)))
    x4 = three_interpolate(x4.contiguous(), *muc.three_nn_upsampling(pc3, pc4))
    x3 = F.relu(c(e.conv6, torch.cat((x3, x4), 1)))
    x3 = three_interpolate(x3.contiguous(), *muc.three_nn_upsampling(pc2, pc3))
    x2 = F.relu(c(e.conv7, torch.cat((x2, x3), 1)))
    x2 = three_interpolate(x2.contiguous(), *muc.three_nn_upsampling(pc1, pc2))
    dense = c(e.conv8, torch.cat((x1, x2), 1))
    fine = c(d.conv2, F.relu(c(d.conv1, dense)))
    if fine.shape[2] > d.num_fine:
        idx = muc.furthest_point_sample(fine.transpose(1, 2).contiguous(), d.num_fine)
        fine = muc.gather_points(fine.contiguous(), idx)
    return coarse.transpose(1, 2).contiguous(), fine.transpose(1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, num_input, num_coarse, num_points = args.batch, 2048, 1024, 2048
    net = ecg.Model(ecg_weights.args(num_points), num_coarse=num_coarse, num_input=num_input)
    net.load_state_dict({k: torch.tensor(v) for k, v in ecg_weights.make_state(num_coarse, 1).items()}, strict=True)
    net = net.to(dev).eval()
    enc = net.decoder.encoder
    g = torch.Generator().manual_seed(10)
    x = (torch.rand(B, 3, num_input, generator=g) - 0.5).to(dev)
    lines = [f"build {_lib.build_id()}  B={B} num_input={num_input} num_coarse={num_coarse} num_points={num_points}  median of {RUNS} "
             f"after {WARM} warm-up calls, device events"]

    def line(what, a, b):
        lines.append(f"{what:38s}{a:9.3f} ms   torch composition {b:9.3f} ms   ratio {b / a:6.2f}x")
    with torch.no_grad():
        for dc, C, N in ((enc.dense_conv1, 24, num_coarse + num_input), (enc.dense_conv2, 48, 1024)):
            rows = torch.randn(B, N, C, generator=g).to(dev)
            cm = rows.transpose(1, 2).contiguous()
            line(f"knn_feat C={C} N={N} k=16", timed(lambda: ops.knn_feat(rows, 16)), timed(lambda: torch_knn(cm, 16)))
            idx = ops.knn_feat(rows, 16)
            idx64 = idx.long()
            c1, c2 = dc.model.stack_conv_1.model.conv, dc.model.stack_conv_2.model.conv
            a = timed(lambda: ops.dense_conv(rows, idx, dc.first_conv.matrix(), dc.first_conv.bias, c1.matrix(), c1.bias, c2.matrix(),
                                             c2.bias))
            line(f"dense_conv C={C} N={N} k=16", a, timed(lambda: torch_dense(dc, cm, idx64)))
        a = timed(lambda: net(x, prefix="test"))
        b = timed(lambda: torch_model(net, x))
        line("Model forward", a, b)
        own, ref = net(x, prefix="test")["result"], torch_model(net, x)[1]
        lines.append(f"Model forward: {B / a * 1e3:.0f} clouds/s; shapes {tuple(own.shape)} / {tuple(ref.shape)} (the two take different "
                     f"near-tie decisions, so their outputs are not compared here: tests/test_gpu_ecg.py)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
