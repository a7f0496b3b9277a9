#!/usr/bin/env python3
"""PCN training at the config's shape (B = 32, N = 2048, num_points 2048, num_coarse 1024): the encoder's
active-rows backward, the folding stage's recomputing backward and one whole training step (forward + backward + Adam on
total_train_loss, loss cd, alpha 0.5) of models.pcn.Model(trainable=True), each beside the reference's own formulation composed
from torch ops with autograd on the same device in the same script (dense [B,1024,N] / [B,512,N] gradients, the concatenated
[B,1029,2048] feature kept for its backward).  Both sides take the loss from the same calc_cd.  Reported for both: the forward
that keeps what its backward needs, the backward alone, a step with Adam, torch.cuda.max_memory_allocated over a step, and --
from houv_mlp2_max_arg -- the distinct critical points per cloud under the seeded weights.  Median of RUNS timed runs after WARM
warm-up calls, device events.

    python scripts/perf_pcn_train.py [--out profiles/perf_pcn_train.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcn_weights  # noqa: E402
from houv_amd import _lib, ops  # noqa: E402
from houv_amd.model_utils_completion import calc_cd  # noqa: E402
from houv_amd.models import pcn  # noqa: E402
from perf_pcn import RUNS, WARM, timed, torch_block1, torch_block2, torch_fold, torch_model  # noqa: E402


def measure(net, forward, step=True):
    """(forward ms, backward ms, step ms, peak MiB over a step, gradients) of the scalar `forward()` over net's parameters."""
    fwd = timed(forward)

    def backward_ms():
        for p in net.parameters():
            p.grad = None
        loss = forward()                                     # a fresh graph, built outside the timed region
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); loss.backward(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    ms = sorted([backward_ms() for _ in range(RUNS + WARM)][WARM:])
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    whole = peak = float("nan")
    if step:
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        saved = {k: v.clone() for k, v in net.state_dict().items()}

        def one():
            opt.zero_grad(set_to_none=True)
            forward().backward()
            opt.step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        whole = timed(one)
        peak = torch.cuda.max_memory_allocated() / 2 ** 20
        net.load_state_dict(saved, strict=True)              # the timed steps moved the weights: put them back
    return fwd, ms[len(ms) // 2], whole, peak, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N = args.batch, args.points
    num_points, num_coarse = 2048, 1024
    state = {k: torch.tensor(v) for k, v in pcn_weights.make_state(num_coarse).items()}
    own = pcn.Model(pcn_weights.args(num_points), num_coarse=num_coarse, trainable=True)
    ref = pcn.Model(pcn_weights.args(num_points), num_coarse=num_coarse)          # the same parameters, driven through torch ops
    for net in (own, ref):
        net.load_state_dict(state, strict=True)
        net.to(dev)
        net.decoder.grid = net.decoder.grid.to(dev)
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(B, 3, N, generator=g) - 0.5).to(dev)
    gt = (torch.rand(B, num_points, 3, generator=g) - 0.5).to(dev)
    rows = x.transpose(1, 2).contiguous()
    G = (torch.rand(B, 1024, generator=g) - 0.5).to(dev)
    Gf = (torch.rand(B, num_points, 3, generator=g) - 0.5).to(dev)
    with torch.no_grad():
        feat = own.encoder(rows)
        coarse = own.decoder(feat)[0]
        coarse_cm = coarse.transpose(1, 2).contiguous()

    def ref_encoder():
        g1, y = torch_block1(ref.encoder, x)
        return (torch_block2(ref.encoder, y, g1) * G).sum()

    def own_fold():
        d = own.decoder
        with torch.no_grad():
            Wgp = d.conv1.columns(0, 5)
        return (pcn._FoldFunction.apply(coarse, feat, d.grid, d.conv1.matrix(), d.conv1.bias, Wgp, d.conv2.matrix(), d.conv2.bias,
                                        d.conv3.matrix(), d.conv3.bias) * Gf).sum()

    def ref_total():
        out1, out2 = torch_model(ref, x)
        return calc_cd(out1, gt)[0].mean() + calc_cd(out2, gt)[0].mean() * 0.5
    parts = [("encoder, loss <G, feat>", lambda: (own.encoder(rows) * G).sum(), own.encoder, ref_encoder, ref.encoder, True),
             ("fold (+cvec), loss <G, fine>", own_fold, own.decoder, lambda: (torch_fold(ref.decoder, coarse_cm, feat).transpose(1, 2) * Gf).sum(),
              ref.decoder, False),
             ("whole model, total_train_loss", lambda: own(x, gt, prefix="train", alpha=0.5)[2], own, ref_total, ref, True)]
    lines = [f"build {_lib.build_id()}  B={B} N={N} num_points={num_points} num_coarse={num_coarse}  median of {RUNS} after {WARM} "
             f"warm-up calls, device events; 'torch' = the reference's formulation composed from torch ops with autograd"]
    for what, fa, na, fb, nb, step in parts:
        a, b = measure(na, fa, step), measure(nb, fb, step)
        lines.append(what)
        rows_ = [("forward (keeps its graph)", 0, "ms"), ("backward", 1, "ms")]
        if step:
            rows_ += [("step: forward + backward + Adam", 2, "ms"), ("peak memory over a step", 3, "MiB")]
        for label, i, unit in rows_:
            lines.append(f"  {label:34s}{a[i]:10.3f} {unit:3s}  torch {b[i]:10.3f} {unit:3s}  ratio {b[i] / a[i]:6.2f}x")
        worst = max(float((a[4][k] - b[4][k]).abs().max() / b[4][k].abs().max()) for k in a[4])
        lines.append(f"  gradients against torch's: largest difference relative to a tensor's largest entry {worst:.3g}")
    e = own.encoder
    with torch.no_grad():
        g1, arg1, y = ops.mlp2_max_arg(rows, e.conv1.matrix(), e.conv1.bias, e.conv2.matrix(), e.conv2.bias, want_y=True)
        shift1 = ops.gemm(g1, e.conv3.matrix()[:, 256:], shift=e.conv3.bias)
        _, arg2, _ = ops.mlp2_max_arg(y, e.conv3.columns(0, 256), shift1, e.conv4.matrix(), e.conv4.bias)
    n1 = [len(torch.unique(arg1[i])) for i in range(B)]
    n2 = [len(torch.unique(arg2[i])) for i in range(B)]
    both = [len(torch.unique(torch.cat((arg1[i], arg2[i])))) for i in range(B)]
    lines.append(f"distinct critical points per cloud (uniform random clouds, seeded weights): block 1 {min(n1)}..{max(n1)} of <= 256, "
                 f"block 2 {min(n2)}..{max(n2)} of <= 1024, union {min(both)}..{max(both)} of <= 1280 (N = {N})")
    lines.append(f"houv_pcn_fold_backward workspace at this shape: {_lib.load().houv_pcn_fold_backward_workspace_bytes(B, num_coarse, num_points // num_coarse) / 2 ** 20:.0f} MiB")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
