#!/usr/bin/env python3
"""ECG training at the config's shape (B = 32, num_input 2048, num_coarse 1024, num_points 2048, k = 16):
the fused Dense_conv node (houv_dense_conv_arg forward, houv_dense_conv_backward backward) at the two shapes the encoder runs it
at (C = 24 / N = 3072 and C = 48 / N = 1024) and one whole training step (forward + backward + Adam on total_train_loss, loss
cd, alpha 0.5) of models.ecg.Model(trainable=True), each beside the reference's materialising form composed from torch ops with
autograd on the same device in the same script (perf_ecg.torch_dense / torch_model: the [B, 2C, N, 16] edge tensor and the three
growing concatenations kept for the backward).  Both sides use the same neighbour lists (Dense_conv alone) and the same losses
(the step).  Reported for both: the forward that keeps what its backward needs, the backward alone, the peak of
torch.cuda.max_memory_allocated over forward + backward above what was allocated before, and the backward kernels alone.
Median of RUNS timed runs after WARM warm-up calls, device events.

    python scripts/perf_ecg_train.py [--out profiles/perf_ecg_train.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ecg_weights  # noqa: E402
from houv_amd import _lib, ops  # noqa: E402
from houv_amd.model_utils_completion import calc_cd, get_uniform_loss  # noqa: E402
from houv_amd.models import ecg  # noqa: E402
from perf_ecg import RUNS, WARM, timed, torch_dense, torch_model  # noqa: E402


def measure(params, forward):
    """(forward ms, backward ms, peak MiB of forward + backward above the resident tensors) of the scalar `forward()`."""
    fwd = timed(forward)

    def backward_ms():
        for p in params:
            p.grad = None
        loss = forward()                                     # a fresh graph, built outside the timed region
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); loss.backward(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    ms = sorted([backward_ms() for _ in range(RUNS + WARM)][WARM:])
    for p in params:
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    forward().backward()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    grads = [p.grad.clone() for p in params]
    return fwd, ms[len(ms) // 2], peak, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, num_input, num_coarse, num_points, k = args.batch, 2048, 1024, 2048, 16
    state = {n: torch.tensor(v) for n, v in ecg_weights.make_state(num_coarse, 1).items()}
    own = ecg.Model(ecg_weights.args(num_points), num_coarse=num_coarse, num_input=num_input, trainable=True)
    ref = ecg.Model(ecg_weights.args(num_points), num_coarse=num_coarse, num_input=num_input)   # the same parameters, driven through torch ops
    for net in (own, ref):
        net.load_state_dict(state, strict=True)
        net.to(dev)
    g = torch.Generator().manual_seed(9)
    lines = [f"build {_lib.build_id()}  B={B} num_input={num_input} num_coarse={num_coarse} num_points={num_points} k={k}  median of "
             f"{RUNS} after {WARM} warm-up calls, device events; 'torch' = the reference's materialising form composed from torch ops "
             f"with autograd"]
    for C, N, name in ((24, num_coarse + num_input, "dense_conv1"), (48, 1024, "dense_conv2")):
        dc_own, dc_ref = getattr(own.decoder.encoder, name), getattr(ref.decoder.encoder, name)
        rows = (torch.rand(B, N, C, generator=g) - 0.5).to(dev).requires_grad_(True)
        xcm = rows.detach().transpose(1, 2).contiguous().requires_grad_(True)
        G = (torch.rand(B, N, C + 72, generator=g) - 0.5).to(dev)
        Gcm = G.transpose(1, 2).contiguous()
        idx = ops.knn_feat(rows.detach(), k)
        w = dc_own._weights()
        a = measure([rows] + list(dc_own.parameters()), lambda: (ecg._DenseConvFunction.apply(rows, idx, *w, True)[0] * G).sum())
        b = measure([xcm] + list(dc_ref.parameters()), lambda: (torch.relu(torch_dense(dc_ref, xcm, idx.long())) * Gcm).sum())
        with torch.no_grad():
            out, arg = ops.dense_conv_arg(rows.detach(), idx, *w, relu_out=True)
            kern = timed(lambda: ops.dense_conv_backward(rows.detach(), idx, *w, arg, G, out=out, relu_out=True))
            fwd_plain = timed(lambda: ops.dense_conv(rows.detach(), idx, *w, relu_out=True))
        ws = _lib.load().houv_dense_conv_backward_workspace_bytes(B, N, C, k) / 2 ** 20
        lines.append(f"Dense_conv C={C} N={N} (relu_out), loss <G, out>")
        for label, i, unit in (("forward (keeps what backward needs)", 0, "ms"), ("backward", 1, "ms"), ("peak memory, forward + backward", 2, "MiB")):
            lines.append(f"  {label:38s}{a[i]:10.3f} {unit:3s}  torch {b[i]:10.3f} {unit:3s}  ratio {b[i] / a[i]:6.2f}x")
        lines.append(f"  houv_dense_conv_backward alone {kern:.3f} ms (workspace {ws:.0f} MiB); houv_dense_conv alone {fwd_plain:.3f} ms")
        pairs = [(a[3][0], b[3][0].transpose(1, 2))] + [(p, q.view(p.shape)) for p, q in zip(a[3][1:], b[3][1:])]
        worst = max(float((p - q).abs().max() / q.abs().max()) for p, q in pairs)
        lines.append(f"  gradients against torch's: largest difference relative to a tensor's largest entry {worst:.3g}")
        del rows, xcm, G, Gcm, a, b, out, arg
        torch.cuda.empty_cache()

    x = (torch.rand(B, 3, num_input, generator=g) - 0.5).to(dev)
    gt = (torch.rand(B, num_points, 3, generator=g) - 0.5).to(dev)

    def ref_total():
        out1, out2 = torch_model(ref, x)
        return (calc_cd(out1, gt)[0].mean() + get_uniform_loss(out1).mean() * 0.1
                + (calc_cd(out2, gt)[0].mean() + get_uniform_loss(out2).mean() * 0.1) * 0.5)
    lines.append("whole model, total_train_loss (cd + uniform)")
    res = []
    for net, forward in ((own, lambda: own(x, gt, prefix="train", alpha=0.5)[2]), (ref, ref_total)):
        fwd, bwd, peak, _ = measure(list(net.parameters()), forward)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)

        def one():
            opt.zero_grad(set_to_none=True)
            forward().backward()
            opt.step()
        res.append((fwd, bwd, timed(one), peak))
        del opt
        for p in net.parameters():
            p.grad = None
        torch.cuda.empty_cache()
    for label, i, unit in (("forward (keeps its graph)", 0, "ms"), ("backward", 1, "ms"), ("step: forward + backward + Adam", 2, "ms"),
                           ("peak memory, forward + backward", 3, "MiB")):
        lines.append(f"  {label:38s}{res[0][i]:10.3f} {unit:3s}  torch {res[1][i]:10.3f} {unit:3s}  ratio {res[1][i] / res[0][i]:6.2f}x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
