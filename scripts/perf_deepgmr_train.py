"""Forward + backward time and peak memory of one DeepGMR training step at the cfg's shape (B = 32 pairs x N = 2048 points,
k = 20 neighbours, J = 16 Gaussians), this project's path against the reference's module composition on the same device:

  1. the whole step: models.deepgmr.Model(trainable=True) against nn.Conv1d / nn.BatchNorm1d / nn.ReLU on [B, C, N] with the
     torch gmm_params / gmm_register (torch.linalg.svd on the device -- kinder than the reference, which runs the SVD on the
     host) and torch autograd.  Both get the same precomputed RRI features' worth of work: the features are computed by
     houv_rri_features for both (the reference's own NumPy path is not the subject here);
  2. one BatchNorm layer node (_ConvBNReLUFunction) against Conv1d + BatchNorm1d + ReLU, at the model's widths;
  3. the head node (softmax, gmm_params, gmm_register twice, the 4x4 loss) against its torch composition.

HIP events after warm-up calls; the median of the repeats; peak memory from torch.cuda.max_memory_allocated over one step.

    python scripts/perf_deepgmr_train.py [--reps 7] [--out profiles/perf_deepgmr_train.txt]"""
import argparse
import os
import statistics
import sys
from argparse import Namespace

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from houv_amd import _lib, synthetic  # noqa: E402
from houv_amd.models import deepgmr as dg  # noqa: E402

B, N, K, J = 32, 2048, 20, 16


def _time(fn, reps, warm=2):
    for _ in range(warm):
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


def _peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


# ---- the reference's composition, on the device --------------------------------------------------------------------------
class RefBlock(nn.Sequential):
    def __init__(self, a, b):
        super().__init__(nn.Conv1d(a, b, 1, bias=False), nn.BatchNorm1d(b), nn.ReLU())


class RefPointNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(RefBlock(4 * K, 64), RefBlock(64, 128), RefBlock(128, 256), RefBlock(256, 1024))
        self.decoder = nn.Sequential(RefBlock(2048, 512), RefBlock(512, 256), RefBlock(256, 128), nn.Conv1d(128, J, 1))

    def forward(self, x):                                   # x[B, 4k, N]
        f_loc = self.encoder(x)
        f_glob = f_loc.max(dim=2)[0].unsqueeze(2).expand_as(f_loc)
        return self.decoder(torch.cat([f_loc, f_glob], dim=1)).transpose(1, 2)


def ref_gmm_params(gamma, pts):
    pi = gamma.mean(dim=1)
    npi = pi * gamma.shape[1]
    mu = gamma.transpose(1, 2) @ pts / npi.unsqueeze(2)
    diff = pts.unsqueeze(2) - mu.unsqueeze(1)
    sigma = ((diff.unsqueeze(3) @ diff.unsqueeze(4)).squeeze() * gamma).sum(dim=1) / npi
    return pi, mu, sigma


def ref_gmm_register(pi_s, mu_s, mu_t, sigma_t):
    c_s = pi_s.unsqueeze(1) @ mu_s
    c_t = pi_s.unsqueeze(1) @ mu_t
    Ms = torch.sum((pi_s.unsqueeze(2) * (mu_s - c_s)).unsqueeze(3) @ (mu_t - c_t).unsqueeze(2) / sigma_t[:, :, None, None], dim=1)
    U, _, Vh = torch.linalg.svd(Ms)
    V = Vh.transpose(1, 2)
    S = torch.eye(3, device=U.device).unsqueeze(0).repeat(U.shape[0], 1, 1)
    S[:, 2, 2] = torch.det(V @ U.transpose(1, 2))
    R = V @ S @ U.transpose(1, 2)
    t = c_t.transpose(1, 2) - R @ c_s.transpose(1, 2)
    bot = torch.tensor([[[0., 0., 0., 1.]]], device=R.device).repeat(R.shape[0], 1, 1)
    return torch.cat([torch.cat([R, t], dim=2), bot], dim=1)


def _loss(T12, T21, T_gt):
    eye = torch.eye(4, device=T_gt.device).expand_as(T_gt)
    return F.mse_loss(T12 @ torch.inverse(T_gt), eye) + F.mse_loss(T21 @ T_gt, eye)


def ref_head(l1, l2, p1, p2, T_gt):
    g1, g2 = F.softmax(l1, dim=2), F.softmax(l2, dim=2)
    pi1, mu1, s1 = ref_gmm_params(g1, p1)
    pi2, mu2, s2 = ref_gmm_params(g2, p2)
    return _loss(ref_gmm_register(pi1, mu1, mu2, s2), ref_gmm_register(pi2, mu2, mu1, s1), T_gt)


def our_head(l1, l2, p1, p2, T_gt):
    _, pi1, mu1, s1 = dg._GmmParamsFunction.apply(l1, p1)
    _, pi2, mu2, s2 = dg._GmmParamsFunction.apply(l2, p2)
    return _loss(dg._GmmRegisterFunction.apply(pi1, mu1, mu2, s2), dg._GmmRegisterFunction.apply(pi2, mu2, mu1, s1), T_gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src, tgt, pose = synthetic.make_pairs(B, N, seed=7)
    src, tgt = src.to(dev).contiguous(), tgt.to(dev).contiguous()
    T_gt = torch.eye(4, device=dev).repeat(B, 1, 1)
    lines = [f"DeepGMR training step, B = {B}, N = {N}, k = {K}, J = {J}; build {_lib.build_id()}; {torch.cuda.get_device_name(0)}; "
             f"median [min, max] of {a.reps} runs, ms"]

    net = dg.Model(Namespace(use_rri=True, rri_size=K, num_groups=J, use_tnet=False), trainable=True).to(dev).train()
    ref = RefPointNet().to(dev).train()
    with torch.no_grad():
        f1 = net.features(src).transpose(1, 2).contiguous()      # [B, 4k, N] for the reference's layout
        f2 = net.features(tgt).transpose(1, 2).contiguous()

    def ours():
        net.zero_grad(set_to_none=True)
        net(src, tgt, T_gt)[0].backward()

    def ours_no_features():
        net.zero_grad(set_to_none=True)
        l1 = net.backbone.forward_train(f1.transpose(1, 2))
        l2 = net.backbone.forward_train(f2.transpose(1, 2))
        our_head(l1, l2, src, tgt, T_gt).backward()

    def theirs():
        ref.zero_grad(set_to_none=True)
        ref_head(ref(f1), ref(f2), src, tgt, T_gt).backward()

    for name, fn in (("step, this project (k-NN + RRI features included)", ours), ("step, this project (features given)", ours_no_features),
                     ("step, torch composition (features given)", theirs)):
        med, lo, hi = _time(fn, a.reps)
        lines.append(f"{name:55s} | {med:8.2f} [{lo:.2f}, {hi:.2f}] | peak {_peak(fn):8.1f} MiB")

    # one BatchNorm layer node at the model's widths
    for cin, cout in ((80, 64), (64, 128), (128, 256), (256, 1024), (512, 256)):
        x = torch.randn(B * N, cin, device=dev, requires_grad=True)
        xr = x.detach().view(B, N, cin).transpose(1, 2).contiguous().requires_grad_(True)
        layer = dg.Conv1DBNReLU(cin, cout).to(dev)
        block = RefBlock(cin, cout).to(dev).train()
        gy = torch.randn(B * N, cout, device=dev)
        gyr = gy.view(B, N, cout).transpose(1, 2).contiguous()

        def node():
            x.grad = None
            layer.zero_grad(set_to_none=True)
            layer.forward_train(x).backward(gy)

        def torch_node():
            xr.grad = None
            block.zero_grad(set_to_none=True)
            block(xr).backward(gyr)
        m1, lo1, hi1 = _time(node, a.reps)
        m2, lo2, hi2 = _time(torch_node, a.reps)
        lines.append(f"layer {cin:4d} -> {cout:4d} fwd + bwd: node {m1:7.3f} [{lo1:.3f}, {hi1:.3f}] peak {_peak(node):7.1f} MiB | "
                     f"torch {m2:7.3f} [{lo2:.3f}, {hi2:.3f}] peak {_peak(torch_node):7.1f} MiB | {m2 / m1:.2f}x")
        del x, xr, layer, block, gy, gyr

    l1 = torch.randn(B, N, J, device=dev, requires_grad=True)
    l2 = torch.randn(B, N, J, device=dev, requires_grad=True)

    def head():
        l1.grad = l2.grad = None
        our_head(l1, l2, src, tgt, T_gt).backward()

    def torch_head():
        l1.grad = l2.grad = None
        ref_head(l1, l2, src, tgt, T_gt).backward()
    m1, lo1, hi1 = _time(head, a.reps)
    m2, lo2, hi2 = _time(torch_head, a.reps)
    lines.append(f"head fwd + bwd: nodes {m1:7.3f} [{lo1:.3f}, {hi1:.3f}] peak {_peak(head):7.1f} MiB | "
                 f"torch {m2:7.3f} [{lo2:.3f}, {hi2:.3f}] peak {_peak(torch_head):7.1f} MiB | {m2 / m1:.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
