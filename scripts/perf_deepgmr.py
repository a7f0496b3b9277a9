"""Time per call of the DeepGMR head's pieces at B = 32 clouds x N = 2048 points, k = 20 neighbours, J = 16 Gaussians:

  1. get_rri_cluster (houv_knn_cross + houv_rri_features) against a torch restatement of the reference's formula that stays on
     the device (the [B*N,k,k,3] cross products broadcast in chunks of clouds) -- the kindest baseline: the reference's own path
     copies the tangent vectors to the host and does this in NumPy;
  2. gmm_params + gmm_register against their torch composition with torch.linalg.svd on the device (the reference: svd on the CPU);
  3. the whole Model forward (prefix "test", seeded random weights), in pairs per second.

HIP events after a warm-up call; the median of the repeats.

    python scripts/perf_deepgmr.py [--reps 5] [--out profiles/r07_perf_deepgmr.txt]"""
import argparse
import math
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from houv_amd import _lib, model_utils, ops, synthetic  # noqa: E402
from houv_amd.mm3d_pn2 import knn_cross  # noqa: E402
from houv_amd.models.deepgmr import Model  # noqa: E402

B, N, K, J = 32, 2048, 20, 16


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


def torch_rri(pts, idx, chunk=4):
    """deepgmr.py:69-94 on the device: pts[B,N,3], idx[B,N,k] int64 -> [B,N,4k]."""
    outs = []
    for s in range(0, pts.shape[0], chunk):
        x, i = pts[s:s + chunk], idx[s:s + chunk]
        b, n, k = i.shape
        q = torch.gather(x.unsqueeze(1).expand(b, n, n, 3), 2, i.unsqueeze(-1).expand(b, n, k, 3))
        p = x.unsqueeze(2).expand(b, n, k, 3)
        rp, rq = p.norm(dim=-1, keepdim=True), q.norm(dim=-1, keepdim=True)
        pn, qn = p / rp, q / rq
        dot = (pn * qn).sum(-1, keepdim=True)
        theta = torch.acos(dot.clamp(-1, 1))
        Tq = q - dot * p
        sin_psi = (torch.linalg.cross(Tq[:, :, None].expand(b, n, k, k, 3), Tq[:, :, :, None].expand(b, n, k, k, 3), dim=-1)
                   * pn[:, :, None]).sum(-1)
        cos_psi = (Tq[:, :, None] * Tq[:, :, :, None]).sum(-1)
        psi = torch.remainder(torch.atan2(sin_psi, cos_psi), 2 * math.pi)
        phi = psi.kthvalue(2, dim=-1).values.unsqueeze(-1)
        outs.append(torch.cat([rp, rq, theta, phi], -1).view(b, n, 4 * k))
    return torch.cat(outs)


def torch_gmm(gamma, pts):
    pi = gamma.mean(1)
    npi = pi * gamma.shape[1]
    mu = gamma.transpose(1, 2) @ pts / npi.unsqueeze(2)
    d = pts.unsqueeze(2) - mu.unsqueeze(1)
    return pi, mu, ((d * d).sum(-1) * gamma).sum(1) / npi


def torch_register(pi_s, mu_s, mu_t, sigma_t):
    cs, ct = pi_s.unsqueeze(1) @ mu_s, pi_s.unsqueeze(1) @ mu_t
    Ms = ((pi_s.unsqueeze(2) * (mu_s - cs)).unsqueeze(3) @ ((mu_t - ct) / sigma_t.unsqueeze(2)).unsqueeze(2)).sum(1)
    U, _, Vh = torch.linalg.svd(Ms)
    V = Vh.transpose(1, 2)
    S = torch.eye(3, device=Ms.device).repeat(len(Ms), 1, 1)
    S[:, 2, 2] = torch.det(V @ U.transpose(1, 2))
    R = V @ S @ U.transpose(1, 2)
    t = ct.transpose(1, 2) - R @ cs.transpose(1, 2)
    bot = torch.tensor([[[0., 0., 0., 1.]]], device=Ms.device).repeat(len(Ms), 1, 1)
    return torch.cat([torch.cat([R, t], 2), bot], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_deepgmr.py needs an MI355X")
    dev = torch.device("cuda:0")
    src, tgt, _ = synthetic.make_pairs(B, N, seed=7)
    src, tgt = src.to(dev), tgt.to(dev)
    lines = [f"# scripts/perf_deepgmr.py  library build {_lib.build_id()}  {torch.cuda.get_device_name(0)}  reps={args.reps}  "
             f"B={B} N={N} k={K} J={J}", "# what | ms per call (median [min, max])"]

    def row(label, fn):
        med, lo, hi = _time(fn, args.reps)
        lines.append(f"{label} | {med:.3f} [{lo:.3f}, {hi:.3f}]")
        print(lines[-1], flush=True)
        return med

    idx = knn_cross(K + 1, src, src)[1]
    idx64 = idx[..., 1:].long().contiguous()
    a = row("get_rri_cluster: houv_knn_cross (k+1 = 21)", lambda: knn_cross(K + 1, src, src))
    b = row("get_rri_cluster: houv_rri_features", lambda: ops.rri_features(src, idx, K, skip=1))
    c = row("get_rri_cluster: both (model_utils.rri_rows)", lambda: model_utils.rri_rows(src, K))
    d = row("torch on the device, features from given lists (chunks of 4 clouds)", lambda: torch_rri(src, idx64))
    lines.append(f"# features alone: torch / HIP = {d / b:.1f}x; with the k-NN on the HIP side only: {d / c:.1f}x")
    mine, ref = ops.rri_features(src, idx, K, skip=1), torch_rri(src, idx64)
    lines.append(f"# max |HIP - torch| over rp, rq, theta: {float((mine - ref).view(B, N, K, 4)[..., :3].abs().max()):.3g}")

    gamma = torch.softmax(torch.randn(B, N, J, generator=torch.Generator().manual_seed(3)).to(dev) * 1.5, dim=-1)
    pi, mu, sg = ops.gmm_params(gamma, src)
    _, mu_t, sg_t = ops.gmm_params(gamma, tgt)
    e = row("houv_gmm_params", lambda: ops.gmm_params(gamma, src))
    f = row("houv_gmm_register", lambda: ops.gmm_register(pi, mu, mu_t, sg_t))
    g = row("torch gmm_params", lambda: torch_gmm(gamma, src))
    h = row("torch gmm_register (torch.linalg.svd on the device)", lambda: torch_register(pi, mu, mu_t, sg_t))
    lines.append(f"# gmm_params: torch / HIP = {g / e:.2f}x; gmm_register: torch / HIP = {h / f:.1f}x; both: {(g + h) / (e + f):.1f}x")
    lines.append(f"# max |T_HIP - T_torch|: {float((ops.gmm_register(pi, mu, mu_t, sg_t) - torch_register(pi, mu, mu_t, sg_t)).abs().max()):.3g}")

    torch.manual_seed(11)
    net = Model(Namespace(use_rri=True, rri_size=K, num_groups=J, use_tnet=False)).to(dev)
    m = row(f"Model forward, prefix test, {B} pairs", lambda: net(src, tgt, prefix="test"))
    lines.append(f"# whole model: {B / m * 1e3:.0f} pairs/s")
    print("\n".join(l for l in lines if l.startswith("# ")), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
