#!/usr/bin/env python3
"""The edge-preserve pooling of SA_SKN_Res_encoder(trainable=True) at the three pooling levels of the shipped VRCNet config
(B = 24, pk = 10; C / N / S = 64 / 3072 / 1536, 128 / 1536 / 768, 256 / 768 / 384): the forward that keeps its graph, the backward
of L = <G, out>, and the peak memory of forward + backward, two ways -- the fused node (_EdgePoolFunction: houv_edge_pool forward,
houv_edge_pool_backward backward) and the torch composition ECG trains with, cat(_RowGather(feat, p_idx), _RowGather(feat,
pn_idx).max(dim=2).values), on the same device in the same run.  Then one training-mode forward + backward of the whole encoder at
B = 24 (layers 1,1,1,1, one list of 16, pk = 10: the shipped cfg), against the same encoder with only the pooling swapped for that
composition.  The baseline of every row is the torch composition, never an earlier build of these kernels.  Median of RUNS timed
runs after WARM warm-up runs, device events, one device; peak memory is torch's allocator peak over one forward + backward, above
what is allocated before it.

    python scripts/perf_vrcnet_encoder_train.py [--out profiles/perf_vrcnet_encoder_train.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from perf_vrcnet import RUNS, WARM  # noqa: E402
from perf_vrcnet_train import measure  # noqa: E402
from houv_amd import _lib  # noqa: E402
from houv_amd.mm3d_pn2 import furthest_point_sample, knn_cross  # noqa: E402
from houv_amd.model_utils_completion import _RowGather, _take_rows  # noqa: E402
from houv_amd.models import vrcnet  # noqa: E402

POOL_LEVELS = ((64, 3072, 1536), (128, 1536, 768), (256, 768, 384))
PK = 10


def composed_pool(feat, p_idx, pn_idx):
    return torch.cat((_RowGather.apply(feat, p_idx), _RowGather.apply(feat, pn_idx).max(dim=2).values), dim=2)


class ComposedPoolEncoder(vrcnet.SA_SKN_Res_encoder):
    """The trainable encoder with its pooling node swapped for the torch composition; everything else is shared."""

    def _pool(self, level, feat, pts, trace, train=False):
        if not train:
            return super()._pool(level, feat, pts, trace)
        with torch.no_grad():
            p_idx = furthest_point_sample(pts, self.pts_num[level])
            centres = _take_rows(pts, p_idx).contiguous()
            pn_idx = knn_cross(int(min(self.pk, pts.shape[1])), centres, pts)[1]
        return composed_pool(feat, p_idx, pn_idx), centres


def row(name, a, b):
    slower = [n for n, x, y in (("forward", a[0], b[0]), ("backward", a[1], b[1])) if x > y]
    note = f"   <- the fused {' and '.join(slower)} is SLOWER here" if slower else ""
    return (f"{name}: forward {a[0]:8.3f} / {b[0]:8.3f} ms ({b[0] / a[0]:4.2f}x)   backward {a[1]:8.3f} / {b[1]:8.3f} ms "
            f"({b[1] / a[1]:4.2f}x)   peak {a[2]:7.1f} / {b[2]:7.1f} MiB ({b[2] / a[2]:4.1f}x)   this / torch{note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=24)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator().manual_seed(29)
    lines = [f"build {_lib.build_id()}  B={B} pk={PK}  median of {RUNS} after {WARM} warm-up runs, device events; "
             "this = _EdgePoolFunction, torch = cat(_RowGather, _RowGather.max) with autograd"]
    for C, N, S in POOL_LEVELS:
        feat = torch.randn(B, N, C, generator=g).relu_().to(dev).requires_grad_(True)     # rectified, as the encoder's are
        pts = torch.rand(B, N, 3, generator=g).to(dev)
        p_idx = furthest_point_sample(pts, S)
        pn_idx = knn_cross(PK, _take_rows(pts, p_idx).contiguous(), pts)[1]
        G = torch.randn(B, S, 2 * C, generator=g).to(dev)
        a = measure(lambda: vrcnet._EdgePoolFunction.apply(feat, p_idx, pn_idx), [feat], G)
        b = measure(lambda: composed_pool(feat, p_idx, pn_idx), [feat], G)
        vrcnet._EdgePoolFunction.apply(feat, p_idx, pn_idx).mul(G).sum().backward()
        mine, feat.grad = feat.grad.clone(), None
        composed_pool(feat, p_idx, pn_idx).mul(G).sum().backward()
        rel, feat.grad = float((mine - feat.grad).norm() / feat.grad.norm()), None
        lines.append(row(f"pool C={C:3d} N={N:4d} S={S:4d}", a, b))
        lines.append(f"    one gathered [B,S,pk,C] tensor is {B * S * PK * C * 4 / 2 ** 20:.1f} MiB; relative L2 difference of the feature "
                     f"gradient between the two {rel:.1e}")
    torch.manual_seed(29)
    kw = dict(input_size=4, k=[16], pk=PK, output_size=256, layers=(1, 1, 1, 1), trainable=True)
    net = vrcnet.SA_SKN_Res_encoder(**kw).to(dev).train()
    base = ComposedPoolEncoder(**kw).to(dev).train()
    base.load_state_dict(net.state_dict(), strict=True)
    x = torch.cat((torch.rand(B, 3072, 3, generator=g) - 0.5, torch.ones(B, 3072, 1)), dim=2).to(dev)
    G = torch.randn(B, 3072, 256, generator=g).to(dev)
    a = measure(lambda: net.forward_rows(x), list(net.parameters()), G)
    b = measure(lambda: base.forward_rows(x), list(base.parameters()), G)
    lines.append(row("SA_SKN_Res_encoder train() forward + backward, N=3072", a, b))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
