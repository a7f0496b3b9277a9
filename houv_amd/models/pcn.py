"""Mirror of registration/models/pcn.py (`PCN_encoder` :12-29, `PCN_decoder` :86-126, `Model` :129-182; completion/models/pcn.py
is the same code): the PCN completion network as an INFERENCE pipeline over the gfx950 kernels of include/houv_hip.h --
houv_mlp2_max for the two PointNet blocks of the encoder (the max-pool is the second GEMM's epilogue; the [B, 512, N] and
[B, 1024, N] activations are never built), houv_gemm_f32 with the bias / ReLU epilogue for the three linear layers and the two
per-cloud projections, and houv_pcn_fold for the folding stage (the [B, 1029, num_fine] feature is never built).  Nothing goes
through the host.

Two algebraic splits replace the reference's `repeat` + `cat`: conv3 of the encoder sees cat(y, g1) with g1 constant over the
points, so conv3.weight[:, 256:] g1 + bias is one 512-vector per cloud (the `shift1` of the second block); conv1 of the decoder
sees cat(grid, point, global), so conv1.weight[:, 5:] feat + bias is one 512-vector per cloud (`cvec`).

The module tree and parameter names equal the reference's, so its checkpoints load with ``load_state_dict(strict=True)`` (the
repository ships no trained weights: tests use seeded ones).  Training is NOT built: the "train" prefix returns the reference's
tuple computed forward-only, without a graph.  `PCN_Transformer` and `PCN_encoder_label` are not built."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..model_utils_completion import calc_cd, calc_emd, gen_grid_up


class _Conv1x1(nn.Module):
    """Parameter holder with nn.Conv1d's names, shapes and default initialisation for a kernel of width 1."""

    def __init__(self, n_in, n_out):
        super().__init__()
        bound = 1 / math.sqrt(n_in)
        self.weight = nn.Parameter(torch.empty(n_out, n_in, 1).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.empty(n_out).uniform_(-bound, bound))

    def matrix(self):
        return self.weight.view(self.weight.shape[0], self.weight.shape[1])

    def columns(self, lo, hi):
        """A dense copy of matrix()[:, lo:hi], made once and remade only when the weight has been written to or moved (the
        kernels take densely packed weights)."""
        stamp = (self.weight.data_ptr(), self.weight._version)
        cache = self.__dict__.setdefault("_columns", {})
        if cache.get((lo, hi), (None, None))[0] != stamp:
            cache[(lo, hi)] = (stamp, self.matrix()[:, lo:hi].contiguous())
        return cache[(lo, hi)][1]


def _linear(layer, x, relu=False):
    return ops.gemm(x, layer.weight, shift=layer.bias, relu=relu)


class PCN_encoder(nn.Module):
    """pcn.py:12-29 on rows: x[B,N,3] -> global feature [B,1024]."""

    def __init__(self, output_size=1024):
        super().__init__()
        self.conv1 = _Conv1x1(3, 128)
        self.conv2 = _Conv1x1(128, 256)
        self.conv3 = _Conv1x1(512, 512)
        self.conv4 = _Conv1x1(512, output_size)

    @torch.no_grad()
    def forward(self, x):
        g1, y = ops.mlp2_max(x, self.conv1.matrix(), self.conv1.bias, self.conv2.matrix(), self.conv2.bias, want_y=True)
        W3 = self.conv3.matrix()
        shift1 = ops.gemm(g1, W3[:, 256:], shift=self.conv3.bias)               # the pooled half of cat(y, g1): once per cloud
        feat, _ = ops.mlp2_max(y, self.conv3.columns(0, 256), shift1, self.conv4.matrix(), self.conv4.bias)
        return feat


class PCN_decoder(nn.Module):
    """pcn.py:86-126: feat[B,1024] -> (coarse[B,num_coarse,3], fine[B,num_fine,3]), both as rows of points."""

    def __init__(self, num_coarse, num_fine, scale, cat_feature_num):
        super().__init__()
        if scale < 1 or scale & (scale - 1) or num_coarse * scale != num_fine:
            raise ValueError(f"PCN_decoder: scale = num_fine // num_coarse = {scale} must be a power of two with "
                             f"num_coarse * scale == num_fine (got num_coarse={num_coarse}, num_fine={num_fine})")
        self.num_coarse, self.num_fine, self.scale = num_coarse, num_fine, scale
        self.fc1 = nn.Linear(1024, 1024)
        self.fc2 = nn.Linear(1024, 1024)
        self.fc3 = nn.Linear(1024, num_coarse * 3)
        self.grid = gen_grid_up(2 ** int(math.log2(scale)), 0.05).contiguous()   # a plain attribute, as in the reference
        self.conv1 = _Conv1x1(cat_feature_num, 512)
        self.conv2 = _Conv1x1(512, 512)
        self.conv3 = _Conv1x1(512, 3)

    @torch.no_grad()
    def forward(self, x):
        B = x.shape[0]
        coarse = _linear(self.fc3, _linear(self.fc2, _linear(self.fc1, x, relu=True), relu=True))
        coarse = coarse.view(B, 3, self.num_coarse).transpose(1, 2).contiguous()                 # [B,nc,3]
        W1 = self.conv1.matrix()
        cvec = ops.gemm(x, W1[:, 5:], shift=self.conv1.bias)                    # the global feature's share of conv1, per cloud
        if self.grid.device != x.device:
            self.grid = self.grid.to(x.device)
        fine = ops.pcn_fold(coarse, cvec, self.grid, self.conv1.columns(0, 5), self.conv2.matrix(), self.conv2.bias,
                            self.conv3.matrix(), self.conv3.bias)
        return coarse, fine


class Model(nn.Module):
    """``Model(args, num_coarse=1024).forward(x[B,3,N], gt=None, prefix="train", mean_feature=None, alpha=None)`` (pcn.py:129-182).
    ``args``: num_points, loss ('cd' | 'emd'), eval_emd (cfgs/pcn_mi355x.yaml).  "test": {'result': out2}; "val": out1, out2, cd_p,
    cd_t, f1 (the reference computes an `emd` there when eval_emd is set and throws it away: not computed); "train": (out2, loss2,
    total_train_loss), forward only.  out1 [B,num_coarse,3], out2 [B,num_points,3]."""

    def __init__(self, args, num_coarse=1024):
        super().__init__()
        self.num_coarse = num_coarse
        self.num_points = args.num_points
        self.train_loss = args.loss
        self.eval_emd = args.eval_emd
        self.scale = self.num_points // num_coarse
        self.cat_feature_num = 2 + 3 + 1024
        self.encoder = PCN_encoder()
        self.decoder = PCN_decoder(num_coarse, self.num_points, self.scale, self.cat_feature_num)

    @torch.no_grad()
    def forward(self, x, gt=None, prefix="train", mean_feature=None, alpha=None):
        feat = self.encoder(x.transpose(1, 2).contiguous().float())
        out1, out2 = self.decoder(feat)
        if prefix == "train":
            if self.train_loss == 'emd':
                loss1 = calc_emd(out1, gt)
                loss2 = calc_emd(out2, gt)
            elif self.train_loss == 'cd':
                loss1, _ = calc_cd(out1, gt)
                loss2, _ = calc_cd(out2, gt)
            else:
                raise NotImplementedError('Train loss is either CD or EMD!')
            total_train_loss = loss1.mean() + loss2.mean() * alpha
            return out2, loss2, total_train_loss
        elif prefix == "val":
            cd_p, cd_t, f1 = calc_cd(out2, gt, calc_f1=True)
            return {'out1': out1, 'out2': out2, 'cd_p': cd_p, 'cd_t': cd_t, 'f1': f1}
        return {'result': out2}
