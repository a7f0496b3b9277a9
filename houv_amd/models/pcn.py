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
repository ships no trained weights: tests use seeded ones).  Training is opt-in: ``Model(args, num_coarse,
trainable=True)`` runs the encoder (houv_mlp2_max_arg + houv_mlp2_max_backward on the critical points of each cloud), the three
linear layers and the folding stage (houv_pcn_fold_backward, which recomputes what the forward did not keep) through
``torch.autograd.Function``s, and its "train" prefix returns the reference's tuple with a graph.  With the
default ``trainable=False`` the tuple is computed forward-only, without a graph.  `PCN_Transformer` and `PCN_encoder_label` are not built."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..model_utils_completion import _LinearFunction, _transposed, calc_cd, calc_emd, gen_grid_up


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


class _EncoderFunction(torch.autograd.Function):
    """The whole encoder as one differentiable node.  Forward: the two PointNet blocks through
    houv_mlp2_max_arg, bit for bit the inference path's feature.  Backward: both maxima send their gradient to one row per
    channel, so block 2 runs on its <= 1024 critical rows per cloud and hands block 1 the gradient of y on exactly those rows
    (a row list, never a dense [B,N,256] tensor); block 1 adds its own <= 256.  The pooled half of cat(y, g1) was split off
    into shift1 = W3[:, 256:] g1 + b3, so its three gradients are small products of gshift1[B,512]."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, W3, b3, W4, b4, W3y):
        g1, arg1, y = ops.mlp2_max_arg(x, W1, b1, W2, b2, want_y=True)
        shift1 = ops.gemm(g1, W3[:, 256:], shift=b3)
        feat, arg2, _ = ops.mlp2_max_arg(y, W3y, shift1, W4, b4)
        ctx.save_for_backward(x, W1, b1, W2, W3, W4, W3y, y, g1, shift1, arg1, arg2)
        return feat

    @staticmethod
    def backward(ctx, gfeat):
        x, W1, b1, W2, W3, W4, W3y, y, g1, shift1, arg1, arg2 = ctx.saved_tensors
        r2 = ops.mlp2_max_backward(y, W3y, shift1, W4, arg2, gfeat.contiguous(), want_gx=True)
        gs = r2["gshift1"]                                                       # [B,512]: one row per cloud
        gW3 = torch.empty_like(W3)
        gW3[:, :256] = r2["gW1"]
        ops.gemm(_transposed(gs), _transposed(g1), gW3[:, 256:])         # gshift1^T g1
        gg1 = ops.gemm(gs, W3[:, 256:], trans_b=False)                           # what shift1 sends back to the first pool
        r1 = ops.mlp2_max_backward(x, W1, b1, W2, arg1, gg1, rows=r2["act_rows"], nrows=r2["nact"], gy_rows=r2["gx_rows"])
        return None, r1["gW1"], r1["gshift1"].sum(0), r1["gW2"], r1["gb2"], gW3, gs.sum(0), r2["gW2"], r2["gb2"], None


class PCN_encoder(nn.Module):
    """pcn.py:12-29 on rows: x[B,N,3] -> global feature [B,1024].  ``trainable=True`` makes the feature differentiable with
    respect to the eight parameters when grad mode is on (the same bits; not with respect to x, which is refused)."""

    def __init__(self, output_size=1024, trainable=False):
        super().__init__()
        self.trainable = trainable
        self.conv1 = _Conv1x1(3, 128)
        self.conv2 = _Conv1x1(128, 256)
        self.conv3 = _Conv1x1(512, 512)
        self.conv4 = _Conv1x1(512, output_size)

    def forward(self, x):
        if self.trainable and torch.is_grad_enabled():
            if x.requires_grad:
                raise ValueError("PCN_encoder: the gradient with respect to the input cloud is not built (x.requires_grad)")
            with torch.no_grad():
                W3y = self.conv3.columns(0, 256)                                 # a packed copy: its gradient returns through W3
            return _EncoderFunction.apply(x, self.conv1.matrix(), self.conv1.bias, self.conv2.matrix(), self.conv2.bias,
                                          self.conv3.matrix(), self.conv3.bias, self.conv4.matrix(), self.conv4.bias, W3y)
        with torch.no_grad():
            return self._forward(x)

    def _forward(self, x):
        g1, y = ops.mlp2_max(x, self.conv1.matrix(), self.conv1.bias, self.conv2.matrix(), self.conv2.bias, want_y=True)
        W3 = self.conv3.matrix()
        shift1 = ops.gemm(g1, W3[:, 256:], shift=self.conv3.bias)               # the pooled half of cat(y, g1): once per cloud
        feat, _ = ops.mlp2_max(y, self.conv3.columns(0, 256), shift1, self.conv4.matrix(), self.conv4.bias)
        return feat


class _FoldFunction(torch.autograd.Function):
    """The folding stage with the `cvec` split as one differentiable node: houv_pcn_fold forward (nothing kept but its inputs),
    houv_pcn_fold_backward backward.  conv1.weight = [Wgp | Wf]: gWgp comes from the kernel, gWf = gcvec^T feat,
    g(conv1.bias) = sum_b gcvec, and gcvec Wf joins the gradient of the global feature."""

    @staticmethod
    def forward(ctx, coarse, feat, grid, W1, b1, Wgp, W2, b2, W3, b3):
        cvec = ops.gemm(feat, W1[:, 5:], shift=b1)
        ctx.save_for_backward(coarse, feat, grid, W1, Wgp, W2, b2, W3, b3, cvec)
        return ops.pcn_fold(coarse, cvec, grid, Wgp, W2, b2, W3, b3)

    @staticmethod
    def backward(ctx, gfine):
        coarse, feat, grid, W1, Wgp, W2, b2, W3, b3, cvec = ctx.saved_tensors
        r = ops.pcn_fold_backward(coarse, cvec, grid, Wgp, W2, b2, W3, b3, gfine.contiguous())
        gW1 = torch.empty_like(W1)
        gW1[:, :5] = r["gWgp"]
        ops.gemm(_transposed(r["gcvec"]), _transposed(feat), gW1[:, 5:])
        gfeat = ops.gemm(r["gcvec"], W1[:, 5:], trans_b=False)
        return r["gcoarse"], gfeat, None, gW1, r["gcvec"].sum(0), None, r["gW2"], r["gb2"], r["gW3"], r["gb3"]


class PCN_decoder(nn.Module):
    """pcn.py:86-126: feat[B,1024] -> (coarse[B,num_coarse,3], fine[B,num_fine,3]), both as rows of points.  ``trainable=True``:
    differentiable with respect to feat and the twelve parameters when grad mode is on (the same bits)."""

    def __init__(self, num_coarse, num_fine, scale, cat_feature_num, trainable=False):
        super().__init__()
        self.trainable = trainable
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

    def forward(self, x):
        if self.grid.device != x.device:
            self.grid = self.grid.to(x.device)
        if self.trainable and torch.is_grad_enabled():
            lin = lambda layer, t, relu: _LinearFunction.apply(t, layer.weight, layer.bias, relu)
            coarse = lin(self.fc3, lin(self.fc2, lin(self.fc1, x, True), True), False)
            coarse = coarse.view(x.shape[0], 3, self.num_coarse).transpose(1, 2).contiguous()
            with torch.no_grad():
                Wgp = self.conv1.columns(0, 5)                                   # a packed copy: its gradient returns through W1
            fine = _FoldFunction.apply(coarse, x, self.grid, self.conv1.matrix(), self.conv1.bias, Wgp, self.conv2.matrix(),
                                       self.conv2.bias, self.conv3.matrix(), self.conv3.bias)
            return coarse, fine
        with torch.no_grad():
            return self._forward(x)

    def _forward(self, x):
        B = x.shape[0]
        coarse = _linear(self.fc3, _linear(self.fc2, _linear(self.fc1, x, relu=True), relu=True))
        coarse = coarse.view(B, 3, self.num_coarse).transpose(1, 2).contiguous()                 # [B,nc,3]
        W1 = self.conv1.matrix()
        cvec = ops.gemm(x, W1[:, 5:], shift=self.conv1.bias)                    # the global feature's share of conv1, per cloud
        fine = ops.pcn_fold(coarse, cvec, self.grid, self.conv1.columns(0, 5), self.conv2.matrix(), self.conv2.bias,
                            self.conv3.matrix(), self.conv3.bias)
        return coarse, fine


class Model(nn.Module):
    """``Model(args, num_coarse=1024).forward(x[B,3,N], gt=None, prefix="train", mean_feature=None, alpha=None)`` (pcn.py:129-182).
    ``args``: num_points, loss ('cd' | 'emd'), eval_emd (cfgs/pcn_mi355x.yaml).  "test": {'result': out2}; "val": out1, out2, cd_p,
    cd_t, f1 (the reference computes an `emd` there when eval_emd is set and throws it away: not computed); "train": (out2, loss2,
    total_train_loss).  out1 [B,num_coarse,3], out2 [B,num_points,3].

    ``trainable=False`` (the default): everything is computed without a graph, "train" included.  ``trainable=True`` with grad
    mode on: the same outputs and losses bit for bit, with a graph through the encoder, decoder and loss, so that
    ``total_train_loss.backward()`` fills ``.grad`` of all 20 parameters and ``torch.optim.Adam(net.parameters())`` trains as
    completion/train.py does.  The gradient with respect to the input cloud is not built: an x with requires_grad is refused."""

    def __init__(self, args, num_coarse=1024, trainable=False):
        super().__init__()
        self.trainable = trainable
        self.num_coarse = num_coarse
        self.num_points = args.num_points
        self.train_loss = args.loss
        self.eval_emd = args.eval_emd
        self.scale = self.num_points // num_coarse
        self.cat_feature_num = 2 + 3 + 1024
        self.encoder = PCN_encoder(trainable=trainable)
        self.decoder = PCN_decoder(num_coarse, self.num_points, self.scale, self.cat_feature_num, trainable=trainable)

    def forward(self, x, gt=None, prefix="train", mean_feature=None, alpha=None):
        if self.trainable and torch.is_grad_enabled():
            if x.requires_grad:
                raise ValueError("models.pcn.Model: the gradient with respect to the input cloud is not built (x.requires_grad)")
            return self._forward(x, gt, prefix, alpha)
        with torch.no_grad():
            return self._forward(x, gt, prefix, alpha)

    def _forward(self, x, gt, prefix, alpha):
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
