"""Mirror of completion/models/ecg.py (`Stack_conv` :21-33, `Dense_conv` :36-65, `EF_encoder` :68-159, `ECG_decoder` :162-210,
`Model` :213-254): the ECG completion network as an INFERENCE pipeline over the gfx950 kernels of include/houv_hip.h --
houv_mlp2_max for the PCN encoder it shares with models/pcn.py, houv_knn_feat + houv_dense_conv for the four Dense_conv blocks
(the [B, N, N] distance matrix and the [B, 2C .. C+72, N, 16] edge activations are never built), houv_gemm_f32 with the bias / ReLU
epilogue for every 1x1 convolution and linear layer, and the point ops (FPS, houv_knn_cross) for the hierarchy.  Nothing goes
through the host.  DESIGN.md section 9.10.

Activations are rows [B, N, C].  The reference's torch.cat of [B, C, N] tensors are column slices of one row-major buffer per
level: a Dense_conv writes its C + 72 columns straight into it (the `ldo` of houv_dense_conv), the convolution after it reads
the slice it needs (the `lda` of houv_gemm_f32).  conv5 sees cat(global, x4) with the global feature constant over the points,
so conv5.weight[:, :1024] g + bias is one 1024-vector per cloud (the `shift1` split of PCN).

The module tree and parameter names equal the reference's, so its checkpoints load with ``load_state_dict(strict=True)`` (the
repository ships no trained weights: tests use seeded ones).  Training is opt-in: ``Model(args, ...,
trainable=True)`` with grad mode on returns the "train" tuple with a graph whose outputs carry the inference path's bits.  Each
Dense_conv is ONE autograd node (houv_dense_conv_arg forward, houv_dense_conv_backward backward: it keeps x, idx, arg, out and
the weights, never an edge tensor); linear layers go through _LinearRowsFunction, row gathers through the ordered scatter of
houv_scatter_points_grad, every pool through torch.max (one winner), and the reference's concatenations are torch.cat of
[B, N, <= 1800] rows.  The k-NN lists, the samples and the three-NN weights are constants, as in the reference.  With the
default ``trainable=False`` nothing changes: the tuple is computed forward-only, without a graph.  EF_expansion (scale >= 2) is
not wired into this decoder's graph: ``trainable=True`` refuses it at construction (the block's backward now exists --
EF_expansion(trainable=True), DESIGN.md section 9.16, which VRCNet's decoder uses -- and ECG can adopt it).

Discrete decisions.  The network takes ~4000 arg-min / arg-sort decisions per cloud (furthest-point samples, k-NN lists in
coordinate and in feature space, three-NN lists), and the reference does not agree with itself on them across precisions
(DESIGN.md section 9.10).  ``Model(..., trace={})`` records every one of them -- fps1..3, knn_pt1..3, knn_feat1..4 (with the
feature rows each was computed from, knn_feat1_x ..), three_nn1..3, knn_exp (+ knn_exp_x), fps_out -- so that parity can be
stated GIVEN the decisions, and the decisions checked on their own.  With trace=None nothing is recorded or copied."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..mm3d_pn2 import furthest_point_sample, knn_cross, three_interpolate
from ..model_utils_completion import (Conv1x1, EF_expansion, _LinearRowsFunction, _RowGather, _take_rows, _transposed_batch, calc_cd,
                                      calc_emd, get_uniform_loss, knn, three_nn_upsampling)
from .pcn import PCN_encoder

_G = ops.DENSE_CONV_GROWTH


def _linear(layer, x, relu=False):
    return ops.gemm(x, layer.weight, shift=layer.bias, relu=relu)


def _lin(x, W, b, relu=False):
    """The differentiable linear layer on rows (..., K) -> (..., N)."""
    x2 = x.reshape(-1, x.shape[-1])
    return _LinearRowsFunction.apply(x2, W, b, relu).view(*x.shape[:-1], W.shape[0])


def _conv(conv, x, relu=False):
    return _lin(x, conv.matrix(), conv.bias, relu)


class _DenseConvFunction(torch.autograd.Function):
    """Dense_conv as one differentiable node: houv_dense_conv_arg forward (houv_dense_conv's bits),
    houv_dense_conv_backward backward.  Saved: x, idx, arg, out and the weights.  idx is not differentiable."""

    @staticmethod
    def forward(ctx, x, idx, W0, b0, W1, b1, W2, b2, relu_out):
        out, arg = ops.dense_conv_arg(x, idx, W0, b0, W1, b1, W2, b2, relu_out=relu_out)
        ctx.relu_out = relu_out
        ctx.save_for_backward(x, idx, arg, out, W0, b0, W1, b1, W2, b2)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, gout, _garg):
        x, idx, arg, out, W0, b0, W1, b1, W2, b2 = ctx.saved_tensors
        r = ops.dense_conv_backward(x, idx, W0, b0, W1, b1, W2, b2, arg, gout.contiguous(), out=out, relu_out=ctx.relu_out)
        return r["gx"], None, r["gW0"], r["gb0"], r["gW1"], r["gb1"], r["gW2"], r["gb2"], None


class Stack_conv(nn.Module):
    """ecg.py:21-33: y = cat(x, act(conv(x))).  A parameter holder here: Dense_conv evaluates its two Stack_convs inside
    houv_dense_conv."""

    def __init__(self, input_size, output_size, act=None):
        super().__init__()
        self.model = nn.Sequential()
        self.model.add_module('conv', Conv1x1(input_size, output_size, 2))
        if act is not None:
            self.model.add_module('act', act)


class Dense_conv(nn.Module):
    """ecg.py:36-65 for growth_rate = 24, dense_n = 3 (what ECG builds; houv_dense_conv serves input_size 24 and 48)."""

    def __init__(self, input_size, growth_rate=_G, dense_n=3, k=16, trainable=False):
        super().__init__()
        self.trainable = trainable
        if growth_rate != _G or dense_n != 3:
            raise NotImplementedError(f"Dense_conv: growth_rate={growth_rate}, dense_n={dense_n} has no kernel ({_G} and 3 are served)")
        self.growth_rate, self.dense_n, self.k, self.comp, self.input_size = growth_rate, dense_n, k, growth_rate * 2, input_size
        self.first_conv = Conv1x1(input_size * 2, growth_rate, 2)
        self.model = nn.Sequential()
        self.model.add_module('stack_conv_1', Stack_conv(input_size + growth_rate, growth_rate, nn.ReLU()))
        self.model.add_module('stack_conv_2', Stack_conv(input_size + 2 * growth_rate, growth_rate, None))

    def _weights(self):
        c1, c2 = self.model.stack_conv_1.model.conv, self.model.stack_conv_2.model.conv
        return self.first_conv.matrix(), self.first_conv.bias, c1.matrix(), c1.bias, c2.matrix(), c2.bias

    def train_rows(self, rows, relu_out=False, trace=None, name=None):
        """forward_rows with a graph (grad mode on): rows (B,N,input_size) -> a fresh (B,N,input_size+72) with the same bits."""
        with torch.no_grad():
            idx = ops.knn_feat(rows, min(self.k, rows.shape[1]))
        if trace is not None:
            trace[name], trace[name + "_x"] = idx, rows.detach().clone()
        return _DenseConvFunction.apply(rows, idx, *self._weights(), bool(relu_out))[0]

    @torch.no_grad()
    def forward_rows(self, rows, out=None, relu_out=False, trace=None, name=None):
        """rows (B,N,input_size) -> (B,N,input_size+72); `out` may be a column slice of a wider buffer."""
        idx = ops.knn_feat(rows, min(self.k, rows.shape[1]))
        if trace is not None:
            trace[name], trace[name + "_x"] = idx, rows.clone()
        c1, c2 = self.model.stack_conv_1.model.conv, self.model.stack_conv_2.model.conv
        return ops.dense_conv(rows, idx, self.first_conv.matrix(), self.first_conv.bias, c1.matrix(), c1.bias, c2.matrix(), c2.bias,
                              relu_out=relu_out, out=out)

    def forward(self, x):
        """x (B,input_size,N) -> (B,input_size+72,N), the reference's layout: knn + houv_dense_conv.  With trainable=True and
        grad mode on the result carries a graph to x and the six parameters (the same bits)."""
        if self.trainable and torch.is_grad_enabled():
            rows = x.transpose(1, 2).contiguous().float()
            with torch.no_grad():
                idx = knn(x, min(self.k, x.shape[2])).int()
            return _DenseConvFunction.apply(rows, idx, *self._weights(), False)[0].transpose(1, 2).contiguous()
        with torch.no_grad():
            return self._forward(x)

    def _forward(self, x):
        rows = x.transpose(1, 2).contiguous().float()
        idx = knn(x, min(self.k, x.shape[2])).int()
        c1, c2 = self.model.stack_conv_1.model.conv, self.model.stack_conv_2.model.conv
        out = ops.dense_conv(rows, idx, self.first_conv.matrix(), self.first_conv.bias, c1.matrix(), c1.bias, c2.matrix(), c2.bias)
        return out.transpose(1, 2).contiguous()


class EF_encoder(nn.Module):
    """ecg.py:68-159 on rows: points (B,N,3) -> (B,N,output_size)."""

    def __init__(self, growth_rate=_G, dense_n=3, k=16, hierarchy=(1024, 256, 64), input_size=3, output_size=256, trainable=False):
        super().__init__()
        self.trainable = trainable
        self.growth_rate, self.comp, self.dense_n, self.k, self.hierarchy = growth_rate, growth_rate * 2, dense_n, k, list(hierarchy)
        self.init_channel = 24
        self.conv1 = Conv1x1(input_size, self.init_channel)
        self.dense_conv1 = Dense_conv(self.init_channel, growth_rate, dense_n, k, trainable=trainable)
        c1 = self.init_channel * 2 + growth_rate * dense_n                       # 120
        self.conv2 = Conv1x1(c1 * 2, self.comp)
        self.dense_conv2 = Dense_conv(self.comp, growth_rate, dense_n, k, trainable=trainable)
        c2 = c1 * 2 + self.comp + growth_rate * dense_n                          # 360
        self.conv3 = Conv1x1(c2 * 2, self.comp)
        self.dense_conv3 = Dense_conv(self.comp, growth_rate, dense_n, k, trainable=trainable)
        c3 = c2 * 2 + self.comp + growth_rate * dense_n                          # 840
        self.conv4 = Conv1x1(c3 * 2, self.comp)
        self.dense_conv4 = Dense_conv(self.comp, growth_rate, dense_n, k, trainable=trainable)
        c4 = c3 * 2 + self.comp + growth_rate * dense_n                          # 1800
        self.gf_conv = Conv1x1(c4, 1024)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 1024)
        self.conv5 = Conv1x1(c4 + 1024, 1024)
        self.conv6 = Conv1x1(c3 + 1024, 768)
        self.conv7 = Conv1x1(c2 + 768, 512)
        self.conv8 = Conv1x1(c1 + 512, output_size)
        self.widths = (c1, c2, c3, c4)

    def _sample(self, level, feat, pts, out, trace):
        """edge_preserve_sampling (model_utils.py:90-116) on rows: feat (B,N,C), pts (B,N,3) -> writes cat(centre, neighbour max)
        into out (B,S,2C) and returns the sampled points (B,S,3)."""
        S, C = self.hierarchy[level - 1], feat.shape[2]
        p_idx = furthest_point_sample(pts, S)
        centres = _take_rows(pts, p_idx).contiguous()
        pn_idx = knn_cross(int(min(self.k, pts.shape[1])), centres, pts)[1]
        if trace is not None:
            trace[f"fps{level}"], trace[f"knn_pt{level}"] = p_idx, pn_idx
        out[..., :C] = _take_rows(feat, p_idx)
        out[..., C:] = _take_rows(feat, pn_idx).amax(dim=2)
        return centres

    @staticmethod
    def _upsample(level, feat, target, source, out, trace):
        """three_nn_upsampling + three_interpolate on rows: feat (B,M,C) at `source` -> out (B,N,C) at `target`."""
        idx, weight = three_nn_upsampling(target, source)
        if trace is not None:
            trace[f"three_nn{level}"] = idx
        f = _take_rows(feat, idx)                                                 # (B,N,3,C)
        w = weight.unsqueeze(-1)
        out.copy_((w[:, :, 0] * f[:, :, 0] + w[:, :, 1] * f[:, :, 1]) + w[:, :, 2] * f[:, :, 2])

    def _sample_train(self, level, feat, pts, trace):
        """_sample with a graph: -> (cat(centre, neighbour max) (B,S,2C), the sampled points (B,S,3)).  The gathers have the
        ordered gradient; the pool is torch.max, whose gradient goes to one winner."""
        S = self.hierarchy[level - 1]
        with torch.no_grad():
            p_idx = furthest_point_sample(pts, S)
            centres = _take_rows(pts, p_idx).contiguous()
            pn_idx = knn_cross(int(min(self.k, pts.shape[1])), centres, pts)[1]
        if trace is not None:
            trace[f"fps{level}"], trace[f"knn_pt{level}"] = p_idx, pn_idx
        return torch.cat((_RowGather.apply(feat, p_idx), _RowGather.apply(feat, pn_idx).max(dim=2).values), dim=2), centres

    @staticmethod
    def _upsample_train(level, feat, target, source, trace):
        """_upsample with a graph in feat (the weights are constants, as three_nn is in the reference): -> (B,N,C)."""
        with torch.no_grad():
            idx, weight = three_nn_upsampling(target, source)
        if trace is not None:
            trace[f"three_nn{level}"] = idx
        # houv_three_interpolate evaluates (w0 f0 + w1 f1) + w2 f2 without contraction, the expression _upsample spells out in
        # torch ops, and its gradient is the ordered scatter; the (B,N,3,C) gather is not built
        return _transposed_batch(three_interpolate(_transposed_batch(feat), idx, weight))

    def train_rows(self, pts, trace=None):
        """forward_rows with a graph (grad mode on): the reference's concatenations as torch.cat of rows, the same bits.  pts may
        carry a gradient (the decoder's coarse points): it flows through conv1; the samples, lists and weights made from the
        coordinates are constants."""
        B = pts.shape[0]
        c4 = self.widths[3]
        coords = pts.detach()
        x0 = _conv(self.conv1, pts, relu=True)
        L1 = torch.cat((self.dense_conv1.train_rows(x0, relu_out=True, trace=trace, name="knn_feat1"), x0), dim=2)
        s1, pc2 = self._sample_train(1, L1, coords, trace)
        L2 = torch.cat((self.dense_conv2.train_rows(_conv(self.conv2, s1, relu=True), relu_out=True, trace=trace, name="knn_feat2"), s1), dim=2)
        s2, pc3 = self._sample_train(2, L2, pc2, trace)
        L3 = torch.cat((self.dense_conv3.train_rows(_conv(self.conv3, s2, relu=True), relu_out=True, trace=trace, name="knn_feat3"), s2), dim=2)
        s3, pc4 = self._sample_train(3, L3, pc3, trace)
        L4 = torch.cat((self.dense_conv4.train_rows(_conv(self.conv4, s3, relu=True), relu_out=True, trace=trace, name="knn_feat4"), s3), dim=2)

        g = _conv(self.gf_conv, L4).max(dim=1).values
        g = _lin(_lin(g, self.fc1.weight, self.fc1.bias, True), self.fc2.weight, self.fc2.bias, True)
        W5 = self.conv5.matrix()
        shift = _lin(g, W5[:, :1024], self.conv5.bias)                           # the global feature's share of conv5, per cloud
        x4 = torch.relu(_lin(L4, W5[:, 1024:], None).view(B, -1, 1024) + shift.unsqueeze(1))
        x3 = _conv(self.conv6, torch.cat((L3, self._upsample_train(1, x4, pc3, pc4, trace)), dim=2), relu=True)
        x2 = _conv(self.conv7, torch.cat((L2, self._upsample_train(2, x3, pc2, pc3, trace)), dim=2), relu=True)
        return _conv(self.conv8, torch.cat((L1, self._upsample_train(3, x2, coords, pc2, trace)), dim=2))

    @torch.no_grad()
    def forward_rows(self, pts, trace=None):
        B, N, _ = pts.shape
        c1, c2, c3, c4 = self.widths
        d = self.comp + _G * self.dense_n                                         # 120: width of dense_conv2..4's output
        d1 = self.init_channel + _G * self.dense_n                                # 96: of dense_conv1's
        new = lambda n, c: torch.empty((B, n, c), dtype=torch.float32, device=pts.device)
        # one buffer per level: [dense | the level's input | the coarser level's features, up-sampled (the later conv's operand)]
        X1, X2, X3, X4 = new(N, c1 + 512), new(self.hierarchy[0], c2 + 768), new(self.hierarchy[1], c3 + 1024), new(self.hierarchy[2], c4)

        x0 = X1[..., d1:c1]
        self.conv1.rows(pts, relu=True, out=x0)
        self.dense_conv1.forward_rows(x0, out=X1[..., :d1], relu_out=True, trace=trace, name="knn_feat1")
        pc2 = self._sample(1, X1[..., :c1], pts, X2[..., d:c2], trace)

        t = self.conv2.rows(X2[..., d:c2], relu=True)
        self.dense_conv2.forward_rows(t, out=X2[..., :d], relu_out=True, trace=trace, name="knn_feat2")
        pc3 = self._sample(2, X2[..., :c2], pc2, X3[..., d:c3], trace)

        t = self.conv3.rows(X3[..., d:c3], relu=True)
        self.dense_conv3.forward_rows(t, out=X3[..., :d], relu_out=True, trace=trace, name="knn_feat3")
        pc4 = self._sample(3, X3[..., :c3], pc3, X4[..., d:c4], trace)

        t = self.conv4.rows(X4[..., d:c4], relu=True)
        self.dense_conv4.forward_rows(t, out=X4[..., :d], relu_out=True, trace=trace, name="knn_feat4")

        g = self.gf_conv.rows(X4).amax(dim=1)
        g = _linear(self.fc2, _linear(self.fc1, g, relu=True), relu=True)
        W5 = self.conv5.matrix()
        shift = ops.gemm(g, W5[:, :1024], shift=self.conv5.bias)                  # the global feature's share of conv5, per cloud
        x4 = torch.relu_(ops.gemm(X4.view(-1, c4), W5[:, 1024:]).view(B, -1, 1024) + shift.unsqueeze(1))
        self._upsample(1, x4, pc3, pc4, X3[..., c3:], trace)
        x3 = self.conv6.rows(X3, relu=True)
        self._upsample(2, x3, pc2, pc3, X2[..., c2:], trace)
        x2 = self.conv7.rows(X2, relu=True)
        self._upsample(3, x2, pts, pc2, X1[..., c1:], trace)
        return self.conv8.rows(X1)

    def forward(self, x, trace=None):
        """x (B,3,N) -> (B,output_size,N), the reference's layout; with trainable=True and grad mode on, with a graph."""
        rows = x.transpose(1, 2).contiguous().float()
        if self.trainable and torch.is_grad_enabled():
            return self.train_rows(rows, trace).transpose(1, 2).contiguous()
        return self.forward_rows(rows, trace).transpose(1, 2).contiguous()


class ECG_decoder(nn.Module):
    """ecg.py:162-210: (feat (B,1024), input points (B,num_input,3)) -> (coarse (B,num_coarse,3), fine (B,num_fine,3)), rows."""

    def __init__(self, num_coarse, num_fine, num_input, trainable=False):
        super().__init__()
        self.trainable = trainable
        self.num_coarse, self.num_fine = num_coarse, num_fine
        self.scale = int(np.ceil(num_fine / (num_coarse + num_input)))
        if trainable and self.scale >= 2:
            raise NotImplementedError(f"ECG_decoder: trainable=True with scale = ceil(num_fine / (num_coarse + num_input)) = "
                                      f"{self.scale} >= 2 needs the backward of EF_expansion, which is not built (scale 1 is served)")
        self.fc1 = nn.Linear(1024, 1024)
        self.fc2 = nn.Linear(1024, 1024)
        self.fc3 = nn.Linear(1024, num_coarse * 3)
        self.dense_feature_size, self.expand_feature_size, self.input_size = 256, 64, 3
        self.encoder = EF_encoder(growth_rate=_G, dense_n=3, k=16, hierarchy=[1024, 256, 64], input_size=self.input_size,
                                  output_size=self.dense_feature_size, trainable=trainable)
        if self.scale >= 2:
            self.expansion = EF_expansion(input_size=self.dense_feature_size, output_size=self.expand_feature_size,
                                          step_ratio=self.scale, k=4)
            self.conv1 = Conv1x1(self.expand_feature_size, self.expand_feature_size)
        else:
            self.expansion = None
            self.conv1 = Conv1x1(self.dense_feature_size, self.expand_feature_size)
        self.conv2 = Conv1x1(self.expand_feature_size, 3)

    def forward(self, global_feat, point_input, trace=None):
        if self.trainable and torch.is_grad_enabled():
            return self._forward_train(global_feat, point_input, trace)
        with torch.no_grad():
            return self._forward(global_feat, point_input, trace)

    def _forward_train(self, global_feat, point_input, trace):
        B = global_feat.shape[0]
        h = _lin(_lin(global_feat, self.fc1.weight, self.fc1.bias, True), self.fc2.weight, self.fc2.bias, True)
        coarse = _lin(h, self.fc3.weight, self.fc3.bias).view(B, 3, self.num_coarse).transpose(1, 2).contiguous()   # [B,nc,3]
        dense = self.encoder.train_rows(torch.cat((coarse, point_input), dim=1), trace)
        fine = _conv(self.conv2, _conv(self.conv1, dense, relu=True))
        if fine.shape[1] > self.num_fine:
            with torch.no_grad():
                idx = furthest_point_sample(fine.detach(), self.num_fine)
            if trace is not None:
                trace["fps_out"] = idx
            fine = _RowGather.apply(fine, idx).contiguous()
        return coarse, fine

    def _forward(self, global_feat, point_input, trace=None):
        B = global_feat.shape[0]
        coarse = _linear(self.fc3, _linear(self.fc2, _linear(self.fc1, global_feat, relu=True), relu=True))
        coarse = coarse.view(B, 3, self.num_coarse).transpose(1, 2).contiguous()                 # [B,nc,3]
        points = torch.cat((coarse, point_input), dim=1)
        dense = self.encoder.forward_rows(points, trace)
        if self.scale >= 2:
            dense = self.expansion.forward_rows(dense, trace=trace)
        fine = self.conv2.rows(self.conv1.rows(dense, relu=True))
        if fine.shape[1] > self.num_fine:
            idx = furthest_point_sample(fine, self.num_fine)
            if trace is not None:
                trace["fps_out"] = idx
            fine = _take_rows(fine, idx).contiguous()
        return coarse, fine


class Model(nn.Module):
    """``Model(args, num_coarse=1024, num_input=2048, trace=None).forward(x[B,3,N], gt=None, prefix="train", mean_feature=None,
    alpha=None)`` (ecg.py:213-254).  ``args``: num_points, loss ('cd' | 'emd'), eval_emd (cfgs/ecg_mi355x.yaml).  "test":
    {'result': out2}; "val": out1, out2, emd (0 unless eval_emd), cd_p, cd_t, f1; "train": (out2, loss2, total_train_loss) with the
    two get_uniform_loss terms.  out1 [B,num_coarse,3], out2 [B,num_points,3].

    ``trainable=False`` (the default): everything is computed without a graph, "train" included.  ``trainable=True`` with grad
    mode on: the same outputs bit for bit, with a graph through the PCN encoder, the decoder and the losses, so that
    ``total_train_loss.backward()`` fills ``.grad`` of every parameter.  The gradient with respect to the
    input cloud is not built: an x with requires_grad is refused.  scale >= 2 (EF_expansion) is refused at construction.

    The reference evaluates get_uniform_loss under every prefix and throws it away outside "train"; here it is computed only
    there.  The reference therefore cannot run at all with fewer than 500 coarse or 500 fine points (int(N * 0.004) < 2 leaves its
    2-nearest search without a second point); under "test" and "val" this implementation can.  The hierarchy needs
    num_coarse + num_input >= 1024 points either way."""

    def __init__(self, args, num_coarse=1024, num_input=2048, trace=None, trainable=False):
        super().__init__()
        self.trainable = trainable
        self.num_coarse = num_coarse
        self.num_points = args.num_points
        self.train_loss = args.loss
        self.eval_emd = args.eval_emd
        self.trace = trace
        self.encoder = PCN_encoder(trainable=trainable)
        self.decoder = ECG_decoder(num_coarse, self.num_points, num_input, trainable=trainable)

    def forward(self, x, gt=None, prefix="train", mean_feature=None, alpha=None):
        if mean_feature:
            raise NotImplementedError
        if self.trainable and torch.is_grad_enabled():
            if x.requires_grad:
                raise ValueError("models.ecg.Model: the gradient with respect to the input cloud is not built (x.requires_grad)")
            return self._forward(x, gt, prefix, alpha)
        with torch.no_grad():
            return self._forward(x, gt, prefix, alpha)

    def _forward(self, x, gt, prefix, alpha):
        rows = x.transpose(1, 2).contiguous().float()
        feat = self.encoder(rows)
        if self.trace is not None:
            self.trace["feat"] = feat
        out1, out2 = self.decoder(feat, rows, self.trace)
        if prefix == "train":
            uniform_loss1 = get_uniform_loss(out1)
            uniform_loss2 = get_uniform_loss(out2)
            if self.train_loss == 'emd':
                loss1 = calc_emd(out1, gt)
                loss2 = calc_emd(out2, gt)
            elif self.train_loss == 'cd':
                loss1, _ = calc_cd(out1, gt)
                loss2, _ = calc_cd(out2, gt)
            else:
                raise NotImplementedError('Train loss is either CD or EMD!')
            total_train_loss = loss1.mean() + uniform_loss1.mean() * 0.1 + (loss2.mean() + uniform_loss2.mean() * 0.1) * alpha
            return out2, loss2, total_train_loss
        elif prefix == "val":
            emd = calc_emd(out2, gt, eps=0.004, iterations=3000) if self.eval_emd else 0
            cd_p, cd_t, f1 = calc_cd(out2, gt, calc_f1=True)
            return {'out1': out1, 'out2': out2, 'emd': emd, 'cd_p': cd_p, 'cd_t': cd_t, 'f1': f1}
        return {'result': out2}
