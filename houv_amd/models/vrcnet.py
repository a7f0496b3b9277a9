"""Mirror of completion/models/vrcnet.py (`SA_module` :21-67, `Folding` :70-113, `Linear_ResBlock` :116-127, `SK_SA_module`
:130-188, `SKN_Res_unit` :191-224, `SA_SKN_Res_encoder` :227-362, `MSAP_SKN_decoder` :365-507, `Model` :510-656): the VRCNet
completion network as an INFERENCE pipeline over the gfx950 kernels of include/houv_hip.h -- houv_mlp2_max for the PCN encoder
it shares with models/pcn.py, one houv_gemm_f32 + houv_sa_attn per point self-attention block (the [B, C, k, N] edge tensor, its
two projections and the [B, mid, k, N] weight tensor are never built), houv_gemm_f32 with the bias / ReLU / residual epilogue for
every 1x1 convolution and linear layer, and the point ops (FPS, houv_knn, houv_knn_cross, three_nn) for the hierarchy.  Nothing
goes through the host.  DESIGN.md section 9.11.

Activations are rows [B, N, C].  The reference's torch.cat of [B, C, N] tensors are column slices of one row-major buffer per
level: a SKN_Res_unit writes its level's features straight into the slice conv7..9 later read beside the up-sampled coarser
level.  conv6 sees cat(global, x4) with the global feature constant over the points, so conv6.weight[:, :1024] g + bias is one
vector per cloud (the split of EF_encoder.conv5); Folding's [B, 1024 + 64 + 2, num_fine] input is the sum of three such parts.

The module tree and parameter names equal the reference's, so its checkpoints load with ``load_state_dict(strict=True)`` (the
repository ships no trained weights: tests use seeded ones).  SA_module, SK_SA_module and SKN_Res_unit take trainable=True
(one _SAAttnFunction node per attention block over houv_sa_attn_backward), and so does
SA_SKN_Res_encoder (section 9.15: each edge-preserve pooling one _EdgePoolFunction node over houv_edge_pool /
houv_edge_pool_backward, which the inference path shares) and MSAP_SKN_decoder (section 9.16: both EF_expansions through
_EFExpandFunction over houv_ef_expand / houv_ef_expand_backward, Folding as the same three-part sum with a graph), and so
does Model (section 9.17): its "train" prefix doubles the batch, draws two latent samples, and sums four Chamfer losses -- each
one cd_loss node over houv_cd_loss_backward, whose sums are ordered -- with the two KL terms.  The reference's MMD branch calls
a method that does not exist; it raises NotImplementedError here.

Two things the reference does that are easy to miss and are kept: Linear_ResBlock's ReLU is in place, so its residual branch
sees relu(feature) and the CALLER's tensor is rectified too -- the decoder receives relu(feat) + generator(z), not feat +
generator(z); and SA_SKN_Res_encoder's decoder call hard-codes pts_num = [3072, 1536, 768, 384] and the `+ 2048` of up_scale.

Discrete decisions.  ``Model(..., trace={})`` records every one of them, as models/ecg.py does: knn{level}_{i} for each level 1..4
and each list i, fps1..3, knn_pt1..3, three_nn1..3, knn_exp1 (+ knn_exp1_x, the rows it was computed from) when up_scale >= 2,
fps_out, topk, knn_exp2 (+ knn_exp2_x) when local_folding is off, plus feat (the PCN encoder's output) and z; the "train"
prefix adds fps_gt (the sample of the ground truth), q_mu, q_std, p_mu, p_std, global_feat, dl_rec, dl_g and loss1..4, all detached from the step's graph.  With
trace=None nothing is recorded or copied."""
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..mm3d_pn2 import furthest_point_sample, knn_cross
from ..model_utils_completion import (Conv1x1, EF_expansion, _LinearFunction, _LinearRowsFunction, _RowGather, _take_rows,
                                       _weight_grad, calc_cd, calc_emd, cd_loss, gen_grid_up)
from .ecg import EF_encoder, _conv, _lin
from .pcn import PCN_encoder


def _linear(layer, x, relu=False, residual=None):
    return ops.gemm(x, layer.weight, shift=layer.bias, residual=residual, relu=relu)


def _flat(t):
    """[B,N,C] rows (one row stride) -> [B*N,C] without a copy where the strides allow it."""
    return t.reshape(-1, t.shape[-1]) if t.is_contiguous() else t.view(-1, t.shape[-1])


class _Conv1x1NoBias(nn.Module):
    """nn.Conv2d(n_in, n_out, 1, bias=False) as a parameter holder: weight [out, in, 1, 1], the reference's initialisation."""

    def __init__(self, n_in, n_out):
        super().__init__()
        bound = 1 / np.sqrt(n_in)
        self.weight = nn.Parameter(torch.empty((n_out, n_in, 1, 1)).uniform_(-bound, bound))

    def matrix(self):
        return self.weight.view(self.weight.shape[0], self.weight.shape[1])


def _knn_rows(pts, k):
    """pts (B,N,3) contiguous -> (B,N,k) int32, itself first: model_utils_completion.knn on rows."""
    if k in (1, 3, 8, 16, 20) and k <= pts.shape[1]:
        return ops.knn(pts, k)
    return knn_cross(k, pts, pts)[1]


def _builds_graph(module, out):
    """True when a module built with trainable=True is called with grad mode on: its forward then keeps a graph.  Everything else
    runs without one, exactly as before."""
    if not (module.trainable and torch.is_grad_enabled()):
        return False
    if out is not None:
        raise ValueError(f"{type(module).__name__}: `out` is not served with trainable=True under grad mode (the result is a node "
                         "of the graph, not a slice of the caller's buffer)")
    return True


class _SAAttnFunction(torch.autograd.Function):
    """SA_module after its input projections as ONE autograd node: ops.sa_attn forward (the inference
    path's own call, so the output carries its bits; `out` is never `x`), and backward = the outer mask, G = gy . Wout on the
    matrix pipe, houv_sa_attn_backward, gWout = gy^T . relu(o) and gbout = sum gy.  Saved: P, idx, the four weight matrices that
    the backward reads and, when relu_out, the output (for its mask).  idx is not differentiable."""

    @staticmethod
    def forward(ctx, P, x, idx, Ww1, Ww2, bw2, Wout, bout, relu_out):
        out = ops.sa_attn(P, x, idx, Ww1, Ww2, bw2, Wout, bout, relu_out=relu_out)
        ctx.relu_out = bool(relu_out)
        ctx.save_for_backward(P, idx, Ww1, Ww2, bw2, Wout, *((out,) if relu_out else ()))
        return out

    @staticmethod
    def backward(ctx, gout):
        P, idx, Ww1, Ww2, bw2, Wout = ctx.saved_tensors[:6]
        gy = (gout * (ctx.saved_tensors[6] > 0)).contiguous() if ctx.relu_out else gout.contiguous()
        B, N, C = gy.shape
        gy2 = gy.view(B * N, C)
        r = ops.sa_attn_backward(P, idx, Ww1, Ww2, bw2, ops.gemm(gy2, Wout, trans_b=False).view(B, N, -1))
        gWout = _weight_grad(gy2, r["ro"].view(B * N, -1))
        return r["gP"], gy, None, r["gWw1"], r["gWw2"], r["gbw2"], gWout, gy2.sum(0), None


class _EdgePoolFunction(torch.autograd.Function):
    """edge_preserve_sampling's feature half as ONE autograd node: feat (B,N,C), p_idx (B,S), pn_idx
    (B,S,pk) -> (B,S,2C) = cat(centre rows, neighbour max) by ops.edge_pool, the inference path's own kernel, with the slot of
    every maximum recorded.  Saved: the two index arrays and the int8 arg -- no feature tensor.  backward =
    ops.edge_pool_backward, the ordered sum per source row."""

    @staticmethod
    def forward(ctx, feat, p_idx, pn_idx):
        out, arg = ops.edge_pool(feat, p_idx, pn_idx, want_arg=True)
        ctx.N = feat.shape[1]
        ctx.save_for_backward(p_idx, pn_idx, arg)
        return out

    @staticmethod
    def backward(ctx, gout):
        p_idx, pn_idx, arg = ctx.saved_tensors
        return ops.edge_pool_backward(gout.contiguous(), p_idx, pn_idx, arg, ctx.N), None, None


class SA_module(nn.Module):
    """vrcnet.py:21-67, the point self-attention block, for what SKN_Res_unit builds: in_planes = out_planes = C in {64, 128, 256,
    512}, rel_planes = C/16, mid_planes = C/4, share_planes = 8 (houv_sa_attn serves these).  trainable=True: with grad mode on,
    forward_rows builds a graph (the projection through _LinearRowsFunction, the rest one _SAAttnFunction node) whose output
    carries the bits of the inference path; x may require a gradient."""

    def __init__(self, in_planes, rel_planes, mid_planes, out_planes, share_planes=8, k=16, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        C = in_planes
        if (C not in (64, 128, 256, 512) or out_planes != C or rel_planes != C // 16 or mid_planes != C // 4 or share_planes != 8
                or not 1 <= k <= 32):
            raise NotImplementedError(f"SA_module({in_planes}, {rel_planes}, {mid_planes}, {out_planes}, {share_planes}, k={k}) has no "
                                      "kernel: C in (64, 128, 256, 512) with C/16, C/4, C, share_planes 8 and k <= 32 are served")
        self.share_planes, self.k = share_planes, k
        self.conv1 = Conv1x1(in_planes, rel_planes, 2)
        self.conv2 = Conv1x1(in_planes, rel_planes, 2)
        self.conv3 = Conv1x1(in_planes, mid_planes, 2)
        self.conv_w = nn.Sequential(nn.ReLU(inplace=False), _Conv1x1NoBias(rel_planes * (k + 1), mid_planes // share_planes),
                                    nn.ReLU(inplace=False), Conv1x1(mid_planes // share_planes, k * mid_planes // share_planes, 2))
        self.conv_out = Conv1x1(mid_planes, out_planes, 2)

    def forward_rows(self, x, idx, relu_out=False, out=None):
        """x (B,N,C) rows (a column slice is fine), idx (B,N,k) int32 -> (B,N,C); relu_out: SK_SA_module's activation."""
        B, N, C = x.shape
        if idx.shape[2] != self.k:
            raise ValueError(f"SA_module: built for k = {self.k}, got lists of {idx.shape[2]}")
        train = _builds_graph(self, out)
        with torch.set_grad_enabled(train):
            W = torch.cat((self.conv1.matrix(), self.conv2.matrix(), self.conv3.matrix()), 0)
            b = torch.cat((self.conv1.bias, self.conv2.bias, self.conv3.bias), 0)
            w = (self.conv_w[1].matrix(), self.conv_w[3].matrix(), self.conv_w[3].bias, self.conv_out.matrix(), self.conv_out.bias)
            if train:
                P = _LinearRowsFunction.apply(torch.relu(x).reshape(-1, C), W, b, False).view(B, N, -1)
                return _SAAttnFunction.apply(P, x, idx, *w, bool(relu_out))
            P = ops.gemm(torch.relu(x).reshape(-1, C), W, shift=b).view(B, N, -1)
            return ops.sa_attn(P, x, idx, *w, relu_out=relu_out, out=out)

    def forward(self, input):
        """[x (B,C,1,N), idx (B,N,k)] -> [out (B,C,1,N), idx], the reference's layout."""
        x, idx = input
        with torch.set_grad_enabled(_builds_graph(self, None)):
            rows = x.squeeze(2).transpose(1, 2).contiguous().float()
            out = self.forward_rows(rows, idx.int().contiguous())
            return [out.transpose(1, 2).unsqueeze(2).contiguous(), idx]


class SK_SA_module(nn.Module):
    """vrcnet.py:130-188: one SA_module per k-NN list, fused by a softmax over the branches.  With one list the softmax is exactly
    1 and the result is relu(SA_module(x)) (fc / fcs exist, for the checkpoint, and are not evaluated)."""

    def __init__(self, in_planes, rel_planes, mid_planes, out_planes, share_planes=8, k=(10, 20), r=2, L=32, trainable=False):
        super().__init__()
        self.num_kernels = len(k)
        self.trainable = bool(trainable)
        d = max(int(out_planes / r), L)
        self.sams = nn.ModuleList([SA_module(in_planes, rel_planes, mid_planes, out_planes, share_planes, ki, trainable=trainable)
                                   for ki in k])
        self.fc = nn.Linear(out_planes, d)
        self.fcs = nn.ModuleList([nn.Linear(d, out_planes) for _ in k])

    def forward_rows(self, x, idxs, out=None):
        assert self.num_kernels == len(idxs)
        train = _builds_graph(self, out)
        with torch.set_grad_enabled(train):
            if self.num_kernels == 1:
                return self.sams[0].forward_rows(x, idxs[0], relu_out=True, out=out)
            # trainable: the same houv_gemm_f32 calls through _LinearFunction; the mean, the softmax and the fusion are torch ops
            linear = (lambda fc, t: _LinearFunction.apply(t, fc.weight, fc.bias, False)) if train else _linear
            feas = [sam.forward_rows(x, idx, relu_out=True) for sam, idx in zip(self.sams, idxs)]
            fea_s = sum(feas[1:], feas[0]).mean(dim=1)                                        # (B,C)
            fea_z = linear(self.fc, fea_s)
            att = torch.softmax(torch.stack([linear(fc, fea_z) for fc in self.fcs], dim=1), dim=1)        # (B,branches,C)
            v = feas[0] * att[:, 0].unsqueeze(1)
            for i in range(1, self.num_kernels):
                v = v + feas[i] * att[:, i].unsqueeze(1)
            if out is not None:
                out.copy_(v)
                return out
            return v

    def forward(self, input):
        x, idxs = input
        with torch.set_grad_enabled(_builds_graph(self, None)):
            rows = x.squeeze(2).transpose(1, 2).contiguous().float()
            out = self.forward_rows(rows, [i.int().contiguous() for i in idxs])
            return [out.transpose(1, 2).unsqueeze(2).contiguous(), idxs]


class SKN_Res_unit(nn.Module):
    """vrcnet.py:191-224: conv2(relu(sam(conv1(feat)))) + conv_res(feat).

    self.af on the last SK_SA_module's output is skipped, with trainable=True too: that output is a convex combination of
    rectified branches (one rectified branch with a single list), so it is >= 0 and relu is the identity on its value.  The
    gradient is unchanged as well: relu's mask [v > 0] could only drop an element with v == 0, and v == 0 means every branch is
    at 0 there (the softmax weights are positive), i.e. every branch's pre-activation was at or below zero, so the branch masks
    [out > 0] of _SAAttnFunction have already dropped that element's gradient on every path it could take."""

    def __init__(self, input_size, output_size, k=(10, 20), layers=1, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.conv1 = _Conv1x1NoBias(input_size, output_size)
        self.sam = nn.Sequential(*[SK_SA_module(output_size, output_size // 16, output_size // 4, output_size, 8, k,
                                                trainable=trainable) for _ in range(int(layers))])
        self.conv2 = _Conv1x1NoBias(output_size, output_size)
        self.conv_res = _Conv1x1NoBias(input_size, output_size)

    def forward_rows(self, feat, idxs, out=None, relu_out=False):
        """feat (B,N,input_size) -> (B,N,output_size), written to `out` (a column slice is fine) when given."""
        B, N, _ = feat.shape
        train = _builds_graph(self, out)
        with torch.set_grad_enabled(train):
            f2 = _flat(feat)
            if train:
                x = _LinearRowsFunction.apply(f2, self.conv1.matrix(), None, False).view(B, N, -1)
                for layer in self.sam:
                    x = layer.forward_rows(x, idxs)
                res = _LinearRowsFunction.apply(f2, self.conv_res.matrix(), None, False)
                # the GEMM's epilogue is (acc + residual), then max(., 0): the same two fp32 operations as these
                y = _LinearRowsFunction.apply(x.reshape(B * N, -1), self.conv2.matrix(), None, False) + res
                return (torch.relu(y) if relu_out else y).view(B, N, -1)
            x = ops.gemm(f2, self.conv1.matrix()).view(B, N, -1)
            for layer in self.sam:
                x = layer.forward_rows(x, idxs)
            res = ops.gemm(f2, self.conv_res.matrix())
            # self.af(x) is the identity here: an SK_SA_module's output is a convex combination of rectified branches
            y = ops.gemm(x.view(B * N, -1), self.conv2.matrix(), None if out is None else _flat(out), residual=res,
                         relu=relu_out)
            return y.view(B, N, -1) if out is None else out


class SA_SKN_Res_encoder(nn.Module):
    """vrcnet.py:227-362 on rows: points (B,N,input_size), coordinates in columns 0..2 -> (B,N,output_size).  N must equal
    pts_num[0] only in so far as the levels below it are sampled to pts_num[1..3] points.

    trainable=True: with grad mode on, forward_rows and forward build a graph the way
    EF_encoder.train_rows does -- the four SKN_Res_units' own graphs, each pooling one _EdgePoolFunction node, the linear layers
    through _LinearRowsFunction / _LinearFunction, the up-samplings through three_interpolate's ordered gradient, the reference's
    concatenations as torch.cat of rows, and the reference's two nn.Dropout() after the rectified fc layers as F.dropout(., 0.5,
    self.training) (no parameters: the state_dict is unchanged).  The lists, samples and interpolation weights come from the
    detached coordinates and are constants, as in the reference; `points` may carry a gradient, which flows through sam_res1.
    In eval() the output carries the bits of the inference path.  With grad mode off, or trainable=False, the inference path
    runs and builds no graph."""

    def __init__(self, input_size=3, k=(10, 20), pk=16, output_size=64, layers=(2, 2, 2, 2), pts_num=(3072, 1536, 768, 384),
                 trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.init_channel = 64
        c1 = self.init_channel
        c2, c3, c4 = c1 * 2, c1 * 4, c1 * 8
        self.sam_res1 = SKN_Res_unit(input_size, c1, k, int(layers[0]), trainable=trainable)
        self.sam_res2 = SKN_Res_unit(c2, c2, k, int(layers[1]), trainable=trainable)
        self.sam_res3 = SKN_Res_unit(c3, c3, k, int(layers[2]), trainable=trainable)
        self.sam_res4 = SKN_Res_unit(c4, c4, k, int(layers[3]), trainable=trainable)
        self.conv5 = Conv1x1(c4, 1024, 2)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 1024)
        self.conv6 = Conv1x1(c4 + 1024, c4, 2)
        self.conv7 = Conv1x1(c3 + c4, c3, 2)
        self.conv8 = Conv1x1(c2 + c3, c2, 2)
        self.conv9 = Conv1x1(c1 + c2, c1, 2)
        self.conv_out = Conv1x1(c1, output_size, 2)
        self.k, self.pk, self.rate, self.pts_num = list(k), pk, 2, list(pts_num)
        self.widths = (c1, c2, c3, c4)

    def _lists(self, level, pts, trace):
        out = []
        for i, k in enumerate(self.k):
            out.append(_knn_rows(pts, k))
            if trace is not None:
                trace[f"knn{level}_{i}"] = out[-1]
        return out

    def _pool(self, level, feat, pts, trace, train=False):
        """edge_preserve_sampling (model_utils.py:90-116) on rows: feat (B,N,C), pts (B,N,3) -> (cat(centre, neighbour max)
        (B,S,2C), the sampled points (B,S,3)).  One houv_edge_pool either way; `train`: as a node of the graph.  The sample and
        the lists are constants."""
        S = self.pts_num[level]
        with torch.no_grad():
            p_idx = furthest_point_sample(pts, S)
            centres = _take_rows(pts, p_idx).contiguous()
            pn_idx = knn_cross(int(min(self.pk, pts.shape[1])), centres, pts)[1]
        if trace is not None:
            trace[f"fps{level}"], trace[f"knn_pt{level}"] = p_idx, pn_idx
        if train:
            return _EdgePoolFunction.apply(feat, p_idx, pn_idx), centres
        return ops.edge_pool(feat, p_idx, pn_idx), centres

    def forward_rows(self, points, trace=None, out=None):
        """points (B,N,input_size) -> (B,N,output_size), written to `out` when given (the inference path only)."""
        if _builds_graph(self, out):
            return self._train_rows(points, trace)
        with torch.no_grad():
            return self._infer_rows(points, trace, out)

    def _train_rows(self, points, trace):
        """forward_rows with a graph: the same calls in the same order, the buffers' column slices as torch.cat of rows."""
        B = points.shape[0]
        c4 = self.widths[3]
        pt1 = points.detach()[..., :3].contiguous()
        x1 = self.sam_res1.forward_rows(points, self._lists(1, pt1, trace), relu_out=True)
        f, pt2 = self._pool(1, x1, pt1, trace, train=True)
        x2 = self.sam_res2.forward_rows(f, self._lists(2, pt2, trace), relu_out=True)
        f, pt3 = self._pool(2, x2, pt2, trace, train=True)
        x3 = self.sam_res3.forward_rows(f, self._lists(3, pt3, trace), relu_out=True)
        f, pt4 = self._pool(3, x3, pt3, trace, train=True)
        x4 = self.sam_res4.forward_rows(f, self._lists(4, pt4, trace), relu_out=True)

        g = _conv(self.conv5, x4).max(dim=1).values
        g = F.dropout(_LinearFunction.apply(g, self.fc1.weight, self.fc1.bias, True), 0.5, self.training)
        g = F.dropout(_LinearFunction.apply(g, self.fc2.weight, self.fc2.bias, True), 0.5, self.training)
        W6 = self.conv6.matrix()
        shift = _LinearFunction.apply(g, W6[:, :1024], self.conv6.bias, False)    # the global feature's share of conv6, per cloud
        y = torch.relu(_lin(x4, W6[:, 1024:], None).view(B, -1, c4) + shift.unsqueeze(1))
        y = _conv(self.conv7, torch.cat((EF_encoder._upsample_train(1, y, pt3, pt4, trace), x3), dim=2), relu=True)
        y = _conv(self.conv8, torch.cat((EF_encoder._upsample_train(2, y, pt2, pt3, trace), x2), dim=2), relu=True)
        y = _conv(self.conv9, torch.cat((EF_encoder._upsample_train(3, y, pt1, pt2, trace), x1), dim=2), relu=True)
        return _conv(self.conv_out, y)

    def _infer_rows(self, points, trace, out):
        B, N, _ = points.shape
        c1, c2, c3, c4 = self.widths
        new = lambda n, c: torch.empty((B, n, c), dtype=torch.float32, device=points.device)
        # one buffer per level: [the coarser level's features, up-sampled | the level's own], the operand of conv7..9
        X1, X2, X3 = new(N, c2 + c1), new(self.pts_num[1], c3 + c2), new(self.pts_num[2], c4 + c3)
        pt1 = points[..., :3].contiguous()
        x1 = self.sam_res1.forward_rows(points, self._lists(1, pt1, trace), out=X1[..., c2:], relu_out=True)
        f, pt2 = self._pool(1, x1, pt1, trace)
        x2 = self.sam_res2.forward_rows(f, self._lists(2, pt2, trace), out=X2[..., c3:], relu_out=True)
        f, pt3 = self._pool(2, x2, pt2, trace)
        x3 = self.sam_res3.forward_rows(f, self._lists(3, pt3, trace), out=X3[..., c4:], relu_out=True)
        f, pt4 = self._pool(3, x3, pt3, trace)
        x4 = self.sam_res4.forward_rows(f, self._lists(4, pt4, trace), relu_out=True)

        g = self.conv5.rows(x4).amax(dim=1)
        g = _linear(self.fc2, _linear(self.fc1, g, relu=True), relu=True)                 # dropout: the identity at inference
        W6 = self.conv6.matrix()
        shift = ops.gemm(g, W6[:, :1024], shift=self.conv6.bias)                  # the global feature's share of conv6, per cloud
        y = torch.relu_(ops.gemm(x4.view(-1, c4), W6[:, 1024:]).view(B, -1, c4) + shift.unsqueeze(1))
        EF_encoder._upsample(1, y, pt3, pt4, X3[..., :c4], trace)
        y = self.conv7.rows(X3, relu=True)
        EF_encoder._upsample(2, y, pt2, pt3, X2[..., :c3], trace)
        y = self.conv8.rows(X2, relu=True)
        EF_encoder._upsample(3, y, pt1, pt2, X1[..., :c2], trace)
        y = self.conv9.rows(X1, relu=True)
        return self.conv_out.rows(y, out=out)

    def forward(self, features):
        """features (B,input_size,N) -> (B,output_size,N), the reference's layout."""
        with torch.set_grad_enabled(_builds_graph(self, None)):
            return self.forward_rows(features.transpose(1, 2).contiguous().float()).transpose(1, 2).contiguous()


class Folding(nn.Module):
    """vrcnet.py:70-113 on rows: (point_feat (B,n,input_size), global_feat (B,G)) -> (B,n*step_ratio,output_size).  The
    [B, G + input_size + 2, n*step_ratio] input is never built: the pre-activation is the sum of conv.weight's global columns
    (one vector per cloud), its point columns (one per coarse point) and its grid columns (one per grid cell).  trainable=True
    with grad mode on: the same sum with a graph (the two products through _LinearFunction / _LinearRowsFunction over column
    slices of conv.weight, the two grid columns a torch product as below), to both inputs and the convolution."""

    def __init__(self, input_size, output_size, step_ratio, global_feature_size=1024, num_models=1, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.input_size, self.output_size, self.step_ratio, self.num_models = input_size, output_size, step_ratio, num_models
        self.global_feature_size = global_feature_size
        self.conv = Conv1x1(input_size + global_feature_size + 2, output_size, 1)
        # (step_ratio, 2): the reference's factorisation loop and linspace (a 1-step axis is the single value -0.2); not a
        # parameter and not in the state_dict, as in the reference, but it follows the module to its device
        self.register_buffer("grid", gen_grid_up(step_ratio, 0.2).transpose(0, 1).contiguous(), persistent=False)

    def forward_rows(self, point_feat, global_feat):
        B, n, _ = point_feat.shape
        W, G = self.conv.matrix(), self.global_feature_size
        if self.trainable and torch.is_grad_enabled():
            g = _LinearFunction.apply(global_feat, W[:, :G], self.conv.bias, False)
            p = _LinearRowsFunction.apply(_flat(point_feat), W[:, G:G + self.input_size], None, False).view(B, n, 1, -1)
            q = self.grid @ W[:, G + self.input_size:].t()
            return torch.relu((p + g.view(B, 1, 1, -1)) + q.view(1, 1, self.step_ratio, -1)).view(B, n * self.step_ratio, -1)
        with torch.no_grad():
            return self._forward_rows(point_feat, global_feat)

    def _forward_rows(self, point_feat, global_feat):
        B, n, _ = point_feat.shape
        W, G = self.conv.matrix(), self.global_feature_size
        g = ops.gemm(global_feat, W[:, :G], shift=self.conv.bias)                                        # (B,out)
        p = ops.gemm(_flat(point_feat), W[:, G:G + self.input_size]).view(B, n, 1, -1)
        q = self.grid @ W[:, G + self.input_size:].t()                                                   # (step,out): 2 columns
        return torch.relu_((p + g.view(B, 1, 1, -1)) + q.view(1, 1, self.step_ratio, -1)).view(B, n * self.step_ratio, -1)


class Linear_ResBlock(nn.Module):
    """vrcnet.py:116-127.  The reference's ReLU is in place: the residual branch sees relu(feature) too.

    trainable=True: with grad mode on, the same three products through _LinearFunction, the first
    ReLU and the residual add as torch ops.  The GEMM's epilogue computes (acc + bias) + residual, and so does this path
    ((acc + bias) from conv2's node, then + the residual branch): the output carries the bits of the inference path.  With grad
    mode off, or trainable=False, the inference path runs and builds no graph."""

    def __init__(self, input_size=1024, output_size=256, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.conv1 = nn.Linear(input_size, input_size)
        self.conv2 = nn.Linear(input_size, output_size)
        self.conv_res = nn.Linear(input_size, output_size)

    def forward(self, feature):
        if self.trainable and torch.is_grad_enabled():
            lin = lambda fc, t, relu: _LinearFunction.apply(t, fc.weight, fc.bias, relu)
            r = torch.relu(feature)
            return lin(self.conv2, lin(self.conv1, r, True), False) + lin(self.conv_res, r, False)
        with torch.no_grad():
            r = torch.relu(feature)
            return _linear(self.conv2, _linear(self.conv1, r, relu=True), residual=_linear(self.conv_res, r))


class MSAP_SKN_decoder(nn.Module):
    """vrcnet.py:365-507: (global_feat (B,1024), input points (B,num_input,3)) -> (coarse_raw, coarse_high, coarse, fine), rows
    of points.

    trainable=True: with grad mode on, forward builds a graph -- fc1..3 through _LinearFunction, the
    encoder's own trainable path (coarse_raw carries a gradient into sam_res1), both EF_expansions through _EFExpandFunction,
    conv_cup1/2 and conv_f1/2 through _LinearRowsFunction, Folding's graph path, and both row selections through _RowGather.
    The furthest-point sample runs on the detached coarse_high and the score branch under no_grad: its top-k yields indices
    only, so conv_s1..3 get no gradient, exactly as in the reference.  global_feat may require a gradient; a point_input that
    does is refused.  With grad mode off, or trainable=False, the inference path runs and builds no graph; the graph path's
    output equals it within fp32 spread, not bit for bit (the expansions' per-point split rounds differently)."""

    def __init__(self, num_coarse_raw, num_fps, num_coarse, num_fine, layers=(2, 2, 2, 2), knn_list=(10, 20), pk=10,
                 points_label=False, local_folding=False, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.num_coarse_raw, self.num_fps, self.num_coarse, self.num_fine = num_coarse_raw, num_fps, num_coarse, num_fine
        self.points_label, self.local_folding = points_label, local_folding
        self.fc1 = nn.Linear(1024, 1024)
        self.fc2 = nn.Linear(1024, 1024)
        self.fc3 = nn.Linear(1024, num_coarse_raw * 3)
        self.dense_feature_size, self.expand_feature_size = 256, 64
        self.input_size = 4 if points_label else 3
        self.encoder = SA_SKN_Res_encoder(input_size=self.input_size, k=knn_list, pk=pk, output_size=self.dense_feature_size,
                                          layers=layers, trainable=trainable)
        self.up_scale = int(np.ceil(num_fine / (num_coarse_raw + 2048)))
        if self.up_scale >= 2:
            self.expansion1 = EF_expansion(input_size=self.dense_feature_size, output_size=self.expand_feature_size,
                                           step_ratio=self.up_scale, k=4, trainable=trainable)
            self.conv_cup1 = Conv1x1(self.expand_feature_size, self.expand_feature_size)
        else:
            self.expansion1 = None
            self.conv_cup1 = Conv1x1(self.dense_feature_size, self.expand_feature_size)
        self.conv_cup2 = Conv1x1(self.expand_feature_size, 3)
        self.conv_s1 = Conv1x1(self.expand_feature_size, 16)
        self.conv_s2 = Conv1x1(16, 8)
        self.conv_s3 = Conv1x1(8, 1)
        if local_folding:
            self.expansion2 = Folding(input_size=self.expand_feature_size, output_size=self.dense_feature_size,
                                      step_ratio=num_fine // num_coarse, trainable=trainable)
        else:
            self.expansion2 = EF_expansion(input_size=self.expand_feature_size, output_size=self.dense_feature_size,
                                           step_ratio=num_fine // num_coarse, k=4, trainable=trainable)
        self.conv_f1 = Conv1x1(self.dense_feature_size, self.expand_feature_size)
        self.conv_f2 = Conv1x1(self.expand_feature_size, 3)

    def forward(self, global_feat, point_input, trace=None):
        if self.trainable and torch.is_grad_enabled():
            if point_input.requires_grad:
                raise ValueError("MSAP_SKN_decoder: the gradient with respect to the input cloud is not built (point_input.requires_grad)")
            return self._forward_train(global_feat, point_input, trace)
        with torch.no_grad():
            return self._forward(global_feat, point_input, trace)

    def _forward_train(self, global_feat, point_input, trace):
        """forward with a graph: the same steps in the same order; every discrete decision from detached values."""
        B = global_feat.shape[0]
        lin = lambda fc, t, relu: _LinearFunction.apply(t, fc.weight, fc.bias, relu)
        raw = lin(self.fc3, lin(self.fc2, lin(self.fc1, global_feat, True), True), False)
        coarse_raw = raw.view(B, 3, self.num_coarse_raw).transpose(1, 2).contiguous()
        points = torch.cat((coarse_raw, point_input), dim=1)
        if self.points_label:
            label = points.new_ones((B, points.shape[1], 1))
            label[:, :self.num_coarse_raw] = 0
            points = torch.cat((points, label), dim=2)
        dense = self.encoder.forward_rows(points, trace)
        if self.up_scale >= 2:
            dense = self.expansion1.forward_rows(dense, trace=trace, name="knn_exp1")
        feats = _conv(self.conv_cup1, dense, relu=True)
        coarse_high = _conv(self.conv_cup2, feats)
        coarse = coarse_high
        if coarse.shape[1] > self.num_fps:
            with torch.no_grad():
                idx = furthest_point_sample(coarse_high.detach().contiguous(), self.num_fps)
            if trace is not None:
                trace["fps_out"] = idx
            coarse, feats = _RowGather.apply(coarse_high, idx).contiguous(), _RowGather.apply(feats, idx).contiguous()
        if coarse.shape[1] > self.num_coarse:
            with torch.no_grad():                # the scores select rows and carry no gradient: top-k returns indices only
                s = self.conv_s3.rows(self.conv_s2.rows(self.conv_s1.rows(feats.detach(), relu=True), relu=True))
                idx = F.softplus(s).view(B, -1).topk(self.num_coarse, dim=1)[1].int()
            if trace is not None:
                trace["topk"] = idx
            coarse, feats = _RowGather.apply(coarse, idx).contiguous(), _RowGather.apply(feats, idx).contiguous()
        if coarse.shape[1] < self.num_fine:
            step = self.num_fine // self.num_coarse
            if self.local_folding:
                up = self.expansion2.forward_rows(feats, global_feat)
                centre = coarse.unsqueeze(2).expand(-1, -1, step, -1).reshape(B, self.num_fine, 3)
                fine = _conv(self.conv_f2, _conv(self.conv_f1, up, relu=True)) + centre
            else:
                up = self.expansion2.forward_rows(feats, trace=trace, name="knn_exp2")
                fine = _conv(self.conv_f2, _conv(self.conv_f1, up, relu=True))
        else:
            assert coarse.shape[1] == self.num_fine
            fine = coarse
        return coarse_raw, coarse_high, coarse, fine

    def _forward(self, global_feat, point_input, trace=None):
        B = global_feat.shape[0]
        raw = _linear(self.fc3, _linear(self.fc2, _linear(self.fc1, global_feat, relu=True), relu=True))
        coarse_raw = raw.view(B, 3, self.num_coarse_raw).transpose(1, 2).contiguous()
        points = torch.cat((coarse_raw, point_input), dim=1)
        if self.points_label:
            label = points.new_ones((B, points.shape[1], 1))
            label[:, :self.num_coarse_raw] = 0
            points = torch.cat((points, label), dim=2)
        dense = self.encoder.forward_rows(points, trace)
        if self.up_scale >= 2:
            dense = self.expansion1.forward_rows(dense, trace=trace, name="knn_exp1")
        feats = self.conv_cup1.rows(dense, relu=True)
        coarse_high = self.conv_cup2.rows(feats)
        coarse = coarse_high
        if coarse.shape[1] > self.num_fps:
            idx = furthest_point_sample(coarse_high, self.num_fps)
            if trace is not None:
                trace["fps_out"] = idx
            coarse, feats = _take_rows(coarse_high, idx).contiguous(), _take_rows(feats, idx).contiguous()
        if coarse.shape[1] > self.num_coarse:
            s = self.conv_s3.rows(self.conv_s2.rows(self.conv_s1.rows(feats, relu=True), relu=True))
            idx = F.softplus(s).view(B, -1).topk(self.num_coarse, dim=1)[1].int()
            if trace is not None:
                trace["topk"] = idx
            coarse, feats = _take_rows(coarse, idx).contiguous(), _take_rows(feats, idx).contiguous()
        if coarse.shape[1] < self.num_fine:
            step = self.num_fine // self.num_coarse
            if self.local_folding:
                up = self.expansion2.forward_rows(feats, global_feat)
                centre = coarse.unsqueeze(2).expand(-1, -1, step, -1).reshape(B, self.num_fine, 3)
                fine = self.conv_f2.rows(self.conv_f1.rows(up, relu=True)) + centre
            else:
                up = self.expansion2.forward_rows(feats, trace=trace, name="knn_exp2")
                fine = self.conv_f2.rows(self.conv_f1.rows(up, relu=True))
        else:
            assert coarse.shape[1] == self.num_fine
            fine = coarse
        return coarse_raw, coarse_high, coarse, fine


class Model(nn.Module):
    """``Model(args, size_z=128, global_feature_size=1024, trace=None, trainable=False).forward(x[B,3,N], gt=None,
    prefix="train", mean_feature=None, alpha=None, z=None, eps=None)`` (vrcnet.py:510-656).  ``args``: layers, knn_list
    (comma-separated strings), distribution_loss, loss, eval_emd, num_fps, num_points, num_coarse, num_coarse_raw, pk,
    local_folding, points_label (cfgs/vrcnet_mi355x.yaml).

    "test": {'result': fine}.  "val": the reference's dictionary out1 (coarse_raw), out2 (fine), cd_p, cd_t, f1, and 'emd' as well
    when eval_emd is set (the reference computes it and drops it).  Both run the inference path, without a graph, under either
    flag and either grad mode.

    "train" (trainable=True) -> (fine [2B, num_points, 3], loss4_t [2B], total), the reference's tuple
    with rows of points: the batch doubled with a furthest-point sample of gt, the posterior from x and the prior from that
    sample, one latent draw from each, the decoder on both, four cd_loss nodes against the doubled gt and the two KL terms.
    With grad mode on, total.backward() reaches every parameter but conv_s1..3 (the scores only select rows), and two steps
    from the same state, `eps` and dropout seed give bit-equal gradients.  Under torch.no_grad() the same tuple is computed
    without a graph: the decoder then runs its inference path, whose two dropouts are the identity, so it is the eval() result
    (within the fp32 spread between the decoder's two paths).  With the default trainable=False "train" raises
    NotImplementedError.

    The reference draws the latent z = q.rsample() even under "test"; ``z`` (B,size_z), when given, replaces the sample, and
    with z=None q_mu + softplus(q_std) * randn is drawn on the device (torch's generator: seed it for a repeatable result).
    ``eps`` = (eps_q, eps_p), two (B,size_z) tensors, does the same for the two draws of "train": z_q = q_mu + q_std * eps_q,
    z_p = p_mu + p_std * eps_p."""

    def __init__(self, args, size_z=128, global_feature_size=1024, trace=None, trainable=False):
        super().__init__()
        layers = [int(i) for i in str(args.layers).split(',')]
        knn_list = [int(i) for i in str(args.knn_list).split(',')]
        self.size_z = size_z
        self.distribution_loss, self.train_loss, self.eval_emd = args.distribution_loss, args.loss, args.eval_emd
        self.trace = trace
        self.trainable = bool(trainable)
        block = lambda n_in, n_out: Linear_ResBlock(input_size=n_in, output_size=n_out, trainable=trainable)
        self.encoder = PCN_encoder(output_size=global_feature_size, trainable=trainable)
        self.posterior_infer1 = block(global_feature_size, global_feature_size)
        self.posterior_infer2 = block(global_feature_size, size_z * 2)
        self.prior_infer = block(global_feature_size, size_z * 2)
        self.generator = block(size_z, global_feature_size)
        self.decoder = MSAP_SKN_decoder(num_fps=args.num_fps, num_fine=args.num_points, num_coarse=args.num_coarse,
                                        num_coarse_raw=args.num_coarse_raw, layers=layers, knn_list=knn_list, pk=args.pk,
                                        local_folding=args.local_folding, points_label=args.points_label, trainable=trainable)

    def forward(self, x, gt=None, prefix="train", mean_feature=None, alpha=None, z=None, eps=None):
        if prefix == "train":
            if not self.trainable:
                raise NotImplementedError('VRCNet: the "train" prefix (doubled batch, two latent samples, KL terms) needs '
                                          'Model(..., trainable=True)')
            return self._forward_train(x, gt, alpha, eps)
        with torch.no_grad():
            return self._forward_infer(x, gt, prefix, z)

    def _forward_train(self, x, gt, alpha, eps):
        """vrcnet.py:565-641 on rows.  The reference rectifies feat_x and feat_y in place (posterior_infer1's and prior_infer's
        ReLU act on views of the encoder's output, which torch 2.10 refuses on a chunk view): relu(feat_x) and relu(feat_y)
        are the values every later use sees, and the gradients flow back through those two ReLUs."""
        if self.distribution_loss == "MMD":
            raise NotImplementedError("VRCNet: distribution_loss = 'MMD' is not built (the reference's branch calls mmd_loss2, a "
                                      "method that does not exist)")
        if self.distribution_loss != "KLD":
            raise NotImplementedError("Distribution loss is either MMD or KLD")
        if self.train_loss != "cd":
            raise NotImplementedError("Only CD is supported")
        if gt is None or alpha is None:
            raise ValueError('VRCNet: the "train" prefix needs gt and alpha')
        if x.requires_grad:
            raise ValueError("VRCNet: the gradient with respect to the input cloud is not built (x.requires_grad)")
        if self.training and not torch.is_grad_enabled():
            warnings.warn('VRCNet: "train" under torch.no_grad() runs the decoder\'s inference path, whose dropouts are the identity: '
                          "the result is the eval() one although the model is in train() mode", stacklevel=3)
        rows = x.transpose(1, 2).contiguous().float()
        gt = gt.detach().contiguous().float()
        with torch.no_grad():                                        # the sample is a constant
            fps_gt = furthest_point_sample(gt, rows.shape[1])
            y = _take_rows(gt, fps_gt).contiguous()
        feat = self.encoder(torch.cat((rows, y), dim=0))
        q_mu, q_std, p_mu, p_std, z, global_feat, dl_rec, dl_g = self._latent_head(*feat.chunk(2), eps)
        x2, gt2 = torch.cat((rows, rows), dim=0), torch.cat((gt, gt), dim=0)
        coarse_raw, coarse_high, coarse, fine = self.decoder(global_feat, x2, self.trace)
        loss1, _ = cd_loss(coarse_raw, gt2)
        loss2, _ = cd_loss(coarse_high, gt2)
        loss3, _ = cd_loss(coarse, gt2)
        loss4, loss4_t = cd_loss(fine, gt2)
        total = loss1.mean() * 10 + loss2.mean() * 0.5 + loss3.mean() + loss4.mean() * alpha
        total = total + (dl_rec.mean() + dl_g.mean()) * 20
        if self.trace is not None:                       # detached: a trace that is kept does not keep the step's graph alive
            rec = dict(feat=feat, fps_gt=fps_gt, q_mu=q_mu, q_std=q_std, p_mu=p_mu, p_std=p_std, z=z, global_feat=global_feat,
                       dl_rec=dl_rec, dl_g=dl_g, loss1=loss1, loss2=loss2, loss3=loss3, loss4=loss4,
                       coarse_raw=coarse_raw, coarse_high=coarse_high, coarse=coarse, fine=fine)
            self.trace.update({n: t.detach() for n, t in rec.items()})
        return fine, loss4_t, total

    def _latent_head(self, feat_x, feat_y, eps):
        """vrcnet.py:578-605 and :622-625 from the two halves of the encoder's output: -> (q_mu, q_std, p_mu, p_std, z,
        global_feat, dl_rec, dl_g).  The two ReLUs are the reference's in-place ones: relu(feat_x) is what the generator's
        output is added to."""
        Normal, kl = torch.distributions.Normal, torch.distributions.kl_divergence
        B = feat_x.shape[0]
        feat_x, feat_y = torch.relu(feat_x), torch.relu(feat_y)
        q_mu, q_std = torch.split(self.posterior_infer2(self.posterior_infer1(feat_x)), self.size_z, dim=1)
        p_mu, p_std = torch.split(self.prior_infer(feat_y), self.size_z, dim=1)
        q_std, p_std = F.softplus(q_std), F.softplus(p_std)
        if eps is None:
            eps = (torch.randn_like(q_mu), torch.randn_like(p_mu))
        eps_q, eps_p = (e.detach().to(feat_x.dtype) for e in eps)
        if tuple(eps_q.shape) != (B, self.size_z) or tuple(eps_p.shape) != (B, self.size_z):
            raise ValueError(f"VRCNet: eps must be a pair of [{B},{self.size_z}] tensors")
        z = torch.cat((q_mu + q_std * eps_q, p_mu + p_std * eps_p), dim=0).contiguous()
        global_feat = torch.cat((feat_x, feat_x), dim=0) + self.generator(z)
        dl_rec = kl(Normal(torch.zeros_like(p_mu), torch.ones_like(p_std)), Normal(p_mu, p_std))
        dl_g = kl(Normal(p_mu.detach(), p_std.detach()), Normal(q_mu, q_std))
        return q_mu, q_std, p_mu, p_std, z, global_feat, dl_rec, dl_g

    def _forward_infer(self, x, gt, prefix, z):
        rows = x.transpose(1, 2).contiguous().float()
        feat = self.encoder(rows)
        o_x = self.posterior_infer2(self.posterior_infer1(feat))
        q_mu, q_std = torch.split(o_x, self.size_z, dim=1)
        if z is None:
            z = q_mu + F.softplus(q_std) * torch.randn_like(q_mu)
        z = z.to(feat.dtype).contiguous()
        if self.trace is not None:
            self.trace["feat"], self.trace["z"] = feat, z
        # posterior_infer1's in-place ReLU has rectified feat by the time the reference adds the generator's output to it
        global_feat = torch.relu(feat) + self.generator(z)
        coarse_raw, coarse_high, coarse, fine = self.decoder(global_feat, rows, self.trace)
        if self.trace is not None:
            self.trace.update(coarse_raw=coarse_raw, coarse_high=coarse_high, coarse=coarse, fine=fine)
        if prefix == "val":
            cd_p, cd_t, f1 = calc_cd(fine, gt, calc_f1=True)
            res = {'out1': coarse_raw, 'out2': fine, 'cd_p': cd_p, 'cd_t': cd_t, 'f1': f1}
            if self.eval_emd:
                res['emd'] = calc_emd(fine, gt, eps=0.004, iterations=3000)
            return res
        return {'result': fine}
