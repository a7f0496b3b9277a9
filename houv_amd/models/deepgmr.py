"""Mirror of registration/models/deepgmr.py (`Model`, :200-255): DeepGMR -- rotation-invariant RRI features (:54-95), a
PointNet that turns each point into responsibilities over J Gaussians (:174-197), the mixture parameters of both clouds (:98-120)
and the closed-form pose between the two mixtures (:123-143) -- as an INFERENCE pipeline over the gfx950 kernels of
include/houv_hip.h: houv_knn_cross + houv_rri_features, houv_gemm_f32 with the folded-BatchNorm/ReLU epilogue for every 1x1
convolution, houv_softmax_rows, houv_gmm_params, houv_gmm_register.  Nothing goes through the host: the reference copies the
tangent vectors to NumPy for the features and runs the 3x3 SVD on the CPU.

The module tree and parameter names equal the reference's, so a reference checkpoint's ``net_state_dict`` loads with
``load_state_dict`` unchanged (the repository ships no trained weights: tests use seeded random ones).  BatchNorm runs in eval
mode (running statistics).  Activations are point-major rows [B*N, C] throughout (the reference keeps [B, C, N]).

``Model(args, trainable=True)`` in ``train()`` mode is the reference's training forward: BatchNorm on the
batch statistics (houv_bn_rows_stats, houv_bn_relu_rows and its backward, one autograd node per Conv1DBNReLU), the head as
autograd nodes over houv_gmm_params_backward and houv_gmm_register_backward, the 4x4 loss algebra in torch.  In ``eval()`` mode
it is the inference pipeline above, bit for bit."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..model_utils import get_rri_cluster, rri_rows  # noqa: F401  (get_rri_cluster: the reference's module-level name)
from ..model_utils_completion import _LinearRowsFunction, _transposed, _weight_grad
from ..train_utils import rmse_loss, rotation_error, rotation_geodesic_error, translation_error
from .dcp import _BN


def gmm_params(gamma, pts):
    """gamma[B,N,J], pts[B,N,3] -> (pi[B,J], mu[B,J,3], sigma[B,J]).  sigma is the scalar of the reference's isotropic
    ``sigma * eye(3)`` [B,J,3,3] (deepgmr.py:117-119); `gmm_register` below takes the scalar."""
    return ops.gmm_params(gamma.contiguous().float(), pts.contiguous().float())


def gmm_register(pi_s, mu_s, mu_t, sigma_t):
    """-> T[B,4,4] (deepgmr.py:123-143).  sigma_t: the scalar [B,J] of `gmm_params`, or the reference's [B,J,3,3] sigma * eye(3)."""
    if sigma_t.dim() == 4:
        sigma_t = sigma_t[:, :, 0, 0]
    return ops.gmm_register(pi_s.contiguous().float(), mu_s.contiguous().float(), mu_t.contiguous().float(),
                            sigma_t.contiguous().float())


class _ConvBNReLUFunction(torch.autograd.Function):
    """relu(bn(x W^T)) under BATCH statistics as one node: a raw GEMM, houv_bn_rows_stats, houv_bn_relu_rows; backward: the fused
    BatchNorm / ReLU backward (mask and xhat recomputed from the saved z), then gx = gz W and gW = gz^T x (_weight_grad).  gx is
    left out when x needs none (the first layer: features carry no gradient).  n_group > 0 also returns the per-cloud column
    maximum and its lowest row (the max-pool, read off the same pass).  -> (y, mean, var[, gmax, garg])."""

    @staticmethod
    def forward(ctx, x, W, weight, bias, eps, n_group):
        z = ops.gemm(x, W)
        mean, var = ops.bn_rows_stats(z)
        out = ops.bn_relu_rows(z, mean, var, weight, bias, eps, True, n_group)
        out = (out, mean, var) if not n_group else (out[0], mean, var, out[1], out[2])
        ctx.eps = eps
        ctx.save_for_backward(x, W, z, mean, var, weight, bias)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, gy, *unused):
        x, W, z, mean, var, weight, bias = ctx.saved_tensors
        gz, gweight, gbias = ops.bn_relu_rows_backward(gy.contiguous(), z, mean, var, weight, bias, ctx.eps, True)
        gx = ops.gemm(gz, W, trans_b=False) if ctx.needs_input_grad[0] else None
        return gx, _weight_grad(gz, x), gweight, gbias, None, None


class _DecoderFirstFunction(torch.autograd.Function):
    """The decoder's first Conv1DBNReLU on cat(f_loc, f_glob) in the split form of PointNet.forward, under batch statistics, with
    the max-pool's backward folded in.  Forward: z = f_loc W_loc^T + (f_glob W_glob^T, one row per cloud, as the GEMM's
    residual).  Backward: the residual's gradient is the per-cloud column sum of gz; it gives W_glob's gradient and, times
    W_glob, the gradient of f_glob, which returns to f_loc at the rows the maxima came from (garg: one row per (cloud, channel),
    so the scatter touches every address once).  No [B*N, 2048] tensor in either direction.  -> (y, mean, var)."""

    @staticmethod
    def forward(ctx, f_loc, f_glob, garg, W, weight, bias, eps):
        B, C = f_glob.shape
        N = f_loc.shape[0] // B
        O = W.shape[0]
        res = ops.gemm(f_glob, W[:, C:])                                        # [B, 512]
        z = ops.gemm(f_loc.view(B, N, C), W[:, :C].unsqueeze(0).expand(B, O, C),
                     residual=res.unsqueeze(1).expand(B, N, O)).view(B * N, O)
        mean, var = ops.bn_rows_stats(z)
        y = ops.bn_relu_rows(z, mean, var, weight, bias, eps, True)
        ctx.eps = eps
        ctx.save_for_backward(f_loc, f_glob, garg, W, z, mean, var, weight, bias)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, gy, *unused):
        f_loc, f_glob, garg, W, z, mean, var, weight, bias = ctx.saved_tensors
        B, C = f_glob.shape
        O = W.shape[0]
        gz, gweight, gbias = ops.bn_relu_rows_backward(gy.contiguous(), z, mean, var, weight, bias, ctx.eps, True)
        gres = gz.view(B, -1, O).sum(1)                                         # [B, 512]
        gW = torch.cat((_weight_grad(gz, f_loc), ops.gemm(_transposed(gres), _transposed(f_glob))), 1)
        gx = ops.gemm(gz, W[:, :C], trans_b=False)                              # [B*N, 1024]
        gglob = ops.gemm(gres, W[:, C:], trans_b=False)                         # [B, 1024]
        at = (garg.long() * C + torch.arange(C, device=garg.device)).view(-1)   # distinct addresses: no accumulation needed
        flat = gx.view(-1)
        flat[at] = flat[at] + gglob.view(-1)
        return gx, None, None, gW, gweight, gbias, None


class _GmmParamsFunction(torch.autograd.Function):
    """logits[B,N,J], pts -> (gamma, pi, mu, sigma): houv_softmax_rows and houv_gmm_params; backward houv_gmm_params_backward
    (softmax backward included).  gamma is returned for the module's records and carries no gradient of its own."""

    @staticmethod
    def forward(ctx, logits, pts):
        gamma = ops.softmax_rows_(logits.detach().clone())
        pi, mu, sigma = ops.gmm_params(gamma, pts)
        ctx.save_for_backward(gamma, pts, pi, mu, sigma)
        ctx.mark_non_differentiable(gamma)
        return gamma, pi, mu, sigma

    @staticmethod
    def backward(ctx, g_gamma, g_pi, g_mu, g_sigma):
        gamma, pts, pi, mu, sigma = ctx.saved_tensors
        return ops.gmm_params_backward(gamma, pts, pi, mu, sigma, g_pi.contiguous(), g_mu.contiguous(), g_sigma.contiguous()), None


class _GmmRegisterFunction(torch.autograd.Function):
    """gmm_register with houv_gmm_register_backward (the polar form of the rotation's derivative; no SVD on the host)."""

    @staticmethod
    def forward(ctx, pi_s, mu_s, mu_t, sigma_t):
        ctx.save_for_backward(pi_s, mu_s, mu_t, sigma_t)
        return ops.gmm_register(pi_s, mu_s, mu_t, sigma_t)

    @staticmethod
    def backward(ctx, g_T):
        return ops.gmm_register_backward(*ctx.saved_tensors, g_T.contiguous())


class _Conv1d(nn.Module):
    def __init__(self, n_in, n_out, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n_out, n_in, 1).uniform_(-1, 1) / n_in ** 0.5)
        if bias:
            self.bias = nn.Parameter(torch.zeros(n_out))


class _Linear(nn.Module):
    def __init__(self, n_in, n_out, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n_out, n_in).uniform_(-1, 1) / n_in ** 0.5)
        if bias:
            self.bias = nn.Parameter(torch.zeros(n_out))

    def forward(self, x):
        return ops.gemm(x, self.weight, shift=self.bias)


class Conv1DBNReLU(nn.Module):
    """relu(bn(conv1x1(x))) on rows x[R, C_in] -> [R, C_out]: one GEMM, BatchNorm and ReLU in its epilogue (deepgmr.py:44-51)."""

    def __init__(self, in_channel, out_channel, ksize=1):
        super().__init__()
        assert ksize == 1
        self.conv = _Conv1d(in_channel, out_channel, bias=False)
        self.bn = _BN(out_channel)

    def forward(self, x):
        s, h = self.bn.folded()
        return ops.gemm(x, self.conv.weight.squeeze(2), scale=s, shift=h, relu=True)

    def forward_train(self, x, n_group=0):
        """The layer under batch statistics (one _ConvBNReLUFunction node); the running statistics take the step
        nn.BatchNorm1d takes.  -> y, or (y, gmax, garg) with n_group > 0."""
        out = _ConvBNReLUFunction.apply(x, self.conv.weight.squeeze(2), self.bn.weight, self.bn.bias, self.bn.eps, n_group)
        _track(self.bn, out[1], out[2], x.shape[0])
        return (out[0], out[3], out[4]) if n_group else out[0]


def _track(bn, mean, var, rows, momentum=0.1):
    """nn.BatchNorm1d's update of the running statistics from one batch: the variance enters unbiased."""
    with torch.no_grad():
        bn.running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
        bn.running_var.mul_(1 - momentum).add_(var, alpha=momentum * rows / (rows - 1))
        bn.num_batches_tracked.add_(1)


class FCBNReLU(nn.Module):
    """relu(bn(linear(x))) (deepgmr.py:34-41)."""

    def __init__(self, in_planes, out_planes):
        super().__init__()
        self.linear = _Linear(in_planes, out_planes, bias=False)
        self.bn = _BN(out_planes)

    def forward(self, x):
        s, h = self.bn.folded()
        return ops.gemm(x, self.linear.weight, scale=s, shift=h, relu=True)


class TNet(nn.Module):
    """deepgmr.py:146-171: a learned rotation applied to the raw coordinates (only meaningful with use_rri False)."""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(Conv1DBNReLU(3, 64), Conv1DBNReLU(64, 128), Conv1DBNReLU(128, 256))
        self.decoder = nn.Sequential(FCBNReLU(256, 128), FCBNReLU(128, 64), _Linear(64, 6, bias=True))

    @staticmethod
    def f2R(f):
        r1 = F.normalize(f[:, :3])
        proj = (r1.unsqueeze(1) @ f[:, 3:].unsqueeze(2)).squeeze(2)
        r2 = F.normalize(f[:, 3:] - proj * r1)
        r3 = torch.cross(r1, r2, dim=1)
        return torch.stack([r1, r2, r3], dim=2)

    def forward(self, pts):
        """pts[B,N,3] rows -> [B,N,3] rows of R @ p (the 6-vector to R and the 3x3 products are a handful of tiny torch ops)."""
        B, N, _ = pts.shape
        f = self.encoder(pts.reshape(B * N, 3)).view(B, N, -1).amax(dim=1)
        R = self.f2R(self.decoder(f.contiguous()))
        return pts @ R.transpose(1, 2)


class PointNet(nn.Module):
    """deepgmr.py:174-197.  forward(x[B,N,C]) -> logits[B,N,num_groups].

    The decoder's first layer takes cat(f_loc, f_glob) in the reference, f_glob the per-cloud maximum repeated for every point.
    Here W . [f_loc; f_glob] = W_loc . f_loc + (W_glob . f_glob): the second term is one [B,1024] x [1024,512] GEMM per forward and
    enters the first as a residual whose row stride is 0 (one row per cloud), so the [B*N, 2048] concatenation is never built and
    the layer reads half the operand."""

    def __init__(self, args):
        super().__init__()
        self.use_tnet = bool(args.use_tnet)
        self.tnet = TNet() if self.use_tnet else None
        d_input = args.rri_size * 4 if args.use_rri else 3
        self.encoder = nn.Sequential(Conv1DBNReLU(d_input, 64), Conv1DBNReLU(64, 128), Conv1DBNReLU(128, 256),
                                     Conv1DBNReLU(256, 1024))
        self.decoder = nn.Sequential(Conv1DBNReLU(1024 * 2, 512), Conv1DBNReLU(512, 256), Conv1DBNReLU(256, 128),
                                     _Conv1d(128, args.num_groups, bias=True))

    def forward(self, x):
        if self.use_tnet:
            x = self.tnet(x)
        B, N, C = x.shape
        f_loc = self.encoder(x.reshape(B * N, C).contiguous())                 # [B*N, 1024]
        f_glob = f_loc.view(B, N, 1024).amax(dim=1)                            # [B, 1024]
        first = self.decoder[0]
        s, h = first.bn.folded()
        W = first.conv.weight.squeeze(2)                                        # [512, 2048]
        shift_b = ops.gemm(f_glob, W[:, 1024:], scale=s)                        # [B, 512]: scale * (W_glob . f_glob), per cloud
        y = ops.gemm(f_loc.view(B, N, 1024), W[:, :1024].unsqueeze(0).expand(B, 512, 1024), scale=s, shift=h,
                     residual=shift_b.unsqueeze(1).expand(B, N, 512), relu=True).view(B * N, 512)
        y = self.decoder[2](self.decoder[1](y))
        last = self.decoder[3]
        return ops.gemm(y, last.weight.squeeze(2), shift=last.bias).view(B, N, -1)

    def forward_train(self, x):
        """forward under batch statistics, with a graph (RRI features only).  The rows the max-pool picked stay on the module
        (``pool_rows`` [B,1024] int32, counted over all B*N rows)."""
        B, N, C = x.shape
        h = x.reshape(B * N, C).contiguous()
        for layer in self.encoder[:3]:
            h = layer.forward_train(h)
        f_loc, f_glob, self.pool_rows = self.encoder[3].forward_train(h, n_group=N)
        first = self.decoder[0]
        y, mean, var = _DecoderFirstFunction.apply(f_loc, f_glob, self.pool_rows, first.conv.weight.squeeze(2), first.bn.weight,
                                                   first.bn.bias, first.bn.eps)
        _track(first.bn, mean, var, B * N)
        y = self.decoder[2].forward_train(self.decoder[1].forward_train(y))
        last = self.decoder[3]
        return _LinearRowsFunction.apply(y, last.weight.squeeze(2), last.bias, False).view(B, N, -1)


class Model(nn.Module):
    """``Model(args).forward(pts1[B,N,3], pts2[B,M,3], T_gt=None, prefix="train")`` (deepgmr.py:200-255): T_12[B,4,4] for
    prefix == "test", else (loss, r_err, t_err, rmse, mse).  ``args``: use_rri, rri_size, num_groups, use_tnet
    (cfgs/deepgmr_mi355x.yaml).  ``trainable=True``: in train() mode the loss carries a graph to all 23 parameters and the BatchNorm
    buffers are updated (module docstring); without it, or in eval() mode, inference only.  ``nbr``: optionally the two clouds'
    neighbour lists (int32 [B,N,k], the point itself left out) for the RRI features, instead of houv_knn_cross's.  As in the
    reference, the intermediate results of the last forward stay on the module (gamma1, pi1, mu1, sigma1, ... T_12, T_21);
    sigma is the scalar [B,J] of the isotropic covariance."""

    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        if self.trainable and bool(args.use_tnet):
            raise NotImplementedError("models.deepgmr.Model(trainable=True) does not train the T-Net (use_tnet: True); the "
                                      "shipped cfg and the reference's training use the RRI features")
        self.backbone = PointNet(args)
        self.use_rri = bool(args.use_rri)
        self.k = int(args.rri_size)

    def features(self, pts, nbr=None):
        """pts[B,N,3] -> the backbone's input rows [B,N,C]: RRI features (C = 4k) or the centred coordinates (C = 3)."""
        if self.use_rri:
            if nbr is not None:
                return ops.rri_features(pts.detach(), nbr.int().contiguous(), self.k)
            return rri_rows(pts, self.k)
        return pts - pts.mean(dim=1, keepdim=True)

    def responsibilities(self, pts):
        logits = self.backbone(self.features(pts))
        return ops.softmax_rows_(logits)                                        # F.softmax(..., dim=2), in place

    def _cloud_train(self, pts, nbr):
        logits = self.backbone.forward_train(self.features(pts, nbr))
        return _GmmParamsFunction.apply(logits, pts)

    def _forward_train(self, pts1, pts2, T_gt, prefix, nbr):
        self.pts1 = pts1 = pts1.detach().contiguous().float()
        self.pts2 = pts2 = pts2.detach().contiguous().float()
        nbr = nbr if nbr is not None else (None, None)
        self.gamma1, self.pi1, self.mu1, self.sigma1 = self._cloud_train(pts1, nbr[0])
        self.pool_rows1 = self.backbone.pool_rows
        self.gamma2, self.pi2, self.mu2, self.sigma2 = self._cloud_train(pts2, nbr[1])
        self.pool_rows2 = self.backbone.pool_rows
        self.T_12 = _GmmRegisterFunction.apply(self.pi1, self.mu1, self.mu2, self.sigma2)
        if prefix == "test":
            return self.T_12
        self.T_21 = _GmmRegisterFunction.apply(self.pi2, self.mu2, self.mu1, self.sigma1)
        self.T_gt = T_gt
        eye = torch.eye(4, device=T_gt.device).expand_as(T_gt)
        self.mse1 = F.mse_loss(self.T_12 @ torch.inverse(T_gt), eye)
        self.mse2 = F.mse_loss(self.T_21 @ T_gt, eye)
        loss = self.mse1 + self.mse2
        with torch.no_grad():
            T_12 = self.T_12.detach()
            self.r_err = rotation_error(T_12[:, :3, :3], T_gt[:, :3, :3])
            self.t_err = translation_error(T_12[:, :3, 3], T_gt[:, :3, 3])
            self.rmse = rmse_loss(pts1, T_12, T_gt)
            self.mse = rotation_geodesic_error(T_12[:, :3, :3], T_gt[:, :3, :3]) + self.t_err
        return loss, self.r_err, self.t_err, self.rmse, self.mse

    def forward(self, pts1, pts2, T_gt=None, prefix="train", nbr=None):
        if self.trainable and self.training:
            return self._forward_train(pts1, pts2, T_gt, prefix, nbr)
        with torch.no_grad():
            return self._forward_eval(pts1, pts2, T_gt, prefix, nbr)

    def _forward_eval(self, pts1, pts2, T_gt, prefix, nbr):
        if nbr is not None:
            raise ValueError("nbr is an option of the training forward")
        self.pts1 = pts1 = pts1.contiguous().float()
        self.pts2 = pts2 = pts2.contiguous().float()
        self.gamma1 = self.responsibilities(pts1)
        self.pi1, self.mu1, self.sigma1 = gmm_params(self.gamma1, pts1)
        self.gamma2 = self.responsibilities(pts2)
        self.pi2, self.mu2, self.sigma2 = gmm_params(self.gamma2, pts2)
        self.T_12 = gmm_register(self.pi1, self.mu1, self.mu2, self.sigma2)
        if prefix == "test":
            return self.T_12
        self.T_21 = gmm_register(self.pi2, self.mu2, self.mu1, self.sigma1)
        self.T_gt = T_gt
        eye = torch.eye(4, device=T_gt.device).expand_as(T_gt)
        self.mse1 = F.mse_loss(self.T_12 @ torch.inverse(T_gt), eye)
        self.mse2 = F.mse_loss(self.T_21 @ T_gt, eye)
        loss = self.mse1 + self.mse2
        self.r_err = rotation_error(self.T_12[:, :3, :3], T_gt[:, :3, :3])
        self.t_err = translation_error(self.T_12[:, :3, 3], T_gt[:, :3, 3])
        self.rmse = rmse_loss(pts1, self.T_12, T_gt)
        self.mse = rotation_geodesic_error(self.T_12[:, :3, :3], T_gt[:, :3, :3]) + self.t_err
        return loss, self.r_err, self.t_err, self.rmse, self.mse
