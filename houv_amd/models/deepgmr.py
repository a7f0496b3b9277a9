"""Mirror of registration/models/deepgmr.py (`Model`, :200-255): DeepGMR -- rotation-invariant RRI features (:54-95), a
PointNet that turns each point into responsibilities over J Gaussians (:174-197), the mixture parameters of both clouds (:98-120)
and the closed-form pose between the two mixtures (:123-143) -- as an INFERENCE pipeline over the gfx950 kernels of
include/houv_hip.h: houv_knn_cross + houv_rri_features, houv_gemm_f32 with the folded-BatchNorm/ReLU epilogue for every 1x1
convolution, houv_softmax_rows, houv_gmm_params, houv_gmm_register.  Nothing goes through the host: the reference copies the
tangent vectors to NumPy for the features and runs the 3x3 SVD on the CPU.

The module tree and parameter names equal the reference's, so a reference checkpoint's ``net_state_dict`` loads with
``load_state_dict`` unchanged (the repository ships no trained weights: tests use seeded random ones).  BatchNorm runs in eval
mode (running statistics).  Activations are point-major rows [B*N, C] throughout (the reference keeps [B, C, N])."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..model_utils import get_rri_cluster, rri_rows  # noqa: F401  (get_rri_cluster: the reference's module-level name)
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


class Model(nn.Module):
    """``Model(args).forward(pts1[B,N,3], pts2[B,M,3], T_gt=None, prefix="train")`` (deepgmr.py:200-255): T_12[B,4,4] for
    prefix == "test", else (loss, r_err, t_err, rmse, mse).  ``args``: use_rri, rri_size, num_groups, use_tnet
    (cfgs/deepgmr_mi355x.yaml).  Inference only.  As in the reference, the intermediate results of the last forward stay on the
    module (gamma1, pi1, mu1, sigma1, ... T_12, T_21); sigma is the scalar [B,J] of the isotropic covariance."""

    def __init__(self, args):
        super().__init__()
        self.backbone = PointNet(args)
        self.use_rri = bool(args.use_rri)
        self.k = int(args.rri_size)

    def features(self, pts):
        """pts[B,N,3] -> the backbone's input rows [B,N,C]: RRI features (C = 4k) or the centred coordinates (C = 3)."""
        if self.use_rri:
            return rri_rows(pts, self.k)
        return pts - pts.mean(dim=1, keepdim=True)

    def responsibilities(self, pts):
        logits = self.backbone(self.features(pts))
        return ops.softmax_rows_(logits)                                        # F.softmax(..., dim=2), in place

    @torch.no_grad()
    def forward(self, pts1, pts2, T_gt=None, prefix="train"):
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
