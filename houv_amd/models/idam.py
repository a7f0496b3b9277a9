"""Mirror of registration/models/idam.py (`Model`, :191-358): IDAM -- a five-layer graph network over 12 nearest neighbours
(:115-149), a significance head that keeps N // 6 points of each cloud (:229-258), and `num_iters` rounds of similarity matrix ->
correspondence -> weighted Kabsch (:267-342) -- as an INFERENCE pipeline over the gfx950 kernels of include/houv_hip.h:
houv_knn_cross, houv_edge_diff, houv_gemm_f32 with the folded-BatchNorm/ReLU epilogue for every 1x1 convolution,
houv_max_over_k, houv_idam_simmat (one call per round: no [B, ., M, M] tensor is ever built) and houv_kabsch.  Nothing goes
through the host: the reference drops to NumPy for the kept indices (:245-248) and gathers by fancy indexing.

The module tree and parameter names equal the reference's (its spelling `propogate1..5` included), so a reference checkpoint's
``net_state_dict`` loads with ``load_state_dict`` unchanged (the repository ships no trained weights: tests use seeded ones).
BatchNorm runs in eval mode.  Activations are point-major rows [B*N, C] throughout (the reference keeps [B, C, N]).  The
training-time sampling branch (`batch_choice`, the three losses) and the FPFH branch (Open3D) are not built."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..mm3d_pn2 import knn_cross
from ..train_utils import rmse_loss, rotation_error, rotation_geodesic_error, rt_to_transformation, translation_error
from .dcp import _BN

K_NN = 12


def knn_idx(cloud):
    """cloud[B,N,3] -> idx[B,N,12] int32, nearest first, the point itself included (knn, idam.py:28-34)."""
    return knn_cross(K_NN, cloud, cloud)[1]


class _Conv(nn.Module):
    """Parameter holder with nn.Conv1d's / nn.Conv2d's names and shapes for a 1x1 kernel (`tail` = (1,) or (1, 1))."""

    def __init__(self, n_in, n_out, tail, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty((n_out, n_in) + tail).uniform_(-1, 1) / n_in ** 0.5)
        if bias:
            self.bias = nn.Parameter(torch.zeros(n_out))

    def matrix(self):
        return self.weight.view(self.weight.shape[0], self.weight.shape[1])

    def forward(self, x):
        return ops.gemm(x, self.matrix(), shift=self.bias)


class _ConvBNReLU(nn.Module):
    tail = (1,)

    def __init__(self, in_channel, out_channel, ksize=1):
        super().__init__()
        assert ksize == 1
        self.conv = _Conv(in_channel, out_channel, self.tail, bias=False)
        self.bn = _BN(out_channel)
        self.relu = nn.ReLU()

    def forward(self, x):
        """relu(bn(conv1x1(x))) on rows x[R, C_in] -> [R, C_out]: one GEMM, BatchNorm and ReLU in its epilogue."""
        s, h = self.bn.folded()
        return ops.gemm(x, self.conv.matrix(), scale=s, shift=h, relu=True)


class _ConvBlock(nn.Module):
    layer = _ConvBNReLU

    def __init__(self, channels, ksize=1):
        super().__init__()
        self.conv = nn.ModuleList()
        for i in range(len(channels) - 2):
            self.conv.append(self.layer(channels[i], channels[i + 1], ksize))
        self.conv.append(_Conv(channels[-2], channels[-1], self.layer.tail, bias=True))

    def forward(self, x):
        for conv in self.conv:
            x = conv(x)
        return x


class Conv1DBNReLU(_ConvBNReLU):
    """idam.py:59-70."""


class Conv1DBlock(_ConvBlock):
    """idam.py:73-84, on rows."""
    layer = Conv1DBNReLU


class Conv2DBNReLU(_ConvBNReLU):
    """idam.py:87-98 (a 1x1 Conv2d is the same GEMM on rows; the weight keeps its [out, in, 1, 1] shape)."""
    tail = (1, 1)


class Conv2DBlock(_ConvBlock):
    """idam.py:101-112, on rows."""
    layer = Conv2DBNReLU


class Propagate(nn.Module):
    """idam.py:115-128 on rows: edge differences -> GEMM (+BN+ReLU) -> GEMM -> max over the k neighbours -> GEMM.  The
    reference's order subtract-then-convolve is kept (convolving first cancels badly on the 3-channel layer); the second
    convolution's bias is added after the maximum, which commutes with a per-channel constant."""

    def __init__(self, in_channel, emb_dims):
        super().__init__()
        self.conv2d = Conv2DBlock((in_channel, emb_dims, emb_dims), 1)
        self.conv1d = Conv1DBlock((emb_dims, emb_dims), 1)

    def forward(self, x, idx):
        """x[B,N,C] rows, idx[B,N,k] int32 -> [B,N,emb_dims]."""
        B, N, C = x.shape
        k = idx.shape[2]
        ldo = (C + 3) // 4 * 4                                                  # a 3-channel input gets an aligned row stride
        d = ops.edge_diff(x, idx, k, ldo)                                       # [B*N*k, ldo], zero padding columns
        first, second = self.conv2d.conv
        W = first.conv.matrix()
        if ldo != C:
            W = F.pad(W, (0, ldo - C))
        s, h = first.bn.folded()
        a = ops.gemm(ops.gemm(d, W, scale=s, shift=h, relu=True), second.matrix())
        m = torch.empty((B * N, a.shape[1]), dtype=torch.float32, device=x.device)
        ops.max_over_k(a, k, m, 0)
        m += second.bias
        return self.conv1d(m).view(B, N, -1)


class GNN(nn.Module):
    """idam.py:131-149."""

    def __init__(self, emb_dims=64):
        super().__init__()
        self.propogate1 = Propagate(3, 64)
        self.propogate2 = Propagate(64, 64)
        self.propogate3 = Propagate(64, 64)
        self.propogate4 = Propagate(64, 64)
        self.propogate5 = Propagate(64, emb_dims)

    def forward(self, x, nn_idx=None):
        """x[B,N,3] rows -> [B,N,emb_dims]."""
        if nn_idx is None:
            nn_idx = knn_idx(x)
        for p in (self.propogate1, self.propogate2, self.propogate3, self.propogate4, self.propogate5):
            x = p(x, nn_idx)
        return x


class SVDHead(nn.Module):
    """idam.py:152-188: the weighted Kabsch solve with unweighted centring, which is houv_kabsch."""

    def __init__(self, args):
        super().__init__()
        self.emb_dims = args.descriptor_size
        reflect = torch.eye(3)
        reflect[2, 2] = -1
        self.reflect = nn.Parameter(reflect, requires_grad=False)

    def forward(self, src, src_corr, weights):
        """src, src_corr [B,3,M], weights [B,1,M] -> R[B,3,3], t[B,3]."""
        return ops.kabsch(src.contiguous(), src_corr.contiguous(), weights.contiguous())


class Model(nn.Module):
    """``Model(args).forward(src[B,N,3], tgt[B,N,3], T_gt=None, prefix="train")`` (idam.py:191-358): T[B,4,4] when T_gt is None,
    else (loss, r_err, t_err, rmse, mse) with loss = 0 (inference only: no sampling branch, no losses).  ``args``:
    descriptor_size, num_iters, use_fpfh (cfgs/idam_mi355x.yaml).  The last forward's intermediates stay on the module
    (src_idx, tgt_idx, the kept points and embeddings `kept`, and per iteration the source on entry / corr_idx / weights / R / t in `self.iters`)."""

    def __init__(self, args):
        super().__init__()
        if getattr(args, "use_fpfh", False):
            raise NotImplementedError("IDAM's FPFH branch (use_fpfh: True) needs Open3D and is not built; use the GNN embedding")
        self.emb_dims = int(args.descriptor_size)
        self.num_iter = int(args.num_iters)
        self.emb_nn = GNN(self.emb_dims)
        self.significance_fc = Conv1DBlock((self.emb_dims, 64, 32, 1), 1)
        self.sim_mat_conv1 = nn.ModuleList([Conv2DBlock((self.emb_dims * 2 + 4, 32, 32), 1) for _ in range(self.num_iter)])
        self.sim_mat_conv2 = nn.ModuleList([Conv2DBlock((32, 32, 1), 1) for _ in range(self.num_iter)])
        self.weight_fc = nn.ModuleList([Conv1DBlock((32, 32, 1), 1) for _ in range(self.num_iter)])
        self.head = SVDHead(args=args)

    def simmat_params(self, i):
        """The ten parameter tensors of houv_idam_simmat for iteration i, BatchNorm folded."""
        a, b = self.sim_mat_conv1[i].conv, self.sim_mat_conv2[i].conv
        s1, t1 = a[0].bn.folded()
        s3, t3 = b[0].bn.folded()
        return (a[0].conv.matrix(), s1, t1, a[1].matrix(), a[1].bias, b[0].conv.matrix(), s3, t3, b[1].weight.view(32),
                b[1].bias)

    def embed(self, cloud):
        """cloud[B,N,3] -> (embedding[B,N,E], significance[B,N])."""
        B, N, _ = cloud.shape
        emb = self.emb_nn(cloud)
        return emb, self.significance_fc(emb.view(B * N, -1)).view(B, N)

    @torch.no_grad()
    def forward(self, src, tgt, T_gt=None, prefix="train"):
        self.pts = src = src.contiguous().float()
        tgt = tgt.contiguous().float()
        B, N, _ = src.shape
        tgt_emb, tgt_sig = self.embed(tgt)
        src_emb, src_sig = self.embed(src)
        M = N // 6                                                              # hard point elimination, on the device
        self.src_idx = src_sig.topk(k=M, dim=-1)[1]
        self.tgt_idx = tgt_sig.topk(k=M, dim=-1)[1]
        take = lambda t, i: torch.gather(t, 1, i.unsqueeze(-1).expand(-1, -1, t.shape[2])).contiguous()
        src, es = take(src, self.src_idx), take(src_emb, self.src_idx)
        tgt, et = take(tgt, self.tgt_idx), take(tgt_emb, self.tgt_idx)
        self.kept = (src, tgt, es, et)
        R = torch.eye(3, device=src.device).expand(B, 3, 3)
        t = torch.zeros(B, 3, device=src.device)
        self.iters = []
        for i in range(self.num_iter):
            src_in = src
            rowmax, corr_idx, corr, _ = ops.idam_simmat(src, tgt, es, et, *self.simmat_params(i))
            w = torch.sigmoid(self.weight_fc[i](rowmax.view(B * M, 32)).view(B, M))
            w = w * (w >= w.median(-1, keepdim=True)[0]).float()                # torch.median: the LOWER median for even M
            w = w / (w.sum(-1, keepdim=True) + 1e-8)
            R_i, t_i = self.head(src.transpose(1, 2), corr, w.unsqueeze(1))
            src = (src @ R_i.transpose(1, 2) + t_i.unsqueeze(1)).contiguous()
            R = R_i @ R
            t = (R_i @ t.unsqueeze(-1)).squeeze(-1) + t_i
            self.iters.append(dict(src=src_in, corr_idx=corr_idx, weights=w, R=R_i, t=t_i))
        self.T = rt_to_transformation(R, t.unsqueeze(-1))
        if T_gt is None:
            return self.T
        R_gt, t_gt = T_gt[:, :3, :3], T_gt[:, :3, 3]
        mse = rotation_geodesic_error(R, R_gt) + translation_error(t, t_gt)
        loss = torch.zeros((), device=src.device)
        return loss, rotation_error(R, R_gt), translation_error(t, t_gt), rmse_loss(self.pts, self.T, T_gt), mse

    def get_transform(self):
        return self.T
