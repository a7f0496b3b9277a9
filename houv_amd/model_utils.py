"""Hot-path slice of registration/model_utils.py: ``SVDHead`` (:213-255), ``nearest_neighbor`` (:33-37) and
``get_rri_cluster`` (:76, twin of registration/models/deepgmr.py:54-95)."""
import torch
import torch.nn as nn

from . import ops


def nearest_neighbor(src, dst):
    """src, dst [3,N] / [3,M] -> (negated squared distance of the NN, its index), model_utils.py:33-37."""
    inner = -2 * torch.matmul(src.transpose(1, 0).contiguous(), dst)
    distances = -torch.sum(src ** 2, dim=0, keepdim=True).transpose(1, 0).contiguous() - inner - torch.sum(
        dst ** 2, dim=0, keepdim=True)
    return distances.topk(k=1, dim=-1)


class SVDHead(nn.Module):
    """Kabsch rigid solve.  ``forward(src[B,3,N], src_corr[B,3,N], weights[B,1,N]|None) -> (R[B,3,3], t[B,3])``.
    The per-sample Python loop of torch.svd calls (model_utils.py:232-240) is one HIP launch: 3x3 weighted
    covariance reduction + register-resident Jacobi SVD with the reference's reflection fix."""

    def __init__(self, args=None):
        super(SVDHead, self).__init__()
        if args is not None:
            self.emb_dims = 33 if getattr(args, "use_fpfh", False) else getattr(args, "descriptor_size", 512)
        self.reflect = nn.Parameter(torch.eye(3), requires_grad=False)
        self.reflect[2, 2] = -1

    def forward(self, src, src_corr, weights=None):
        w = None if weights is None else weights.contiguous().float()
        return ops.kabsch(src.contiguous().float(), src_corr.contiguous().float(), w)


def rri_rows(pts, k):
    """pts[B,N,3] -> [B,N,4k] rotation-invariant features, channel 4*j + f (the layout houv_rri_features writes and the 1x1
    convolutions of models/deepgmr.py read as GEMM rows).  Neighbours: the k+1 nearest points of the cloud by (squared distance,
    index), first entry dropped."""
    from .mm3d_pn2 import knn_cross
    pts = pts.detach().contiguous().float()
    _, idx = knn_cross(k + 1, pts, pts)
    return ops.rri_features(pts, idx, k, skip=1)


def get_rri_cluster(cluster_pts, k):
    """cluster_pts[B,3,S,M] (M clusters of S points) -> [B,4k,S,M]: per point and neighbour j the four rotation-invariant values
    (|p|, |q_j|, angle between p and q_j, smallest positive angle from q_j's tangent-plane direction to another neighbour's), at
    channel 4*j + f.  Clusters are folded into the batch as in the reference; the result is a transposed VIEW of the kernel's
    [B*M,S,4k] (the reference returns the same values contiguous).

    Neighbour lists differ from the reference's in rounding only: it ranks the expanded form -|a|^2 + 2ab - |b|^2 with
    ``topk`` and drops the first entry, here houv_knn_cross ranks the direct form fma(dz,dz,fma(dy,dy,dx*dx)), equal distances
    lower index first, and the first entry is dropped the same way (DESIGN.md sections 9.3, 9.7).  Near-ties at the k-th place
    may pick another neighbour; with exactly duplicated points the dropped entry may be the duplicate instead of the point
    itself, which gives the same features.  The whole computation stays on the device (the reference builds the [B*S,k,k,3]
    cross products in NumPy on the host)."""
    B, C, S, M = cluster_pts.shape
    if C != 3:
        raise ops._lib.HouvHipError("get_rri_cluster: expected cluster_pts[B,3,S,M]")
    pts = cluster_pts.permute(0, 3, 2, 1).reshape(B * M, S, 3)
    return rri_rows(pts, k).view(B, M, S, 4 * k).transpose(1, 3)
