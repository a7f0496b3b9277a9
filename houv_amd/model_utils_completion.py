"""Loss glue on top of ``metrics.cd`` and ``metrics.emd``: the hot-path slice of registration/model_utils_completion.py
(calc_cd :69-80, calc_cd_percent :83-100, calc_cd_percent_aligned :103-117, loss_view :157-166, calc_emd :170-175).
These are the un-fused, differentiable forms (one Chamfer launch + torch.topk each); the optimisation
loop itself never calls them -- it runs inside houv_solve_iterate.
Below them, the sampling / regularisation helpers of the same file that sit on the mm3d_pn2 point ops
(edge_preserve_sampling :178-204, get_repulsion_loss :278-297, get_uniform_loss :300-330, knn :346-351, knn_point :354-365,
symmetric_sample :383-392, three_nn_upsampling :395-402), with the reference's signatures and return tuples, and the folding
grids of the completion decoders (gen_grid :223-227, gen_1d_grid :230-233, gen_grid_up :236-249; pure torch, on the CPU)."""
import math

import torch

from . import _lib, ops
from .metrics import cd, emd
from .mm3d_pn2 import (ball_query, furthest_point_sample, gather_points, grouping_operation, knn_cross, three_nn)


def _f1(dist1, dist2, threshold=0.0001):
    """F-score of two clouds from their SQUARED nearest-neighbour distances (utils/metrics/CD/fscore.py:3-16): the harmonic mean of
    the two fractions of points closer than `threshold`; 0 where both fractions are 0."""
    near1 = (dist1 < threshold).to(dist1.dtype).mean(dim=1)
    near2 = (dist2 < threshold).to(dist2.dtype).mean(dim=1)
    both = near1 + near2
    return torch.where(both > 0, 2 * near1 * near2 / both.clamp_min(torch.finfo(dist1.dtype).tiny), torch.zeros_like(both))


def calc_cd(output, gt, calc_f1=False):
    dist1, dist2, _, _ = cd()(gt, output)
    cd_p = (torch.sqrt(dist1).mean(1) + torch.sqrt(dist2).mean(1)) / 2
    cd_t = dist1.mean(1) + dist2.mean(1)
    return (cd_p, cd_t, _f1(dist1, dist2)) if calc_f1 else (cd_p, cd_t)


def calc_cd_percent(output, gt, calc_f1=False, percent=1):
    k = int(output.shape[1] * percent)
    dist1, dist2, _, _ = cd()(gt, output)
    dist1, _ = dist1.topk(k, dim=1, largest=False, sorted=True)
    dist2, _ = dist2.topk(k, dim=1, largest=False, sorted=True)
    cd_p, cd_t = torch.sqrt(dist1).mean(1), torch.sqrt(dist2).mean(1)
    return (cd_p, cd_t, _f1(dist1, dist2)) if calc_f1 else (cd_p, cd_t)      # the F-score of the KEPT distances, as :96-98 has it


def calc_cd_percent_aligned(output, gt, percent=1):
    k = int(output.shape[1] * percent)
    dist1, dist2, idx1, idx2 = cd()(gt, output)
    dist1, idxx1 = dist1.topk(k, dim=1, largest=False, sorted=True)
    dist2, idxx2 = dist2.topk(k, dim=1, largest=False, sorted=True)
    return torch.sqrt(dist1).mean(1), torch.sqrt(dist2).mean(1), idx1, idx2, idxx1, idxx2


def loss_view(src, tgt, dim=0, percent=1):
    keep = torch.ones((1, 1, 3), dtype=src.dtype, device=src.device)
    keep[:, :, dim] = 0
    return calc_cd_percent(src * keep, tgt * keep, percent=percent)


def calc_emd(output, gt, eps=0.005, iterations=50):
    """Mean EMD point distance per cloud: sqrt of the auction's squared distances, averaged (:170-175)."""
    dist, _ = emd()(output, gt, eps, iterations)
    return torch.sqrt(dist).mean(1)


def gen_grid(num_grid_point):
    """[2, n*n]: the flat (x, y) pairs of an n x n mesh over [-0.05, 0.05], VIEWED as two rows (so a row interleaves x and y)."""
    x = torch.linspace(-0.05, 0.05, steps=num_grid_point)
    x, y = torch.meshgrid(x, x, indexing="ij")
    return torch.stack([x, y], dim=-1).view(2, num_grid_point ** 2)


def gen_1d_grid(num_grid_point):
    return torch.linspace(-0.05, 0.05, num_grid_point).view(1, num_grid_point)


def gen_grid_up(up_ratio, grid_size=0.2):
    """[2, up_ratio]: row 0 the x and row 1 the y of a num_x x num_y mesh over [-grid_size, grid_size], num_x the largest divisor
    of up_ratio that is <= int(sqrt(up_ratio)) + 1."""
    sqrted = int(math.sqrt(up_ratio)) + 1
    for i in range(sqrted, 0, -1):
        if up_ratio % i == 0:
            num_x, num_y = i, up_ratio // i
            break
    grid_x = torch.linspace(-grid_size, grid_size, steps=num_x)
    grid_y = torch.linspace(-grid_size, grid_size, steps=num_y)
    x, y = torch.meshgrid(grid_x, grid_y, indexing="ij")
    return torch.stack([x, y], dim=-1).view(-1, 2).transpose(0, 1).contiguous()


def knn_point(pk, point_input, point_output):
    """The pk nearest points of point_input (B,n,3) for every point of point_output (B,m,3): (-squared distance (B,m,pk),
    index (B,m,pk) int64), nearest first.  The reference ranks the expanded form -|a|^2 + 2ab - |b|^2 with torch.topk; here
    houv_knn_cross ranks the direct form fma(dz,dz,fma(dy,dy,dx*dx)), which differs from it in rounding (and so in the order of
    near-ties); equal distances keep the lower index first.  No gradient flows through the distances."""
    d2, idx = knn_cross(pk, point_output, point_input)
    return -d2, idx.long()


def knn(x, k):
    """x (B,3,N) -> (B,N,k) int64 indices of each point's k nearest points, itself first.  houv_knn serves k = 1, 3, 8, 16, 20;
    any other k <= 32 goes through houv_knn_cross of the cloud with itself."""
    _lib.require_gpu(x)
    if x.dim() != 3 or x.shape[1] != 3:
        raise _lib.HouvHipError("knn: expected x[B,3,N] (only 3-D coordinates have a kernel)")
    pts = x.detach().transpose(1, 2).contiguous().float()
    if k in (1, 3, 8, 16, 20) and k <= pts.shape[1]:
        return ops.knn(pts, k).long()
    return knn_cross(k, pts, pts)[1].long()


def edge_preserve_sampling(feature_input, point_input, num_samples, k=10):
    """Furthest-point-sample num_samples centres of point_input (B,N,3) and give each the channel-wise maximum of feature_input
    (B,C,N) over its min(k,N) nearest points, stacked under the centre's own features -> (net (B,2C,num_samples),
    p_idx (B,num_samples) int32, pn_idx (B,num_samples,pk) int32, point_output (B,num_samples,3))."""
    _lib.require_gpu(feature_input, point_input)
    B, C, N = feature_input.shape
    p_idx = furthest_point_sample(point_input, num_samples)
    point_output = gather_points(point_input.transpose(1, 2).contiguous(), p_idx).transpose(1, 2).contiguous()
    pk = int(min(k, N))
    _, pn_idx = knn_point(pk, point_input, point_output)
    pn_idx = pn_idx.int()
    neighbours = gather_points(feature_input, pn_idx.view(B, num_samples * pk)).view(B, C, num_samples, pk)
    neighbour_feature = neighbours.max(dim=3).values
    center_feature = grouping_operation(feature_input, p_idx.unsqueeze(2)).view(B, -1, num_samples)
    return torch.cat((center_feature, neighbour_feature), 1), p_idx, pn_idx, point_output


def get_repulsion_loss(pred, nsample=20, radius=0.07):
    """Repulsion loss of pred (B,N,3): over each point's 4 nearest other points among its nsample nearest,
    mean(radius - d * exp(-d^2 / h^2)) with h = 0.03 and d^2 clamped at 1e-12."""
    _lib.require_gpu(pred)
    flipped = pred.transpose(1, 2).contiguous()
    idx = knn(flipped, nsample).int()
    offsets = grouping_operation(flipped, idx) - flipped.unsqueeze(-1)          # (B,3,N,nsample)
    d2 = (offsets ** 2).sum(dim=1)
    d2 = -torch.topk(-d2, 5).values[:, :, 1:]                                     # drop the point itself
    d2 = d2.clamp_min(1e-12)
    h = 0.03
    return torch.mean(radius - torch.sqrt(d2) * torch.exp(-d2 / h ** 2))


def get_uniform_loss(pcd, percentages=(0.004, 0.006, 0.008, 0.010, 0.012), radius=1.0):
    """Uniformity loss of pcd (B,N,3): for each percentage p, balls of radius sqrt(p*radius) around int(0.05 N) furthest-point
    samples hold int(N p) slots; inside each ball every point's distance to its nearest other point is compared with the spacing
    of a uniform disk, sqrt(pi radius^2 p / nsample): mean((d - e)^2 / (e + 1e-8)) * (100 p)^2, averaged over the percentages."""
    _lib.require_gpu(pcd)
    B, N, _ = pcd.shape
    npoint = int(N * 0.05)
    flipped = pcd.transpose(1, 2).contiguous()
    loss = 0
    for p in percentages:
        nsample = int(N * p)
        r = math.sqrt(p * radius)
        expect_len = math.sqrt(math.pi * (radius ** 2) * p / nsample)
        new_xyz = gather_points(flipped, furthest_point_sample(pcd, npoint)).transpose(1, 2).contiguous()
        idx = ball_query(0, r, nsample, pcd, new_xyz)
        grouped = grouping_operation(flipped, idx).permute(0, 2, 3, 1).contiguous().view(-1, nsample, 3)
        # the distances must carry the gradient, so they are recomputed from the gathered neighbours (knn_point's are detached)
        _, nn_idx = knn_point(2, grouped, grouped)
        other = torch.gather(grouped, 1, nn_idx[:, :, 1:].expand(-1, -1, 3))
        d2 = ((grouped - other) ** 2).sum(dim=2, keepdim=True)
        d = torch.sqrt(torch.abs(d2 + 1e-8)).mean(dim=-1)
        loss = loss + torch.mean((d - expect_len) ** 2 / (expect_len + 1e-8)) * math.pow(p * 100, 2)
    return loss / len(percentages)


def symmetric_sample(points, num=512):
    """Furthest-point-sample num points of points (B,N,3) and append their mirror images in the z = 0 plane -> (B,2*num,3)."""
    idx = furthest_point_sample(points, num)
    kept = gather_points(points.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    mirrored = kept * kept.new_tensor([1.0, 1.0, -1.0])
    return torch.cat([kept, mirrored], dim=1)


def three_nn_upsampling(target_points, source_points):
    """Inverse-distance weights of the three nearest source points of every target point: (idx (B,N,3) int32, weight (B,N,3)),
    the weights 1/max(d, 1e-10) normalised to sum 1 -- the arguments three_interpolate takes."""
    dist, idx = three_nn(target_points, source_points)
    inv = 1.0 / dist.clamp_min(1e-10)
    return idx, inv / inv.sum(dim=2, keepdim=True)
