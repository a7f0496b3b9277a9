"""Loss glue on top of ``metrics.cd`` and ``metrics.emd``: the hot-path slice of registration/model_utils_completion.py
(calc_cd :69-80, calc_cd_percent :83-100, calc_cd_percent_aligned :103-117, loss_view :157-166, calc_emd :170-175).
These are the un-fused, differentiable forms (one Chamfer launch + torch.topk each); the optimisation
loop itself never calls them -- it runs inside houv_solve_iterate.
Below them, the sampling / regularisation helpers of the same file that sit on the mm3d_pn2 point ops
(edge_preserve_sampling :178-204, get_repulsion_loss :278-297, get_uniform_loss :300-330, knn :346-351, knn_point :354-365,
symmetric_sample :383-392, three_nn_upsampling :395-402), with the reference's signatures and return tuples, and the folding
grids of the completion decoders (gen_grid :223-227, gen_1d_grid :230-233, gen_grid_up :236-249; pure torch, on the CPU).
From completion/model_utils.py, for the ECG network (houv_amd/models/ecg.py): knn on features of up
to 256 channels (houv_knn_feat), get_graph_feature :164-187, get_edge_features :119-132 and EF_expansion :24-55."""
import math

import torch
import torch.nn as nn

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


class _CdLossFunction(torch.autograd.Function):
    """calc_cd(output, gt) as ONE autograd node.  forward: calc_cd's own operations -- the Chamfer
    launch, then the same torch sqrt, mean and / 2 -- so cd_p and cd_t carry its bits.  backward: one ops.cd_loss_backward, the
    ordered sums of houv_cd_loss_backward (no float atomics, no zeroed buffer, no [B,N] / [B,M] gradient of the distances).
    Saved: output, gt, dist1, dist2, idx1, idx2.  gt gets no gradient."""

    @staticmethod
    def forward(ctx, output, gt):
        output, gt = output.contiguous(), gt.contiguous()
        B, M, _ = output.shape
        N = gt.shape[1]
        dev = output.device
        dist1 = torch.empty((B, N), dtype=torch.float32, device=dev)
        dist2 = torch.empty((B, M), dtype=torch.float32, device=dev)
        idx1 = torch.empty((B, N), dtype=torch.int32, device=dev)
        idx2 = torch.empty((B, M), dtype=torch.int32, device=dev)
        ops.chamfer_forward(gt, output, dist1, dist2, idx1, idx2)
        cd_p = (torch.sqrt(dist1).mean(1) + torch.sqrt(dist2).mean(1)) / 2
        cd_t = dist1.mean(1) + dist2.mean(1)
        ctx.save_for_backward(output, gt, dist1, dist2, idx1, idx2)
        return cd_p, cd_t

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_p, g_t):
        return ops.cd_loss_backward(*ctx.saved_tensors, g_p.contiguous(), g_t.contiguous()), None


def cd_loss(output, gt):
    """(cd_p[B], cd_t[B]) of calc_cd(output[B,M,3], gt[B,N,3]), bit for bit, as one autograd node whose gradient with respect to
    `output` is summed in a fixed order: two backward passes over the same values give the same bits (calc_cd's go through
    float atomics).  The gradient with respect to the ground truth is not built: a gt that requires one is refused."""
    if gt.requires_grad:
        raise ValueError("cd_loss: the gradient with respect to the ground truth is not built (gt.requires_grad)")
    return _CdLossFunction.apply(output, gt)


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
    """x (B,C,N) -> (B,N,k) int64 indices of each point's k nearest points, itself first.  C = 3: houv_knn serves k = 1, 3, 8, 16,
    20; any other k <= 32 goes through houv_knn_cross of the cloud with itself.  Any other C <= 256 (features): houv_knn_feat,
    which ranks the direct form d = fma(t, t, d), t = x_j[c] - x_i[c], c ascending, the lower index first among equal distances;
    the reference ranks the expanded form -|a|^2 + 2ab - |b|^2 with torch.topk and differs at near-ties."""
    _lib.require_gpu(x)
    if x.dim() != 3 or not 1 <= x.shape[1] <= 256:
        raise _lib.HouvHipError("knn: expected x[B,C,N] with 1 <= C <= 256")
    pts = x.detach().transpose(1, 2).contiguous().float()
    if x.shape[1] != 3:
        return ops.knn_feat(pts, k).long()
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


def _transposed(a):
    """a[m,n] -> a fresh, densely packed [n,m].  Not ``a.t().contiguous()``: with m == 1 torch already calls the transposed view
    contiguous and returns it as it is, with a last stride of n, which the GEMM (unit last stride) refuses -- a batch of one
    cloud would not train."""
    out = torch.empty((a.shape[1], a.shape[0]), dtype=a.dtype, device=a.device)
    out.copy_(a.t())
    return out


class _LinearFunction(torch.autograd.Function):
    """relu?(x W^T + b) over ops.gemm, with its backward over ops.gemm: gx = gz W, gW = gz^T x, gb = sum gz, gz = gy * [y > 0].
    x[M,K] and W[N,K] may be column slices of wider row-major buffers (a weight's columns: its gradient then returns through
    the slice); b may be None.  Shared by the trainable paths of models/pcn.py and models/ecg.py."""

    @staticmethod
    def forward(ctx, x, W, b, relu):
        y = ops.gemm(x, W, shift=b, relu=relu)
        ctx.relu, ctx.bias = relu, b is not None
        ctx.save_for_backward(x, W, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, W, y = ctx.saved_tensors
        gz = (gy * (y > 0)).contiguous() if ctx.relu else gy.contiguous()
        return ops.gemm(gz, W, trans_b=False), ops.gemm(_transposed(gz), _transposed(x)), gz.sum(0) if ctx.bias else None, None


class _LinearRowsFunction(_LinearFunction):
    """_LinearFunction for layers applied to every point of a batch (models/ecg.py): the same forward; the weight gradient's
    sum over the rows is split into chunks (_weight_grad) and gx is left out when x needs none."""

    @staticmethod
    def backward(ctx, gy):
        x, W, y = ctx.saved_tensors
        gz = (gy * (y > 0)).contiguous() if ctx.relu else gy.contiguous()
        gx = ops.gemm(gz, W, trans_b=False) if ctx.needs_input_grad[0] else None
        return gx, _weight_grad(gz, x), gz.sum(0) if ctx.bias else None, None


def _weight_grad(gz, x):
    """gz[M,N]^T x[M,K] -> [N,K].  The output is small and the reduction runs over the M rows: with many rows (every point of a
    batch) one GEMM would keep a handful of workgroups busy for the whole sum, so the rows are split into S equal chunks (a
    power of two, chunks of at least 512 rows), one batched GEMM writes S partial products, and they are added in chunk order.
    A fixed shape gives a fixed order: the same bits from call to call.  Few rows: one GEMM."""
    gzT, xT = _transposed(gz), _transposed(x)
    M = gz.shape[0]
    S = 1
    while S < 64 and M % (2 * S) == 0 and M // (2 * S) >= 512:
        S *= 2
    if S == 1:
        return ops.gemm(gzT, xT)
    Mc = M // S
    part = ops.gemm(gzT.view(-1, S, Mc).transpose(0, 1), xT.view(-1, S, Mc).transpose(0, 1))      # [S,N,K]
    return part.sum(0)


class _RowGather(torch.autograd.Function):
    """_take_rows with an ordered gradient: rows (B,N,C), idx (B,...) int -> (B,...,C) = rows[b, idx[b,...]].  The backward is
    houv_scatter_points_grad's sum in ascending order of the flattened idx (no float atomics, unlike torch.gather's)."""

    @staticmethod
    def forward(ctx, rows, idx):
        ctx.save_for_backward(idx)
        ctx.N = rows.shape[1]
        return _take_rows(rows, idx)

    @staticmethod
    def backward(ctx, grad):
        from .mm3d_pn2 import _scatter_grad
        idx, = ctx.saved_tensors
        B, C = grad.shape[0], grad.shape[-1]
        g = _transposed_batch(grad.reshape(B, -1, C))
        return _transposed_batch(_scatter_grad(g, idx.reshape(B, -1).int().contiguous(), None, ctx.N, 1)), None


def _transposed_batch(a):
    """a[B,m,n] -> a fresh, densely packed [B,n,m] (see _transposed for why not .transpose().contiguous())."""
    out = torch.empty((a.shape[0], a.shape[2], a.shape[1]), dtype=a.dtype, device=a.device)
    out.copy_(a.transpose(1, 2))
    return out


def _take_rows(rows, idx):
    """rows (B,N,C) (any row stride), idx (B,...) -> (B,...,C) = rows[b, idx[b,...]]."""
    B, _, C = rows.shape
    flat = idx.reshape(B, -1, 1).long().expand(-1, -1, C)
    return torch.gather(rows, 1, flat).view(*idx.shape, C)


def get_edge_features(x, idx):
    """x (B,C,1,N) or (B,C,N), idx (B,N,k) -> (B,C,k,N): the features of every point's listed neighbours (model_utils.py:119-132)."""
    if x.dim() == 4:
        x = x.squeeze(2)
    return _take_rows(x.transpose(1, 2), idx).permute(0, 3, 2, 1)


def get_graph_feature(x, k=20, minus_center=True, idx=None):
    """x (B,C,N) -> (B,2C,N,k): cat(x_i, x_j - x_i) (minus_center) or cat(x_i, x_j) over each point's k nearest points in feature
    space, itself first (model_utils.py:164-187).  This is the reference's materialised layout, for callers that want it;
    Dense_conv does not build it (houv_dense_conv).  `idx` (B,N,k), when given, replaces the search."""
    if idx is None:
        idx = knn(x, k)
    rows = x.transpose(1, 2)
    feature = _take_rows(rows, idx)                                               # (B,N,k,C)
    centre = rows.unsqueeze(2).expand_as(feature)
    return torch.cat((centre, feature - centre if minus_center else feature), dim=3).permute(0, 3, 1, 2)


class Conv1x1(nn.Module):
    """Parameter holder with the names, shapes and default initialisation of nn.Conv1d (dims = 1: weight [out, in, 1]) or
    nn.Conv2d (dims = 2: [out, in, 1, 1]) for a kernel of size 1: the product itself runs on houv_gemm_f32 or inside a fused
    kernel."""

    def __init__(self, n_in, n_out, dims=1):
        super().__init__()
        bound = 1 / math.sqrt(n_in)
        self.weight = nn.Parameter(torch.empty((n_out, n_in) + (1,) * dims).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.empty(n_out).uniform_(-bound, bound))

    def matrix(self):
        return self.weight.view(self.weight.shape[0], self.weight.shape[1])

    def rows(self, x, relu=False, out=None, lo=0, hi=None):
        """x (..., hi - lo) rows (one row stride) -> relu?(x . matrix()[:, lo:hi]^T + bias), written to `out` when given."""
        W = self.matrix()[:, lo:hi]
        y = ops.gemm(x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x.view(-1, x.shape[-1]), W,
                     None if out is None else out.view(-1, out.shape[-1]), shift=self.bias, relu=relu)
        return y.view(*x.shape[:-1], W.shape[0]) if out is None else out


class _EFExpandFunction(torch.autograd.Function):
    """EF_expansion past its per-point projections as one autograd node (houv_ef_expand / houv_ef_expand_backward; DESIGN.md
    section 9.16): proj (B,N,2O+2Or) = [U | V | P | Q], idx (B,N,k) int32 (a constant: no gradient), W2a (O r, O) (a column
    slice of conv2's weight: its gradient returns through the slice), W3 (O,O), b3 (O) -> (B, N r, O).  Saved: proj, idx, the
    int8 arg of the maxima and the two matrices; nothing of extent (B,k,N,.) is kept."""

    @staticmethod
    def forward(ctx, proj, idx, W2a, W3, b3, r):
        out, arg = ops.ef_expand(proj, idx, W2a, W3, b3, r, want_arg=True)
        ctx.r = r
        ctx.save_for_backward(proj, idx, arg, W2a, W3)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, gout, _garg):
        proj, idx, arg, W2a, W3 = ctx.saved_tensors
        g = ops.ef_expand_backward(proj, idx, arg, W2a, W3, gout.contiguous(), ctx.r)
        return g["gproj"], None, g["gW2a"], g["gW3"], g["gb3"], None


class EF_expansion(nn.Module):
    """model_utils.py:24-55: x (B,input_size,N) -> (B,output_size,N*step_ratio), composed from houv_knn_feat, row gathers and
    houv_gemm_f32 (not fused: ECG uses it only when num_points > num_coarse + num_input; VRCNet's two expansions, 256 -> 64 and
    64 -> 256, are the same code).  The reference's view / permute chain
    is kept: the (B,k,N,output_size*step_ratio) activations of conv2 are REINTERPRETED as (B,k,N*step_ratio,output_size).
    trainable=True (output_size in 64, 128, 256, step_ratio and k <= 8): with grad mode on, forward_rows
    builds a graph -- two per-point products and one _EFExpandFunction node -- whose output equals the composition's within fp32
    spread, not bit for bit; rows may require a gradient.  With the flag off, or grad mode off, the composition runs, no graph."""

    def __init__(self, input_size, output_size=64, step_ratio=2, k=4, trainable=False):
        super().__init__()
        self.step_ratio, self.k, self.input_size, self.output_size = step_ratio, k, input_size, output_size
        self.trainable = bool(trainable)
        self.conv1 = Conv1x1(input_size * 2, output_size, 2)
        self.conv2 = Conv1x1(input_size * 2 + output_size, output_size * step_ratio, 2)
        self.conv3 = Conv1x1(output_size, output_size, 2)

    def forward_rows(self, rows, idx=None, trace=None, name="knn_exp"):
        """rows (B,N,input_size) -> (B,N*step_ratio,output_size); `name`: the key under which a trace records the lists.
        trainable=True with grad mode on: the graph path (_forward_rows_graph); otherwise the composition below, no graph."""
        if self.trainable and torch.is_grad_enabled():
            return self._forward_rows_graph(rows, idx, trace, name)
        with torch.no_grad():
            return self._forward_rows_composed(rows, idx, trace, name)

    def _forward_rows_graph(self, rows, idx, trace, name):
        """everything that depends on one point alone is a per-point product -- [U | V] = x W1^T (+ b1
        on U) and [P | Q] = relu(x) W2[:, O:]^T (+ b2 on P), two _LinearRowsFunction calls over column slices of the conv
        weights -- and the per-edge rest is one node (_EFExpandFunction).  The lists come from the detached rows: constants,
        as in the reference."""
        B, N, C = rows.shape
        O, r = self.output_size, self.step_ratio
        with torch.no_grad():
            if idx is None:
                idx = ops.knn_feat(rows.detach(), self.k)
            if trace is not None:
                trace[name], trace[name + "_x"] = idx, rows.detach().clone()
        x = rows.reshape(B * N, C)
        W1, W2 = self.conv1.matrix(), self.conv2.matrix()
        zeros = rows.new_zeros(O)
        # one product per activation: W1's halves stacked as [W1c; W1n] (2O rows of C columns), conv2's x-columns as [W2c; W2n]
        UV = _LinearRowsFunction.apply(x, torch.cat((W1[:, :C], W1[:, C:]), 0), torch.cat((self.conv1.bias, zeros)), False)
        PQ = _LinearRowsFunction.apply(torch.relu(x), torch.cat((W2[:, O:O + C], W2[:, O + C:]), 0),
                                       torch.cat((self.conv2.bias, rows.new_zeros(O * r))), False)
        proj = torch.cat((UV, PQ), 1).view(B, N, 2 * O + 2 * O * r)
        out, _ = _EFExpandFunction.apply(proj, idx.int().contiguous(), W2[:, :O], self.conv3.matrix(), self.conv3.bias, r)
        return out

    def _forward_rows_composed(self, rows, idx=None, trace=None, name="knn_exp"):
        B, N, C = rows.shape
        if idx is None:
            idx = ops.knn_feat(rows, self.k)
        if trace is not None:
            trace[name], trace[name + "_x"] = idx, rows.clone()
        k = idx.shape[2]
        nb = _take_rows(rows, idx).permute(0, 2, 1, 3)                            # (B,k,N,C): the reference's B C K N as rows
        edge = torch.cat((rows.unsqueeze(1).expand_as(nb), nb), dim=3).contiguous()
        cat = torch.empty((B, k, N, self.output_size + 2 * C), dtype=rows.dtype, device=rows.device)
        cat[..., :self.output_size] = self.conv1.rows(edge)
        cat[..., self.output_size:] = edge
        e = self.conv2.rows(torch.relu_(cat), relu=True)                          # (B,k,N,output_size*step_ratio)
        e = self.conv3.rows(e.view(B, k, N * self.step_ratio, self.output_size))
        return e.amax(dim=1)

    def forward(self, x):
        return self.forward_rows(x.transpose(1, 2).contiguous().float()).transpose(1, 2).contiguous()
