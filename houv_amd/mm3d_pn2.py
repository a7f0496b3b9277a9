"""Mirror of the `mm3d_pn2` ops the reference imports (registration/train_utils.py:20, registration/model_utils_completion.py:19,
registration/models/vrcnet.py:18): ``furthest_point_sample, gather_points, grouping_operation, ball_query, three_nn,
three_interpolate`` and the ``QueryAndGroup`` / ``GroupAll`` modules, on the gfx950 kernels of houv_amd/csrc/pointops.hip and
pointops_group.hip.  FPS, three_nn and ball_query are non-differentiable, as in the reference; gather_points,
grouping_operation and three_interpolate carry a gradient for their features, computed by the ordered scatter
houv_scatter_points_grad (deterministic: no float atomics)."""
import torch

from . import _lib

_F32, _I32 = torch.float32, torch.int32


def _f32(t, name):
    """The kernels read raw fp32: convert other float dtypes (the result must stay referenced until after the launch)."""
    if not t.is_floating_point():
        raise _lib.HouvHipError(f"{name}: expected a floating-point tensor, got {t.dtype}")
    return t if t.dtype == _F32 else t.float()


def _i32(t, name, bound):
    """Indices arrive as int32 (the reference's ops) or int64 (torch.topk / argsort defaults): convert the latter, and
    refuse anything outside [0, bound) -- the gather kernels do not bounds-check."""
    if t.dtype not in (_I32, torch.int64):
        raise _lib.HouvHipError(f"{name}: expected int32 / int64 indices, got {t.dtype}")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= bound):
        raise _lib.HouvHipError(f"{name}: index out of range [0, {bound})")
    return t if t.dtype == _I32 else t.to(_I32)


def furthest_point_sample(points_xyz, num_points):
    """points_xyz (B,N,3) contiguous, N >= num_points -> (B,num_points) int32 indices (furthest_point_sample.py:15-36)."""
    _lib.require_gpu(points_xyz)
    if points_xyz.dim() != 3 or points_xyz.shape[2] != 3 or not 0 < int(num_points) <= points_xyz.shape[1]:
        raise _lib.HouvHipError("furthest_point_sample: expected points_xyz[B,N,3] and 0 < num_points <= N")
    pts = _f32(points_xyz, "points_xyz")                 # kept alive in a local until the launch is enqueued
    B, N, _ = pts.shape
    out = torch.empty((B, num_points), dtype=_I32, device=pts.device)
    _lib.call("houv_furthest_point_sample", pts, pts, B, N, num_points, out)
    return out


def _scatter_grad(grad_out, idx, weight, N, S):
    """houv_scatter_points_grad: grad_out (B,C,M/S), idx (B,M) int32 in [0,N), weight (B,M) or None -> (B,C,N)."""
    grad_out = grad_out.contiguous()
    if grad_out.dtype != _F32:
        grad_out = grad_out.float()
    B, C, _ = grad_out.shape
    M = idx.shape[1]
    ws = _lib.workspace("houv_scatter_points_workspace_bytes", grad_out.device, B, N, M, floor=0)[0]
    grad = torch.empty((B, C, N), dtype=_F32, device=grad_out.device)
    _lib.call("houv_scatter_points_grad", grad_out, grad_out, idx, weight, B, C, N, M, S, grad, ws)
    return grad


def _gather_forward(feats, idx):
    """feats (B,C,N) fp32, idx (B,M) int32, both contiguous and validated -> (B,C,M)."""
    B, C, N = feats.shape
    M = idx.shape[1]
    out = torch.empty((B, C, M), dtype=_F32, device=feats.device)
    _lib.call("houv_gather_points", feats, feats, idx, B, C, N, M, out)
    return out


class _Gather(torch.autograd.Function):
    """gather_points and grouping_operation: one gather forward, one ordered scatter backward, over idx viewed as (B,M)."""

    @staticmethod
    def forward(ctx, feats, idx):
        ctx.save_for_backward(idx)
        ctx.N = feats.shape[2]
        return _gather_forward(feats, idx)

    @staticmethod
    def backward(ctx, grad_out):
        idx, = ctx.saved_tensors
        return _scatter_grad(grad_out, idx, None, ctx.N, 1), None


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, idx, weight):
        B, C, M = feats.shape
        N = idx.shape[1]
        ctx.save_for_backward(idx, weight)
        ctx.M = M
        out = torch.empty((B, C, N), dtype=_F32, device=feats.device)
        _lib.call("houv_three_interpolate", feats, feats, idx, weight, B, C, M, N, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        B, N, _ = idx.shape
        return _scatter_grad(grad_out, idx.view(B, N * 3), weight.view(B, N * 3), ctx.M, 3), None, None


def gather_points(features, indices):
    """features (B,C,N), indices (B,M) int32 -> (B,C,M) (gather_points.py:14-35); differentiable in features."""
    _lib.require_gpu(features, indices)
    if features.dim() != 3 or indices.dim() != 2 or indices.shape[0] != features.shape[0]:
        raise _lib.HouvHipError("gather_points: expected features[B,C,N], indices[B,M]")
    feats = _f32(features, "features")
    idx = _i32(indices, "indices", features.shape[2]).contiguous()
    return _Gather.apply(feats, idx)


def grouping_operation(features, indices):
    """features (B,C,N), indices (B,npoint,nsample) -> (B,C,npoint,nsample) = features[b,c,indices[b,p,s]]
    (group_points.py:166-221); differentiable in features.  The forward is houv_gather_points over indices viewed as
    (B, npoint*nsample)."""
    _lib.require_gpu(features, indices)
    if features.dim() != 3 or indices.dim() != 3 or indices.shape[0] != features.shape[0]:
        raise _lib.HouvHipError("grouping_operation: expected features[B,C,N], indices[B,npoint,nsample]")
    B, C, N = features.shape
    _, npoint, nsample = indices.shape
    feats = _f32(features, "features")
    idx = _i32(indices, "indices", N).contiguous().view(B, npoint * nsample)
    return _Gather.apply(feats, idx).view(B, C, npoint, nsample)


def three_interpolate(features, indices, weight):
    """features (B,C,M), indices (B,N,3) into M, weight (B,N,3) -> (B,C,N): the weighted sum of three source features per target
    point (three_interpolate.py:10-60); differentiable in features."""
    _lib.require_gpu(features, indices, weight)
    if features.dim() != 3 or indices.dim() != 3 or indices.shape[2] != 3 or weight.shape != indices.shape \
            or indices.shape[0] != features.shape[0]:
        raise _lib.HouvHipError("three_interpolate: expected features[B,C,M], indices[B,N,3], weight[B,N,3]")
    feats = _f32(features, "features")
    idx = _i32(indices, "indices", features.shape[2]).contiguous()
    w = _f32(weight, "weight").detach()
    return _ThreeInterpolate.apply(feats, idx, w)


def ball_query(min_radius, max_radius, sample_num, xyz, center_xyz, return_count=False):
    """xyz (B,N,3), center_xyz (B,npoint,3) -> (B,npoint,sample_num) int32: per centre the first sample_num points, in index
    order, at squared distance 0 or in [min_radius^2, max_radius^2); unused slots repeat the first, all 0 when there is none
    (ball_query.py:9-47).  Non-differentiable.  return_count=True adds the (B,npoint) int32 number of hits (capped)."""
    _lib.require_gpu(xyz, center_xyz)
    if xyz.dim() != 3 or center_xyz.dim() != 3 or xyz.shape[2] != 3 or center_xyz.shape[2] != 3 \
            or xyz.shape[0] != center_xyz.shape[0] or xyz.shape[1] < 1:
        raise _lib.HouvHipError("ball_query: expected xyz[B,N>=1,3], center_xyz[B,npoint,3]")
    if not 1 <= int(sample_num) <= 64 or not float(min_radius) < float(max_radius):
        raise _lib.HouvHipError("ball_query: expected 1 <= sample_num <= 64 and min_radius < max_radius")
    pts, ctr = _f32(xyz.detach(), "xyz"), _f32(center_xyz.detach(), "center_xyz")
    B, N, _ = pts.shape
    Mc = ctr.shape[1]
    idx = torch.empty((B, Mc, int(sample_num)), dtype=_I32, device=pts.device)
    cnt = torch.empty((B, Mc), dtype=_I32, device=pts.device) if return_count else None
    _lib.call("houv_ball_query", pts, pts, ctr, B, N, Mc, min_radius, max_radius, sample_num, idx, cnt)
    return (idx, cnt) if return_count else idx


def knn_cross(k, query, ref):
    """The k (1..32) nearest points of ref (B,M,3) for every query (B,N,3), nearest first -> (dist2 (B,N,k) squared, idx (B,N,k)
    int32) (houv_knn_cross).  Non-differentiable."""
    _lib.require_gpu(query, ref)
    if query.dim() != 3 or ref.dim() != 3 or query.shape[2] != 3 or ref.shape[2] != 3 or query.shape[0] != ref.shape[0] \
            or not 1 <= int(k) <= min(32, ref.shape[1]):
        raise _lib.HouvHipError("knn_cross: expected query[B,N,3], ref[B,M,3] and 1 <= k <= min(32, M)")
    q, r = _f32(query.detach(), "query"), _f32(ref.detach(), "ref")
    B, N, _ = q.shape
    d2 = torch.empty((B, N, int(k)), dtype=_F32, device=q.device)
    idx = torch.empty((B, N, int(k)), dtype=_I32, device=q.device)
    _lib.call("houv_knn_cross", q, q, r, B, N, r.shape[1], k, d2, idx)
    return d2, idx


def three_nn(target, source):
    """target (B,N,3), source (B,M,3) -> (dist (B,N,3) L2 distances, idx (B,N,3)) (three_nn.py:11-37 returns sqrt(dist2))."""
    _lib.require_gpu(target, source)
    if target.dim() != 3 or source.dim() != 3 or target.shape[2] != 3 or source.shape[2] != 3 or source.shape[0] != target.shape[0] \
            or source.shape[1] < 3:
        raise _lib.HouvHipError("three_nn: expected target[B,N,3], source[B,M>=3,3]")
    target, source = _f32(target, "target"), _f32(source, "source")
    B, N, _ = target.shape
    M = source.shape[1]
    d2 = torch.empty((B, N, 3), dtype=_F32, device=target.device)
    idx = torch.empty((B, N, 3), dtype=_I32, device=target.device)
    _lib.call("houv_knn_cross", target, target, source, B, N, M, 3, d2, idx)
    return torch.sqrt(d2), idx


class QueryAndGroup(torch.nn.Module):
    """Group the neighbours of every centre (group_points.py:11-122): the ball query of (min_radius, max_radius) with sample_num
    slots, or, with max_radius None, the sample_num nearest points.  forward(points_xyz (B,N,3), center_xyz (B,npoint,3),
    features (B,C,N) or None) -> (B, 3+C, npoint, sample_num): the neighbours' offsets from their centre (divided by max_radius
    under normalize_xyz) stacked on their features; features alone with use_xyz False; offsets alone without features.
    return_grouped_xyz appends the offsets.  uniform_sample (random re-draws of the unique hits on the host) is not built."""

    def __init__(self, max_radius, sample_num, min_radius=0, use_xyz=True, return_grouped_xyz=False, normalize_xyz=False,
                 uniform_sample=False, return_unique_cnt=False):
        super().__init__()
        if uniform_sample or return_unique_cnt:
            raise NotImplementedError("QueryAndGroup: uniform_sample / return_unique_cnt are not built")
        if max_radius is None and normalize_xyz:
            raise ValueError("QueryAndGroup: normalize_xyz needs a max_radius")
        self.max_radius, self.min_radius, self.sample_num = max_radius, min_radius, sample_num
        self.use_xyz, self.return_grouped_xyz, self.normalize_xyz = use_xyz, return_grouped_xyz, normalize_xyz

    def forward(self, points_xyz, center_xyz, features=None):
        if features is None and not self.use_xyz:
            raise ValueError("QueryAndGroup: without features, use_xyz must be set")
        if self.max_radius is None:
            _, idx = knn_cross(self.sample_num, center_xyz, points_xyz)
        else:
            idx = ball_query(self.min_radius, self.max_radius, self.sample_num, points_xyz, center_xyz)
        grouped_xyz = grouping_operation(points_xyz.transpose(1, 2).contiguous(), idx)
        grouped_xyz = grouped_xyz - center_xyz.transpose(1, 2).unsqueeze(-1)
        if self.normalize_xyz:
            grouped_xyz = grouped_xyz / self.max_radius
        if features is None:
            new_features = grouped_xyz
        else:
            grouped = grouping_operation(features, idx)
            new_features = torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped
        return (new_features, grouped_xyz) if self.return_grouped_xyz else new_features


class GroupAll(torch.nn.Module):
    """One group holding every point (group_points.py:125-163): forward(xyz (B,N,3), new_xyz ignored, features (B,C,N) or None)
    -> (B, 3+C, 1, N), the coordinates stacked on the features (features alone with use_xyz False)."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped
