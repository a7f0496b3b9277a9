"""GPU: ball_query, grouping_operation, three_interpolate, their gradients (the ordered scatter), houv_knn_cross for k in 1..32
and the model_utils_completion helpers built on them, against the host restatements of tests/pointops_host.py.  Ball query,
three-interpolate and the scatter are compared EXACTLY: both sides evaluate the same fp32 expression tree in the same order."""
import numpy as np
import pytest
import torch

import pointops_host as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bq(dev, xyz, ctr, lo, hi, ns):
    from houv_amd.mm3d_pn2 import ball_query
    idx, cnt = ball_query(lo, hi, ns, torch.from_numpy(xyz).to(dev), torch.from_numpy(ctr).to(dev), return_count=True)
    assert idx.dtype == torch.int32 and not idx.requires_grad
    return idx.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("N,Mc,ns,seed", [(300, 1, 1, 0), (300, 102, 8, 1), (2048, 102, 24, 2), (2048, 2048, 64, 3),
                                           (5000, 102, 64, 4), (5000, 2048, 8, 5), (2048, 1, 24, 6), (300, 2048, 1, 7)])
def test_ball_query_random_clouds(dev, N, Mc, ns, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.random((2, N, 3), dtype=np.float32)
    ctr = rng.random((2, Mc, 3), dtype=np.float32)
    r = 0.5 * (ns * 6.0 / (np.pi * N)) ** (1 / 3)            # about half the balls fill up
    idx, cnt = _bq(dev, xyz, ctr, 0.3 * r, r, ns)
    ridx, rcnt = host.ball_query(xyz, ctr, 0.3 * r, r, ns)
    print(f"N={N} Mc={Mc} nsample={ns}: full {np.mean(rcnt == ns):.2f} empty {np.mean(rcnt == 0):.2f}")
    np.testing.assert_array_equal(cnt, rcnt)
    np.testing.assert_array_equal(idx, ridx)


def test_ball_query_bounds_and_edges(dev):
    """Coordinates on the 1/8 grid with radii 0.25 / 0.5: d2 lands exactly on both bounds (0.0625 inclusive, 0.25 strict)."""
    rng = np.random.default_rng(11)
    xyz = (rng.integers(0, 9, (2, 700, 3)) / 8.0).astype(np.float32)
    ctr = (rng.integers(0, 9, (2, 150, 3)) / 8.0).astype(np.float32)
    ctr[0, 0] = xyz[0, 17]                                   # a centre on a point with min_radius > 0: the d2 == 0 clause
    ctr[0, 1] = 50.0                                         # no hit: all slots 0, cnt 0
    ctr[1, 2] = [3.0, 0.0, 0.0]
    xyz[1, 650] = [3.25, 0.0, 0.0]                           # exactly min_radius away: in
    xyz[1, 651] = [3.5, 0.0, 0.0]                            # exactly max_radius away: out
    xyz[1, 652] = [3.125, 0.0, 0.0]                          # inside min_radius: out
    xyz[1, 653] = [3.375, 0.0, 0.0]                          # in: two hits for 24 slots, the padding repeats 650
    idx, cnt = _bq(dev, xyz, ctr, 0.25, 0.5, 24)
    ridx, rcnt = host.ball_query(xyz, ctr, 0.25, 0.5, 24)
    np.testing.assert_array_equal(cnt, rcnt)
    np.testing.assert_array_equal(idx, ridx)
    assert cnt[0, 1] == 0 and (idx[0, 1] == 0).all()
    assert cnt[1, 2] == 2 and idx[1, 2].tolist() == [650, 653] + [650] * 22
    d2 = ((ctr.astype(np.float64)[:, :, None] - xyz.astype(np.float64)[:, None]) ** 2).sum(-1)      # exact on this grid
    hit = (d2 == 0) | ((d2 >= 0.0625) & (d2 < 0.25))
    assert hit[0, 0, 17] and 17 in idx[0, 0].tolist()
    assert (d2[hit] == 0.0625).any() and (d2 == 0.25).any()                  # both bounds are met exactly somewhere
    nhit = hit.sum(-1)
    assert (nhit > 24).any() and ((nhit > 0) & (nhit < 24)).any()            # more and fewer hits than slots
    for b, c in zip(*np.nonzero(nhit > 24)):
        assert idx[b, c].tolist() == np.flatnonzero(hit[b, c])[:24].tolist()  # the first nsample in index order


def test_ball_query_validation(dev):
    from houv_amd import _lib
    from houv_amd.mm3d_pn2 import ball_query
    x = torch.rand(1, 10, 3, device=dev)
    for bad in (lambda: ball_query(0, 0.1, 65, x, x), lambda: ball_query(0.2, 0.1, 4, x, x), lambda: ball_query(0, 0.1, 4, x[0], x),
                lambda: ball_query(0, 0.1, 0, x, x)):
        with pytest.raises(_lib.HouvHipError):
            bad()


def test_three_interpolate_forward_and_validation(dev):
    from houv_amd import _lib
    from houv_amd.mm3d_pn2 import three_interpolate
    rng = np.random.default_rng(5)
    f = rng.standard_normal((3, 17, 512)).astype(np.float32)
    idx = rng.integers(0, 512, (3, 2048, 3)).astype(np.int32)
    w = rng.random((3, 2048, 3)).astype(np.float32)
    out = three_interpolate(torch.from_numpy(f).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev))
    assert out.cpu().numpy().tobytes() == host.three_interpolate(f, idx, w).tobytes()
    ft, it, wt = torch.from_numpy(f).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev)
    assert torch.equal(three_interpolate(ft.double(), it.long(), wt), out)
    for bad in (lambda: three_interpolate(ft, it.float(), wt), lambda: three_interpolate(ft, it + 512, wt),
                lambda: three_interpolate(ft, it[:, :, :2].contiguous(), wt[:, :, :2].contiguous()),
                lambda: three_interpolate(ft[0], it, wt)):
        with pytest.raises(_lib.HouvHipError):
            bad()


def _check_grad(got, g, idx, w, N, S, longest):
    """got: the GPU gradient (B,C,N); bit-equal to the ordered restatement, and within fp32 rounding of float64.
    Bound: a sequential fp32 sum of n terms errs by at most (n-1) u sum|t| with u = 2^-24 (Higham, Accuracy and Stability,
    eq. 4.4), each product adding u|t|: at most n u sum|t| <= n^2 u max|t|.  With |t| of order 1 and u = 6e-8 < 1e-5 / n for
    every n used here, atol = 1e-5 * n (n the longest list) covers it, rtol 1e-5 the well-conditioned destinations."""
    ref = host.scatter_points_grad(g, idx, w, N, S)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()
    B, C, _ = g.shape
    M = idx.shape[1]
    terms = torch.from_numpy(g).double()[:, :, torch.arange(M) // S]
    if w is not None:
        terms = terms * torch.from_numpy(w).double()[:, None]
    f64 = torch.zeros(B, C, N, dtype=torch.float64)
    for b in range(B):
        f64[b].index_add_(1, torch.from_numpy(idx[b]).long(), terms[b])
    np.testing.assert_allclose(got, f64.numpy(), rtol=1e-5, atol=1e-5 * longest)


def _longest(idx, N):
    return int(max(np.bincount(row, minlength=N).max() for row in idx))


def test_gather_points_gradient(dev):
    from houv_amd.mm3d_pn2 import gather_points
    rng = np.random.default_rng(21)
    B, C, N, M = 2, 6, 500, 3000
    f = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32)).to(dev).requires_grad_()
    idx = rng.integers(0, N, (B, M)).astype(np.int32)
    g = rng.standard_normal((B, C, M)).astype(np.float32)
    it = torch.from_numpy(idx).to(dev)
    out = gather_points(f, it)
    assert torch.equal(out.detach(), torch.gather(f.detach(), 2, it.long().unsqueeze(1).expand(B, C, M)))
    grad1, = torch.autograd.grad(out, f, torch.from_numpy(g).to(dev))
    grad2, = torch.autograd.grad(gather_points(f, it), f, torch.from_numpy(g).to(dev))
    assert torch.equal(grad1, grad2)
    _check_grad(grad1.cpu().numpy(), g, idx, None, N, 1, _longest(idx, N))


def test_gather_points_gradient_all_indices_equal(dev):
    """One list of length M = 40960: the worst case of the inverse index, and of the summation error."""
    from houv_amd.mm3d_pn2 import gather_points
    rng = np.random.default_rng(22)
    B, C, N, M = 2, 4, 2048, 40960
    f = torch.zeros(B, C, N, device=dev, requires_grad=True)
    idx = np.empty((B, M), np.int32)
    idx[0], idx[1] = 1234, 0
    g = rng.standard_normal((B, C, M)).astype(np.float32)
    it, gt = torch.from_numpy(idx).to(dev), torch.from_numpy(g).to(dev)
    grad1, = torch.autograd.grad(gather_points(f, it), f, gt)
    grad2, = torch.autograd.grad(gather_points(f, it), f, gt)
    assert torch.equal(grad1, grad2)
    _check_grad(grad1.cpu().numpy(), g, idx, None, N, 1, M)
    assert (grad1[0, :, :1234] == 0).all() and (grad1[1, :, 1:] == 0).all()


def test_grouping_operation_gradient_with_ball_query_padding(dev):
    from houv_amd.mm3d_pn2 import ball_query, grouping_operation
    rng = np.random.default_rng(23)
    B, C, N, Mc, ns = 2, 5, 2048, 2048, 20
    xyz = torch.from_numpy(rng.random((B, N, 3), dtype=np.float32)).to(dev)
    idx_t = ball_query(0, 0.06, ns, xyz, xyz)                              # ~2 hits per ball: 18 of 20 slots are padding
    idx = idx_t.cpu().numpy()
    assert (idx[:, :, 1:] == idx[:, :, :1]).mean() > 0.5
    f = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32)).to(dev).requires_grad_()
    out = grouping_operation(f, idx_t)
    assert out.shape == (B, C, Mc, ns)
    want = torch.gather(f.detach(), 2, idx_t.view(B, 1, -1).long().expand(B, C, Mc * ns)).view(B, C, Mc, ns)
    assert torch.equal(out.detach(), want)
    g = rng.standard_normal((B, C, Mc, ns)).astype(np.float32)
    grad1, = torch.autograd.grad(out, f, torch.from_numpy(g).to(dev))
    grad2, = torch.autograd.grad(grouping_operation(f, idx_t), f, torch.from_numpy(g).to(dev))
    assert torch.equal(grad1, grad2)
    flat = idx.reshape(B, Mc * ns)
    _check_grad(grad1.cpu().numpy(), g.reshape(B, C, Mc * ns), flat, None, N, 1, _longest(flat, N))


def test_grouping_operation_gradient_all_indices_equal_and_wide_destinations(dev):
    """M = 40960 equal indices through grouping_operation, and N = 20000 > the 8192 destinations one pass of the inverse index
    holds in LDS."""
    from houv_amd.mm3d_pn2 import grouping_operation
    rng = np.random.default_rng(24)
    B, C, N = 1, 3, 20000
    f = torch.zeros(B, C, N, device=dev, requires_grad=True)
    idx = np.full((B, 2048, 20), 19999, np.int32)
    g = rng.standard_normal((B, C, 2048, 20)).astype(np.float32)
    grad, = torch.autograd.grad(grouping_operation(f, torch.from_numpy(idx).to(dev)), f, torch.from_numpy(g).to(dev))
    _check_grad(grad.cpu().numpy(), g.reshape(B, C, -1), idx.reshape(B, -1), None, N, 1, 40960)
    idx = rng.integers(0, N, (B, 300, 20)).astype(np.int32)
    g = rng.standard_normal((B, C, 300, 20)).astype(np.float32)
    grad, = torch.autograd.grad(grouping_operation(f, torch.from_numpy(idx).to(dev)), f, torch.from_numpy(g).to(dev))
    flat = idx.reshape(B, -1)
    _check_grad(grad.cpu().numpy(), g.reshape(B, C, -1), flat, None, N, 1, _longest(flat, N))


def test_three_interpolate_gradient(dev):
    from houv_amd.mm3d_pn2 import three_interpolate
    rng = np.random.default_rng(25)
    B, C, M, N = 2, 7, 512, 2048
    f = torch.from_numpy(rng.standard_normal((B, C, M)).astype(np.float32)).to(dev).requires_grad_()
    idx = rng.integers(0, M, (B, N, 3)).astype(np.int32)
    idx[1] = 7                                                             # every weight of cloud 1 lands on one source
    w = rng.random((B, N, 3)).astype(np.float32)
    g = rng.standard_normal((B, C, N)).astype(np.float32)
    it, wt, gt = torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev).requires_grad_(), torch.from_numpy(g).to(dev)
    out = three_interpolate(f, it, wt)
    grad1, = torch.autograd.grad(out, f, gt)
    grad2, = torch.autograd.grad(three_interpolate(f, it, wt), f, gt)
    assert torch.equal(grad1, grad2)
    _check_grad(grad1.cpu().numpy(), g, idx.reshape(B, N * 3), w.reshape(B, N * 3), M, 3, N * 3)


@pytest.mark.parametrize("k", [2, 10, 20, 32])
def test_knn_point(dev, k):
    from houv_amd.model_utils_completion import knn_point
    gen = torch.Generator().manual_seed(k)
    t = torch.rand(2, 333, 3, generator=gen); s = torch.rand(2, 1500, 3, generator=gen)
    nd, i = knn_point(k, s.to(dev), t.to(dev))
    assert nd.shape == (2, 333, k) and i.dtype == torch.int64
    rd, ri = (torch.cdist(t.double(), s.double()) ** 2).topk(k, dim=-1, largest=False)
    np.testing.assert_allclose(-nd.cpu().numpy(), rd.float().numpy(), atol=1e-5)
    agree = (i.cpu() == ri).float().mean().item()
    print(f"k={k}: index agreement {agree:.5f}")
    assert agree > 0.999


def test_knn_cross_prefix_property_and_unchanged_kernels(dev):
    """The first k entries of a longer list are the k-list (stable insertion by (distance, index)): every k in 1..32 equals the
    prefix of the 32-list, and k = 1, 3 equal the prefix of the k = 8 kernel's list, which three_nn (k = 3) still returns."""
    from houv_amd import _lib
    from houv_amd.mm3d_pn2 import knn_cross, three_nn
    gen = torch.Generator().manual_seed(9)
    q = torch.rand(2, 777, 3, generator=gen).to(dev); r = torch.rand(2, 1900, 3, generator=gen).to(dev)
    d32, i32 = knn_cross(32, q, r)
    d8, i8 = knn_cross(8, q, r)
    for k in range(1, 33):
        d, i = knn_cross(k, q, r)
        assert torch.equal(d, d32[:, :, :k]) and torch.equal(i, i32[:, :, :k]), k
    for k in (1, 3):
        d, i = knn_cross(k, q, r)
        assert torch.equal(d, d8[:, :, :k]) and torch.equal(i, i8[:, :, :k])
    dist, i3 = three_nn(q, r)
    assert torch.equal(i3, i8[:, :, :3]) and torch.equal(dist, torch.sqrt(d8[:, :, :3]))
    with pytest.raises(_lib.HouvHipError):
        knn_cross(33, q, r)
    with pytest.raises(_lib.HouvHipError):
        knn_cross(5, q, r[:, :4].contiguous())


def _close(a, b, tol=1e-5):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=tol, atol=tol)


def test_edge_preserve_sampling(dev):
    from houv_amd.model_utils_completion import edge_preserve_sampling
    gen = torch.Generator().manual_seed(31)
    pts = torch.rand(2, 1024, 3, generator=gen).to(dev)
    feat = torch.randn(2, 16, 1024, generator=gen).to(dev).requires_grad_()
    net, p_idx, pn_idx, point_output = edge_preserve_sampling(feat, pts, 256, k=10)
    assert net.shape == (2, 32, 256) and p_idx.shape == (2, 256) and pn_idx.shape == (2, 256, 10) and pn_idx.dtype == torch.int32
    feat_r = feat.detach().clone().requires_grad_()
    net_r, out_r = host.edge_preserve_sampling(feat_r, pts, p_idx, pn_idx)
    assert torch.equal(net.detach(), net_r.detach()) and torch.equal(point_output, out_r)
    assert (pn_idx[:, :, 0] == p_idx).all()                                # a sampled point's nearest point is itself
    w = torch.randn(net.shape, generator=gen).to(dev)
    (net * w).sum().backward()
    (net_r * w).sum().backward()
    assert feat.grad.abs().sum() > 0
    _close(feat.grad, feat_r.grad)


def test_get_repulsion_loss(dev):
    from houv_amd.model_utils_completion import get_repulsion_loss, knn
    gen = torch.Generator().manual_seed(32)
    pred = (torch.rand(2, 2048, 3, generator=gen) * 0.5).to(dev).requires_grad_()
    loss = get_repulsion_loss(pred)
    idx = knn(pred.detach().transpose(1, 2).contiguous(), 20)
    assert idx.shape == (2, 2048, 20) and (idx[:, :, 0] == torch.arange(2048, device=dev)).all()
    pred_r = pred.detach().clone().requires_grad_()
    loss_r = host.get_repulsion_loss(pred_r, idx)
    _close(loss, loss_r, 1e-6)
    loss.backward(); loss_r.backward()
    assert pred.grad.abs().sum() > 0
    _close(pred.grad, pred_r.grad, 1e-6)


def test_get_uniform_loss(dev):
    from houv_amd.mm3d_pn2 import ball_query, furthest_point_sample, gather_points
    from houv_amd.model_utils_completion import get_uniform_loss
    gen = torch.Generator().manual_seed(33)
    pcd = torch.rand(2, 2048, 3, generator=gen).to(dev).requires_grad_()
    loss = get_uniform_loss(pcd)
    fps = furthest_point_sample(pcd.detach(), int(2048 * 0.05))
    new_xyz = gather_points(pcd.detach().transpose(1, 2).contiguous(), fps).transpose(1, 2).contiguous()
    balls = [ball_query(0, float(np.sqrt(p)), int(2048 * p), pcd.detach(), new_xyz) for p in (0.004, 0.006, 0.008, 0.010, 0.012)]
    pcd_r = pcd.detach().clone().requires_grad_()
    loss_r = host.get_uniform_loss(pcd_r, fps, balls)
    # the restatement takes the nearest-other distance from the expanded pairwise matrix, the helper from the gathered pair:
    # both are fp32 sums of three squares of values below 1, equal to a few ulps of 1e-2-sized distances
    _close(loss, loss_r, 1e-4)
    loss.backward(); loss_r.backward()
    assert pcd.grad.abs().sum() > 0
    np.testing.assert_allclose(pcd.grad.cpu().numpy(), pcd_r.grad.cpu().numpy(), rtol=1e-3, atol=1e-4 * pcd_r.grad.abs().max().item())


def test_three_nn_upsampling_and_interpolate(dev):
    from houv_amd.mm3d_pn2 import three_interpolate, three_nn
    from houv_amd.model_utils_completion import three_nn_upsampling
    gen = torch.Generator().manual_seed(34)
    tgt = torch.rand(2, 2048, 3, generator=gen).to(dev); src = torch.rand(2, 512, 3, generator=gen).to(dev)
    src[0, 5] = tgt[0, 9]                                                  # a zero distance: clamped at 1e-10
    feat = torch.randn(2, 12, 512, generator=gen).to(dev).requires_grad_()
    idx, weight = three_nn_upsampling(tgt, src)
    dist, idx_r = three_nn(tgt, src)
    assert torch.equal(idx, idx_r) and idx.dtype == torch.int32
    _close(weight, host.three_nn_weights(dist), 1e-6)
    _close(weight.sum(2), torch.ones(2, 2048, device=dev), 1e-6)
    out = three_interpolate(feat, idx, weight)
    feat_r = feat.detach().clone().requires_grad_()
    out_r = (host._take(feat_r, idx) * weight.unsqueeze(1)).sum(-1)
    _close(out, out_r)
    w = torch.randn(out.shape, generator=gen).to(dev)
    (out * w).sum().backward(); (out_r * w).sum().backward()
    assert feat.grad.abs().sum() > 0
    _close(feat.grad, feat_r.grad, 1e-4)


def test_symmetric_sample(dev):
    from houv_amd.mm3d_pn2 import furthest_point_sample
    from houv_amd.model_utils_completion import symmetric_sample
    gen = torch.Generator().manual_seed(35)
    pts = (torch.rand(2, 2048, 3, generator=gen) - 0.5).to(dev).requires_grad_()
    out = symmetric_sample(pts, 512)
    assert out.shape == (2, 1024, 3)
    idx = furthest_point_sample(pts.detach(), 512)
    pts_r = pts.detach().clone().requires_grad_()
    assert torch.equal(out.detach(), host.symmetric_sample(pts_r, idx).detach())
    w = torch.randn(out.shape, generator=gen).to(dev)
    (out * w).sum().backward(); (host.symmetric_sample(pts_r, idx) * w).sum().backward()
    assert pts.grad.abs().sum() > 0
    _close(pts.grad, pts_r.grad, 1e-6)


def test_query_and_group(dev):
    from houv_amd.mm3d_pn2 import GroupAll, QueryAndGroup, ball_query
    gen = torch.Generator().manual_seed(36)
    xyz = torch.rand(2, 1024, 3, generator=gen).to(dev)
    ctr = xyz[:, :128].contiguous()
    feat = torch.randn(2, 6, 1024, generator=gen).to(dev).requires_grad_()
    idx = ball_query(0.02, 0.15, 16, xyz, ctr)
    off = host._take(xyz.transpose(1, 2), idx) - ctr.transpose(1, 2).unsqueeze(-1)
    with_f, gx = QueryAndGroup(0.15, 16, min_radius=0.02, return_grouped_xyz=True)(xyz, ctr, feat)
    assert with_f.shape == (2, 9, 128, 16)
    assert torch.equal(gx, off) and torch.equal(with_f.detach(), torch.cat([off, host._take(feat.detach(), idx)], 1))
    with_f.sum().backward()
    assert feat.grad.abs().sum() > 0
    assert torch.equal(QueryAndGroup(0.15, 16, min_radius=0.02)(xyz, ctr), off)                 # without features
    assert torch.equal(QueryAndGroup(0.15, 16, min_radius=0.02, normalize_xyz=True, use_xyz=False)(xyz, ctr, feat).detach(),
                       host._take(feat.detach(), idx))
    near = QueryAndGroup(None, 8)(xyz, ctr)                                                    # kNN grouping
    assert near.shape == (2, 3, 128, 8) and (near[:, :, :, 0] == 0).all()
    assert GroupAll()(xyz, None, feat).shape == (2, 9, 1, 1024)
