"""GPU: FPS / k-NN cross / gather_points against exact host restatements (tests/pointops_host.py, tests/hostmath): FPS and
k-NN index for index and bit for bit at every kernel instantiation and dispatch border, gather against torch.gather past the
grid cap.  Parity with the reference itself is unpinned: its versions are CUDA extensions with no fixtures."""
import numpy as np
import pytest
import torch

import pointops_host as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- houv_furthest_point_sample ---------------------------------------------------------------------------------------------
# The library is built with -ffp-contract=off and the kernel computes (dx*dx + dy*dy) + dz*dz: operation for operation what
# pointops_host.fps computes in NumPy float32.  There is no sum-order freedom, so every index must agree.
@pytest.mark.parametrize("B,N,m", [(2, 300, 64), (1, 2048, 512), (2, 5000, 100), (3, 100, 100)])
def test_fps(dev, B, N, m):
    from houv_amd.mm3d_pn2 import furthest_point_sample
    gen = torch.Generator().manual_seed(N)
    x = torch.rand(B, N, 3, generator=gen)
    idx = furthest_point_sample(x.to(dev), m).cpu().numpy()
    for b in range(B):
        ref = host.fps(x[b].numpy(), m)
        np.testing.assert_array_equal(idx[b], ref, err_msg=f"batch row {b}")
        assert len(set(idx[b].tolist())) == m or m > N


# (B, N, npoint): the smallest input; npoint = N; fps_kernel<256,4> full | <512,8> with 3071 padding slots; <512,8> full |
# <1024,16>; <1024,16> full.  A different cloud per batch row.
FPS_BRANCHES = [(2, 1, 1), (3, 100, 100), (2, 1024, 33), (2, 1025, 33), (1, 4096, 20), (1, 4097, 20), (1, 16384, 12)]


@pytest.mark.parametrize("B,N,m", FPS_BRANCHES)
def test_fps_every_kernel_and_dispatch_border(dev, B, N, m):
    from houv_amd.mm3d_pn2 import furthest_point_sample
    idx = furthest_point_sample(torch.tensor(host.fps_cloud(B, N)).to(dev), m)
    assert idx.shape == (B, m) and idx.dtype == torch.int32
    np.testing.assert_array_equal(idx.cpu().numpy(), host.fps_expected(B, N, m))


@pytest.mark.parametrize("N", [1500, 5000])
def test_fps_lattice_ties_and_exhaustion(dev, N):
    """The 1/8 lattice (512 sites): every difference, square and sum is exact in fp32, so the result cannot depend on
    contraction or order; thousands of exact ties, each won by the lowest index; 600 picks exhaust the sites, after which
    every running minimum is 0 and the pick is index 0.  No numerical excuse for any difference."""
    from houv_amd.mm3d_pn2 import furthest_point_sample
    B, m = 2, 600
    idx = furthest_point_sample(torch.tensor(host.fps_cloud(B, N, "lattice")).to(dev), m).cpu().numpy()
    want = host.fps_expected(B, N, m, "lattice")
    assert (want[:, -1] == 0).all() and (want[:, 1] != 0).all()
    np.testing.assert_array_equal(idx, want)


def test_fps_refuses_more_than_16384_points(dev):
    from houv_amd import _lib
    from houv_amd.mm3d_pn2 import furthest_point_sample
    with pytest.raises(_lib.HouvHipError):
        furthest_point_sample(torch.zeros(1, 16385, 3, device=dev), 4)


# ---- houv_knn_cross ---------------------------------------------------------------------------------------------------------
# One k per kernel (knn_cross_kernel<1|3>, knn_cross_queued_kernel<8|16|32>) and one per write-prefix kout < K.
KNN_K = (1, 3, 8, 16, 32, 2, 5, 9, 17)
# (B, N, M); M None = k (the list exactly full).  257 queries: a second query block with 255 idle lanes.  M = 1024: one LDS tile
# exactly; 1025: one reference in the second tile; 2049: three tiles.
KNN_SHAPES = [(2, 1, 1), (1, 256, None), (2, 257, 1024), (2, 300, 1025), (1, 255, 2049)]


def _as_bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("B,N,M", KNN_SHAPES)
@pytest.mark.parametrize("family", host.KNN_FAMILIES)
def test_knn_cross_every_entry_exact(dev, family, B, N, M):
    """dist2 bit-identical and idx equal to hm_knn_cross_fmaf, every entry of every list: the (distance, then lower index)
    order, the strict < of the insertion and the stale-threshold queue leave no freedom."""
    from houv_amd.mm3d_pn2 import knn_cross
    ran = 0
    for k in KNN_K:
        m = k if M is None else M
        if k > m:
            continue
        q, r = host.knn_inputs(family, B, N, m)
        want_i, want_d = host.knn_expected(family, B, N, m, k)
        d, i = knn_cross(k, torch.tensor(q).to(dev), torch.tensor(r).to(dev))
        assert d.shape == i.shape == (B, N, k) and d.dtype == torch.float32 and i.dtype == torch.int32
        np.testing.assert_array_equal(i.cpu().numpy(), want_i, err_msg=f"idx, k={k}")
        np.testing.assert_array_equal(_as_bits(d.cpu().numpy()), _as_bits(want_d), err_msg=f"dist2 bits, k={k}")
        ran += 1
    assert ran == (1 if M == 1 else len(KNN_K))


@pytest.mark.parametrize("family", host.KNN_FAMILIES)
def test_three_nn_is_sqrt_of_the_exact_three_list(dev, family):
    from houv_amd.mm3d_pn2 import three_nn
    B, N, M = 2, 300, 1025
    q, r = host.knn_inputs(family, B, N, M)
    want_i, want_d = host.knn_expected(family, B, N, M, 3)
    d, i = three_nn(torch.tensor(q).to(dev), torch.tensor(r).to(dev))
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    want = torch.sqrt(torch.tensor(np.ascontiguousarray(want_d)).to(dev))
    np.testing.assert_array_equal(_as_bits(d.cpu().numpy()), _as_bits(want.cpu().numpy()))


# ---- houv_gather_points -----------------------------------------------------------------------------------------------------
# (B, C, N, M).  The last is 5.12 M outputs > 16384 blocks x 256 lanes: the grid is capped and the kernel strides past the cap.
@pytest.mark.parametrize("B,C,N,M", [(1, 1, 1, 1), (3, 5, 40, 7), (2, 64, 50, 40000)])
@pytest.mark.parametrize("pattern", ["equal", "last", "random"])
def test_gather_points_equals_torch_gather(dev, pattern, B, C, N, M):
    from houv_amd.mm3d_pn2 import gather_points
    gen = torch.Generator().manual_seed(M)
    f = torch.randn(B, C, N, generator=gen).to(dev)
    if pattern == "equal":
        idx = torch.full((B, M), N // 2, dtype=torch.int32)
    elif pattern == "last":
        idx = torch.full((B, M), N - 1, dtype=torch.int32)
    else:
        idx = torch.randint(0, N, (B, M), generator=gen, dtype=torch.int32)
    idx = idx.to(dev)
    out = gather_points(f, idx)
    assert out.shape == (B, C, M)
    assert torch.equal(out, torch.gather(f, 2, idx.long().unsqueeze(1).expand(B, C, M)))


def test_grouping_operation_equals_torch_gather(dev):
    from houv_amd.mm3d_pn2 import grouping_operation
    gen = torch.Generator().manual_seed(9)
    B, C, N, P, S = 2, 9, 50, 300, 16
    f = torch.randn(B, C, N, generator=gen).to(dev)
    idx = torch.randint(0, N, (B, P, S), generator=gen, dtype=torch.int32).to(dev)
    out = grouping_operation(f, idx)
    want = torch.gather(f, 2, idx.long().view(B, 1, P * S).expand(B, C, P * S)).view(B, C, P, S)
    assert out.shape == (B, C, P, S) and torch.equal(out, want)


def test_three_nn_and_gather(dev):
    from houv_amd.mm3d_pn2 import gather_points, three_nn
    gen = torch.Generator().manual_seed(3)
    t = torch.rand(2, 333, 3, generator=gen); s = torch.rand(2, 1500, 3, generator=gen)
    d, i = three_nn(t.to(dev), s.to(dev))
    D = torch.cdist(t.double(), s.double())
    rd, ri = D.topk(3, dim=-1, largest=False)
    np.testing.assert_allclose(d.cpu().numpy(), rd.float().numpy(), atol=1e-5)
    assert (i.cpu().long() == ri).float().mean() > 0.999
    f = torch.randn(2, 7, 1500, generator=gen)
    g = gather_points(f.to(dev), i[:, :, 0].contiguous())
    np.testing.assert_array_equal(g.cpu().numpy(), torch.gather(f, 2, i[:, :, 0].cpu().long().unsqueeze(1).expand(2, 7, 333)).numpy())


def test_combine(dev):
    from houv_amd.train_utils import combine
    a = torch.rand(2, 1500, 3, device=dev); b = torch.rand(2, 1500, 3, device=dev)
    c = combine(a, b)
    assert c.shape == (2, 2048, 3)
    allp = torch.cat([a, b], 1)
    assert torch.equal(c[:, 0], allp[:, 0])                          # FPS starts at point 0
    # every sampled point is exactly the input point FPS chose
    from houv_amd.mm3d_pn2 import furthest_point_sample
    idx = furthest_point_sample(allp.contiguous(), 2048).long()
    assert torch.equal(c, torch.gather(allp, 1, idx.unsqueeze(2).expand(-1, -1, 3)))


def test_wrappers_validate_dtypes_and_indices(dev):
    """torch-default int64 indices (argsort / topk) and non-fp32 features must not be reinterpreted silently;
    out-of-range indices must be refused (the gather kernel does not bounds-check)."""
    from houv_amd import _lib, ops
    from houv_amd.mm3d_pn2 import furthest_point_sample, gather_points, three_nn
    g = torch.Generator().manual_seed(0)
    feats = torch.rand(2, 5, 40, generator=g).to(dev)
    idx64 = torch.argsort(torch.rand(2, 40, generator=g), dim=1)[:, :7].to(dev)          # int64, like torch.topk / argsort give
    want = torch.gather(feats, 2, idx64.unsqueeze(1).expand(2, 5, 7))
    assert torch.equal(gather_points(feats, idx64), want)
    assert torch.equal(gather_points(feats.double(), idx64.int()), want)                 # fp64 features are converted, not reinterpreted
    with pytest.raises(_lib.HouvHipError):
        gather_points(feats, torch.full((2, 3), 40, dtype=torch.int64, device=dev))      # out of range
    with pytest.raises(_lib.HouvHipError):
        gather_points(feats, idx64.float())
    pts = torch.rand(2, 64, 3, generator=g).to(dev)
    assert torch.equal(furthest_point_sample(pts.double(), 9), furthest_point_sample(pts, 9))
    with pytest.raises(_lib.HouvHipError):
        furthest_point_sample(pts, 65)
    d_a, i_a = three_nn(pts.double(), pts[:, :20].double())
    d_b, i_b = three_nn(pts, pts[:, :20].contiguous())
    assert torch.equal(i_a, i_b) and torch.equal(d_a, d_b)
    with pytest.raises(_lib.HouvHipError):
        ops.softmax_rows_(torch.rand(4, 8, device=dev).double())
    with pytest.raises(_lib.HouvHipError):
        ops.layernorm(torch.rand(4, 8, device=dev), torch.ones(7, device=dev), torch.zeros(8, device=dev))
    with pytest.raises(_lib.HouvHipError):
        ops.edgeconv1(pts, torch.zeros(2, 64, 20, dtype=torch.int64, device=dev), torch.rand(64, 6, device=dev),
                      torch.ones(64, device=dev), torch.zeros(64, device=dev))
