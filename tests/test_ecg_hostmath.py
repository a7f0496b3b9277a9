"""CPU: hm_knn_feat (tests/ecg_hostmath), the host statement of houv_knn_feat's contract that the GPU test compares bit for bit,
against a stable float64 sort of the exact squared distances, on inputs with exact ties, and against hm_knn_cross_fmaf at C = 3."""
import numpy as np
import pytest

import ecg_cases as cases
import pointops_host


@pytest.mark.parametrize("family", ["random", "quarter"])
@pytest.mark.parametrize("B,N,C,ld", [(2, 65, 24, 24), (1, 97, 48, 52), (1, 40, 256, 256), (2, 33, 1, 3), (1, 50, 3, 4)])
def test_host_list_equals_float64_sort_where_the_gap_exceeds_tau(family, B, N, C, ld):
    """Where the exact squared distances of consecutive candidates in the float64 ranking differ by more than tau (relatively)
    on both sides of a position, the host list holds the float64 ranking's entry there; on the quarter lattice every distance
    is exact in fp32, so the whole list, ties included, equals the stable float64 sort and the distances are equal."""
    idx, dist = cases.knn_expected(family, B, N, C, ld)
    k = idx.shape[2]
    order, ds = cases.float64_ranking(cases.knn_cloud(family, B, N, C, ld), C, k)
    t = cases.tau(C)
    if family == "quarter":
        assert np.array_equal(idx, order[..., :k]) and np.array_equal(dist.astype(np.float64), ds[..., :k])
        assert (ds[..., 1:k] == ds[..., :k - 1]).sum() > 0                   # the case does hold exact ties
        return
    up = np.ones(idx.shape, bool)
    if N > k:
        up = ds[..., 1:k + 1] - ds[..., :k] > t * ds[..., 1:k + 1]
    else:
        up[..., :-1] = ds[..., 1:k] - ds[..., :k - 1] > t * ds[..., 1:k]
    down = np.ones_like(up)
    down[..., 1:] = up[..., :-1]
    safe = up & down
    assert safe.mean() > 0.9
    assert np.array_equal(idx[safe], order[..., :k][safe])
    assert np.abs(dist - ds[..., :k]).max() <= t / 2 * ds[..., :k].max()


def test_host_list_orders_ties_by_index():
    idx, dist = cases.knn_expected("identical", 2, 70, 24, 28)
    assert np.array_equal(idx, np.broadcast_to(np.arange(32, dtype=np.int32), idx.shape)) and not dist.any()
    # the quarter lattice: within a run of equal distances the indices ascend
    idx, dist = cases.knn_expected("quarter", 2, 65, 24, 24)
    tied = dist[..., 1:] == dist[..., :-1]
    assert tied.sum() > 0 and (idx[..., 1:][tied] > idx[..., :-1][tied]).all()
    assert (dist[..., 1:] >= dist[..., :-1]).all()


@pytest.mark.parametrize("family", cases.KNN_FAMILIES)
def test_three_channels_equal_the_coordinate_host_function(family):
    """C = 3: the chain fma(dz, dz, fma(dy, dy, fma(dx, dx, 0))) is hm_knn_cross_fmaf's fma(dz, dz, fma(dy, dy, dx*dx)) bit for
    bit (fma(t, t, 0) is the rounded product)."""
    x = cases.knn_cloud(family, 2, 70, 3, 3)
    idx, dist = cases.knn_expected(family, 2, 70, 3, 3)
    i3, d3 = pointops_host.knn_cross(x, x, 32)
    assert np.array_equal(idx, i3) and np.array_equal(dist.view(np.int32), d3.view(np.int32))
