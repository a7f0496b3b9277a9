"""GPU: houv_kd_sort (ops.kd_sort / torch.ops.houv.kd_sort) returns, bit for bit, the permutation of solver.kd_sort -- the torch
specification -- on the same device, for every size, leaf, rule and for hostile clouds (ties, zero extents, signed zeros,
infinities, NaNs of either sign and any payload, overflowing areas); and swapping it into solver.spatial_sort changes nothing
downstream."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RULES = ("area", "extent")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gather(x, order):
    return torch.gather(x, 1, order.long().unsqueeze(2).expand(-1, -1, 3))


def _check(x, leaf, rule):
    """ops.kd_sort against solver.kd_sort; the order output is a permutation that produces the sorted cloud.  Returns the output."""
    from houv_amd import ops, solver
    ref = solver.kd_sort(x.clone(), leaf, rule)
    out, order = ops.kd_sort(x, leaf, rule, return_order=True)
    assert out.shape == x.shape and order.shape == x.shape[:2] and order.dtype == torch.int32
    assert torch.equal(_bits(out), _bits(ref)), (tuple(x.shape), leaf, rule)
    assert torch.equal(torch.sort(order.long(), dim=1)[0], torch.arange(x.shape[1], device=x.device).expand(x.shape[0], -1))
    assert torch.equal(_bits(_gather(x, order)), _bits(out))
    assert torch.equal(_bits(ops.kd_sort(x, leaf, rule)), _bits(out))        # without order
    return out


def _cloud(P, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, N, 3, generator=g) * torch.tensor([2.0, 1.0, 0.5]) - 0.3).to(dev)


@pytest.mark.parametrize("N", [1, 20, 32, 33, 64, 600, 1800, 2048, 2049, 3000, 4096])
def test_kd_sort_equals_torch_spec_sizes(dev, N):
    for P in (1, 3):
        x = _cloud(P, N, 1000 * N + P, dev)
        for leaf in (16, 32, 64, 128):
            for rule in RULES:
                _check(x, leaf, rule)


@pytest.mark.parametrize("N,leaf", [(2048, 32), (4096, 64)])
def test_kd_sort_equals_torch_spec_batch_of_256(dev, N, leaf):
    from houv_amd import synthetic
    src, tgt, _ = synthetic.make_pairs(128, N, seed=7)
    x = torch.cat([src, tgt]).to(dev)
    for rule in RULES:
        _check(x, leaf, rule)


def _hostile(dev):
    """name -> cloud [P,N,3] on dev."""
    g = torch.Generator().manual_seed(11)
    N = 700
    base = torch.rand(3, N, 3, generator=g)
    c = {}
    dup = base.clone()
    dup[:, 350:] = dup[:, :350]
    c["duplicates"] = dup[:, torch.randperm(N, generator=g)]
    c["all_equal"] = torch.full((2, 333, 3), 0.25)
    c["grid"] = torch.randint(0, 4, (3, N, 3), generator=g).float()
    c["grid_1d_ties"] = torch.stack([torch.randint(0, 3, (N,), generator=g).float(), torch.zeros(N), torch.zeros(N)], 1)[None]
    plane = base.clone()
    plane[..., 2] = 0.5
    c["planar"] = plane
    line = base.clone()
    line[..., 1] = line[..., 0] * 2.0
    line[..., 2] = 0.0
    c["collinear"] = line
    z = torch.randint(-1, 2, (3, N, 3), generator=g).float()
    neg = torch.rand(3, N, 3, generator=g) < 0.5
    c["signed_zeros"] = torch.where((z == 0) & neg, torch.tensor(-0.0), z)
    inf = base.clone()
    m = torch.rand(3, N, 3, generator=g)
    inf[m < 0.03] = float("inf")
    inf[m > 0.97] = float("-inf")
    c["infinities"] = inf
    # NaNs of both signs and several payloads: torch's device sort orders them by their bits
    nans = torch.tensor([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFF800001, 0x7F800001, 0xFFFFFFFF],
                        dtype=torch.int64).to(torch.int32).view(torch.float32)
    one = base.clone()
    r = torch.randint(0, 3, (3, N), generator=g)
    pick = torch.rand(3, N, generator=g) < 0.05
    for k, (p, i) in enumerate(pick.nonzero().tolist()):
        one[p, i, r[p, i]] = nans[k % len(nans)]
    c["nan_one_coordinate"] = one
    allc = base.clone()
    for k, (p, i) in enumerate(pick.nonzero().tolist()):
        allc[p, i, :] = nans[k % len(nans)]
    c["nan_all_coordinates"] = allc
    mix = c["signed_zeros"].clone()
    mix[0, 5] = float("inf")
    mix[1, 7, 0] = float("nan")
    mix[2, 9, 1] = -float("inf")
    c["mixed_specials"] = mix
    c["near_1e20"] = (base - 0.5) * 2e20                       # products overflow: inf areas, inf - inf never, ties at inf
    big = (base - 0.5) * 2e20
    big[:, ::7, 0] = 3e38
    big[:, 1::7, 0] = -3e38                                    # extents overflow to inf, 0 * inf = NaN areas
    big[:, ::5, 2] = 0.0
    c["overflowing_extents"] = big
    return {k: v.contiguous().to(dev) for k, v in c.items()}


@pytest.mark.parametrize("rule", RULES)
def test_kd_sort_equals_torch_spec_hostile_clouds(dev, rule):
    for name, x in _hostile(dev).items():
        for leaf in (16, 32, 64):
            try:
                _check(x, leaf, rule)
            except AssertionError as e:
                raise AssertionError(f"{name} leaf={leaf}: {e}") from None


def test_kd_sort_order_is_idempotent_and_permutation_invariant(dev):
    from houv_amd import ops
    x = _cloud(3, 1800, 5, dev)
    grid = torch.randint(0, 5, (2, 1000, 3), generator=torch.Generator().manual_seed(6)).float().to(dev)
    for cloud, leaf in ((x, 32), (grid, 64), (grid, 16)):
        for rule in RULES:
            out, order = ops.kd_sort(cloud, leaf, rule, return_order=True)
            again, order2 = ops.kd_sort(out, leaf, rule, return_order=True)
            assert torch.equal(_bits(again), _bits(out))
            assert torch.equal(order2.long(), torch.arange(cloud.shape[1], device=dev).expand(cloud.shape[0], -1))
            perm = torch.randperm(cloud.shape[1], generator=torch.Generator().manual_seed(leaf)).to(dev)
            assert torch.equal(_bits(ops.kd_sort(cloud[:, perm].contiguous(), leaf, rule)), _bits(out))


def test_kd_sort_on_side_stream_and_torch_op(dev):
    from houv_amd import ops
    ops.register_torch_ops()
    x = _cloud(4, 2049, 8, dev)
    ref, ref_order = ops.kd_sort(x, 64, "area", return_order=True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out, order = ops.kd_sort(x, 64, "area", return_order=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert torch.equal(_bits(out), _bits(ref)) and torch.equal(order, ref_order)
    for rule in RULES:
        o1, r1 = torch.ops.houv.kd_sort(x, 32, rule)
        o2, r2 = ops.kd_sort(x, 32, rule, return_order=True)
        assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(r1, r2)


def test_kd_sort_bad_arguments_raise(dev):
    from houv_amd import _lib, ops
    x = _cloud(1, 100, 9, dev)
    for kw in (dict(leaf=0), dict(rule="median")):
        with pytest.raises(_lib.HouvHipError):
            ops.kd_sort(x, **kw)
    with pytest.raises(_lib.HouvHipError):
        ops.kd_sort(_cloud(1, 4097, 9, dev))
    with pytest.raises(_lib.HouvHipError):
        ops.kd_sort(x.cpu())
    assert ops.kd_sort(x[:0]).shape == (0, 100, 3)


def test_spatial_sort_same_tensor_under_both_impls(dev, monkeypatch):
    from houv_amd import solver
    assert solver.KD_SORT_IMPL == "hip"
    for N, leaf in ((640, 32), (2048, 32), (3000, 64)):
        x = _cloud(2, N, N, dev)
        res = {}
        for impl in ("hip", "torch"):
            monkeypatch.setattr(solver, "KD_SORT_IMPL", impl)
            res[impl] = solver.spatial_sort(x, leaf)
            assert solver.spatial_sort(res[impl], leaf) is res[impl]            # recognised as sorted either way
        assert torch.equal(_bits(res["hip"]), _bits(res["torch"]))
        for rule in RULES:
            monkeypatch.setattr(solver, "KD_RULE", rule)
            monkeypatch.setattr(solver, "KD_SORT_IMPL", "hip")
            h = solver.spatial_sort(x, leaf)
            monkeypatch.setattr(solver, "KD_SORT_IMPL", "torch")
            assert torch.equal(_bits(h), _bits(solver.spatial_sort(x, leaf)))


@pytest.mark.parametrize("N", [2048, 3000])
def test_pruned_run_stage_identical_under_both_impls(dev, monkeypatch, N):
    from houv_amd import solver, synthetic
    src, tgt, _ = synthetic.make_pairs(2, N, seed=N)
    p0 = solver.houv_init_params(2 * 13, 2021)
    assert solver.uses_pruned(N, N, True) and solver.sort_leaf(N, N) == (32 if N <= 2048 else 64)
    res = {}
    for impl in ("hip", "torch"):
        monkeypatch.setattr(solver, "KD_SORT_IMPL", impl)
        out, state = solver.run_stage(src.to(dev), tgt.to(dev), p0, 13, 3, angle_base=1, trans_mode=0, use_views=True,
                                      f64_params=False, lr=0.01, pruned=True)
        res[impl] = (out["score"], out["R"], out["T"], state)
    for a, b in zip(res["hip"], res["torch"]):
        assert torch.equal(a, b)
