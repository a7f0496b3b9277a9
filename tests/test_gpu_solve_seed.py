"""GPU: houv_solve_seed (csrc/solve_seed.hip) and the seeded first iteration of solver.run_stage.

The kernel alone: its records are in range, at a finite distance, written where prune_masks reads them and nowhere else; on grid
clouds under the identity pose (tests/solve_seed_cases.py: every product and sum exact in fp32) they equal the float64 statement
of the rule (scripts/sim_solve_seed.py `seed_records`) index for index, ties, NaN points and the partly filled last run included.

The stage: solver.SEED_FIRST on and off give the same bits in state and in every output, in the one-launch form and in the
chunk-by-chunk form -- any in-range record at a finite distance is an attained bound, and iteration 0 rescans every term."""
import ctypes

import numpy as np
import pytest
import torch

from solve_seed_cases import GRID_SHAPES, IDENTITY, expected_records, grid_pair, nan_grid_pair

CANARY = -21846            # 0xAAAA in every int16 the kernel must leave alone
K = 26                     # the fewest restarts houv_init_params accepts
KEYS = ("score", "loss", "R", "T", "grad", "cd")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _state(params, dev):
    state = torch.zeros((len(params), 24), dtype=torch.float64, device=dev)
    state[:, :8] = torch.as_tensor(np.asarray(params), dtype=torch.float64).to(dev)
    return state


def _seed(src, tgt, params, k, base, views):
    """-> (records of direction B [n, M, 4], of direction A [n, N, 4], every other int16 of the workspace) after one call."""
    from houv_amd import ops
    dev = src.device
    n, N, M = len(params), src.shape[1], tgt.shape[1]
    state = _state(params, dev)
    ws = ops.solve_workspace(n, N, M, dev)
    ws.fill_(CANARY)
    before = state.clone()
    ops.solve_seed(src, tgt, state, k, base, 0, views, ws)
    torch.cuda.synchronize()
    assert torch.equal(state, before)
    stride = ws.shape[2]
    flat = ws.cpu().numpy().reshape(n, 16 * stride)
    rec_b = flat[:, :4 * M].reshape(n, M, 4)
    rec_a = flat[:, 4 * stride:4 * stride + 4 * N].reshape(n, N, 4)
    rest = np.concatenate([flat[:, 4 * M:4 * stride], flat[:, 4 * stride + 4 * N:]], 1)
    return rec_b, rec_a, rest


def _generic(P, N, M, dev, seed=91):
    from houv_amd import solver, synthetic
    src, tgt, _ = synthetic.make_pairs(P, max(N, M), seed=seed)
    leaf = solver.sort_leaf(N, M)
    return (solver.spatial_sort(src[:, :N].contiguous().to(dev), leaf), solver.spatial_sort(tgt[:, :M].contiguous().to(dev), leaf))


# (N, M, views, angle window): every solve variant boundary the issue names, both seed-kernel block sizes, N != M with one metric
ALONE = [(257, 257, True, 0), (320, 320, True, 3), (768, 768, True, 0), (2048, 2048, True, 3), (2500, 2500, True, 0),
         (600, 450, False, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,views,base", ALONE)
def test_seed_records_are_in_range_finite_and_nothing_else_is_written(N, M, views, base):
    from houv_amd import ops, solver
    from scripts.sim_solve_seed import metric_sq, seed_records
    dev = _dev()
    P = 2
    src, tgt = _generic(P, N, M, dev)
    params = solver.houv_init_params(P * K)
    rec_b, rec_a, rest = _seed(src, tgt, params, K, base, views)
    nmet = 4 if views else 1
    assert (rest == CANARY).all(), "rows 8..15 and the records past the last point must be left alone"
    assert (rec_b[..., nmet:] == CANARY).all() and (rec_a[..., nmet:] == CANARY).all(), "metrics not in use"
    rb, ra = rec_b[..., :nmet].astype(np.int64), rec_a[..., :nmet].astype(np.int64)
    assert rb.min() >= 0 and rb.max() < N and ra.min() >= 0 and ra.max() < M
    # the kernel's own fp32 pose moves the cloud here too; the float64 statement on those points agrees but for ties within
    # fp32 rounding of two box or point distances (relative 1e-7 on random clouds: far below one query in a hundred)
    _, _, moved = ops.pose_forward(torch.as_tensor(params, dtype=torch.float32).to(dev), base, 0,
                                   src.repeat_interleave(K, dim=0).contiguous())
    moved, tgt_h = moved.cpu().double().numpy(), tgt.cpu().double().numpy()
    for h in (0, K + 4):
        t = tgt_h[h // K]
        for rec, q, refs in ((rb[h], t, moved[h]), (ra[h], moved[h], t)):
            d = np.take_along_axis(metric_sq(q[:, None, :] - refs[rec]), np.arange(nmet)[None, :, None], 2)[..., 0]
            assert np.isfinite(d).all()
            same = (rec == seed_records(q, refs, nmet)).mean()
            print(f"N={N} M={M} hypothesis {h}: {same:.5f} of the records equal the float64 statement")
            assert same >= 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,views", GRID_SHAPES)
@pytest.mark.parametrize("nan_points", [False, True])
def test_seed_records_equal_the_float64_statement_on_grid_clouds(N, M, views, nan_points):
    from scripts.sim_solve_seed import box_sq, run_boxes
    dev = _dev()
    src, tgt = (nan_grid_pair if nan_points else grid_pair)(N, M)
    nmet = 4 if views else 1
    exp_b, exp_a = expected_records(src, tgt, nmet)
    s, t = (torch.from_numpy(c)[None].contiguous().to(dev) for c in (src, tgt))
    rec_b, rec_a, rest = _seed(s, t, np.stack([IDENTITY, IDENTITY]), 2, 0, views)
    assert (rest == CANARY).all()
    for h in range(2):
        assert np.array_equal(rec_b[h, :, :nmet], exp_b), "direction B (target points into the source order)"
        assert np.array_equal(rec_a[h, :, :nmet], exp_a), "direction A (moved points into the target)"
    if nan_points:
        assert (rec_a[:, 5, :nmet] == 0).all() and (rec_b[:, 40, :nmet] == 0).all(), "a NaN query is seeded with 0"
        assert not (rec_b[..., :nmet] == 5).any() and not (rec_a[..., :nmet] == 40).any(), "a NaN reference seeds nobody"
        assert not ((rec_a[..., :nmet] >= 128) & (rec_a[..., :nmet] < 160)).any(), "nor does a run of NaN points"
        # run 6 of the target: a finite box, no point at a finite full-metric distance -> the queries it is nearest to fall back
        with np.errstate(invalid="ignore"):
            bs = box_sq(src.astype(np.float64), *run_boxes(tgt.astype(np.float64)))[..., 0]
        fell_back = np.where(np.isnan(bs), np.inf, bs).argmin(1) == 6
        fell_back[5] = False
        assert fell_back.sum() > 0 and not ((rec_a[0, fell_back, 0] >= 192) & (rec_a[0, fell_back, 0] < 224)).any()
        assert np.isfinite(((src[fell_back].astype(np.float64) - tgt[rec_a[0, fell_back, 0]]) ** 2).sum(1)).all()


@pytest.mark.gpu
def test_seed_refuses_bad_arguments_with_an_error_text():
    from houv_amd import _lib, ops
    dev = _dev()
    N = 320
    src, tgt = _generic(1, N, N, dev)
    state = _state(np.stack([IDENTITY] * 2), dev)
    ws = ops.solve_workspace(2, N, N, dev)
    ws.fill_(CANARY)
    lib = _lib.load()
    stream = _lib.stream_of(src)

    def call(src_=src, tgt_=tgt, P=1, n=N, m=N, k=2, st=state, base=0, mode=0, ws_=ctypes.c_void_p(ws.data_ptr()), stride=ws.shape[2]):
        return lib.houv_solve_seed(_lib.ptr(src_), _lib.ptr(tgt_), P, n, m, k, _lib.ptr(st), base, mode, 1, ws_, stride, stream)

    for kw, text in ((dict(ws_=None), "workspace"), (dict(ws_=ctypes.c_void_p(ws.data_ptr() + 8)), "16-byte aligned"),
                     (dict(stride=N - 8), "ws_stride"), (dict(stride=N + 4), "multiple of 8"), (dict(n=256, m=256), "257..4096"),
                     (dict(n=4097, m=N), "257..4096"), (dict(base=4), "bad argument"), (dict(mode=2), "bad argument"),
                     (dict(k=0), "bad argument"), (dict(n=0), "bad argument"), (dict(src_=None), "null pointer"),
                     (dict(st=None), "null pointer")):
        assert call(**kw) == 0, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    assert call(P=0) == 1
    torch.cuda.synchronize()
    assert bool((ws == CANARY).all()), "a refused call launches nothing"
    with pytest.raises(_lib.HouvHipError, match="nn_ws"):
        ops.solve_seed(src, tgt, state, 2, 0, 0, True, ws[:1])
    with pytest.raises(_lib.HouvHipError, match="state"):
        ops.solve_seed(src, tgt, state[:1], 2, 0, 0, True, ws)


# name: (pairs, N, M, views, f64 parameters, angle window, clouds)
STAGES = {
    "257pt": (2, 257, 257, True, False, 0, "generic"),
    "320pt_f64": (2, 320, 320, True, True, 1, "generic"),
    "768pt": (1, 768, 768, True, False, 2, "generic"),
    "2048pt": (1, 2048, 2048, True, False, 0, "generic"),
    "2500pt_f64": (1, 2500, 2500, True, True, 3, "generic"),
    "600x450_one_metric": (2, 600, 450, False, False, 1, "generic"),
    "300pt_nan_points": (1, 300, 300, True, False, 0, "nan"),
}


def _stage_problem(name, dev):
    from houv_amd import solver
    P, N, M, views, f64, base, kind = STAGES[name]
    if kind == "nan":
        src, tgt = (torch.from_numpy(c)[None].contiguous().to(dev) for c in nan_grid_pair(N, M))
    else:
        src, tgt = _generic(P, N, M, dev, seed=77)
    return src, tgt, torch.as_tensor(solver.houv_init_params(P * K), dtype=torch.float64)


def _run_stage(name, seeded, monkeypatch, dev, iters=8, **extra):
    from houv_amd import solver
    P, N, M, views, f64, base, _ = STAGES[name]
    src, tgt, p0 = _stage_problem(name, dev)
    monkeypatch.setattr(solver, "SEED_FIRST", seeded)
    out, state = solver.run_stage(src, tgt, p0, K, iters, angle_base=base, trans_mode=0, use_views=views, f64_params=f64, lr=0.01,
                                  want_grad=True, want_cd=True, **extra)
    torch.cuda.synchronize()
    solver.check_stage_status(wait=True)
    return out, state


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["one_launch", "chunked"])
@pytest.mark.parametrize("name", sorted(STAGES))
def test_seeded_stage_is_bit_identical_to_the_unseeded_one(name, form, monkeypatch):
    """1 + 7 iterations; chunked = iters_per_launch 3 (launches of 3, 3, 2)."""
    dev = _dev()
    extra = dict(iters_per_launch=3) if form == "chunked" else {}
    ref, st_ref = _run_stage(name, False, monkeypatch, dev, **extra)
    got, st = _run_stage(name, True, monkeypatch, dev, **extra)
    assert torch.equal(_bits(st), _bits(st_ref))
    for key in KEYS:
        assert torch.equal(_bits(got[key]), _bits(ref[key])), key
    if "nan" not in name:
        assert bool(torch.isfinite(ref["loss"]).all())


@pytest.mark.gpu
def test_seeded_stage_with_last_params_is_bit_identical(monkeypatch):
    dev = _dev()
    ref, st_ref = _run_stage("320pt_f64", False, monkeypatch, dev, want_last_params=True)
    got, st = _run_stage("320pt_f64", True, monkeypatch, dev, want_last_params=True)
    assert torch.equal(_bits(st), _bits(st_ref))
    for key in KEYS + ("last_params",):
        assert torch.equal(_bits(got[key]), _bits(ref[key])), key


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["one_launch", "chunked"])
def test_seeded_stage_runs_no_brute_force_sweep(form, monkeypatch):
    """solve_stats of a stage of the bench's kernel: [3] brute-force wave-sweeps, [2] pruned ones, [0] sub-tiles asked for.  One
    iteration alone shows the first iteration's lists: the replay (scripts/sim_solve_seed.py) gives 8.5 .. 9.4 of 64 sub-tiles
    per query at 2048 points; twice that is the bound."""
    from houv_amd import _lib
    dev = _dev()
    extra = dict(iters_per_launch=3) if form == "chunked" else {}
    buf = torch.zeros(8, dtype=torch.int64, device=dev)
    counts = {}
    for seeded, iters in ((False, 8), (True, 8), (True, 1)):
        buf.zero_()
        _lib.debug_set("solve_stats", buf.data_ptr())
        try:
            _run_stage("2048pt", seeded, monkeypatch, dev, iters=iters, **extra)
        finally:
            _lib.debug_set("solve_stats", 0)
        counts[(seeded, iters)] = [int(x) for x in buf.cpu()]
    waves = K * (512 // 64)
    # the first iteration computes every term: both directions of every wave; later ones may drop a direction (term masks), the
    # same ones in both runs since their results are the same bits
    assert counts[(False, 8)][3] == 2 * waves and counts[(False, 8)][2] > 0
    assert counts[(True, 8)][3] == 0 and counts[(True, 8)][2] == counts[(False, 8)][2] + 2 * waves
    first = counts[(True, 1)]
    assert first[3] == 0 and first[2] == 2 * waves
    per_query = first[0] / (first[2] * 64.0 * 4)
    print(f"seeded first iteration: {per_query:.2f} of 64 sub-tiles asked per query")
    assert per_query < 2 * 9.4


@pytest.mark.gpu
def test_retry_stages_give_the_same_answer_seeded_and_unseeded(monkeypatch):
    """best_of_k_with_retry on two pairs that both retry (8 iterations leave every score above 0.030): base stage + three retry
    stages on side streams, every one of them seeded."""
    from houv_amd import solver
    from houv_amd.models.houv import HOUV, predict_model
    dev = _dev()
    src, tgt = _generic(2, 320, 320, dev, seed=77)

    def stage(s, t, base):
        return predict_model(HOUV(s.shape[0] * K, base), s, t, kernel=K, num_epochs=8, angle_base=base)

    res = {}
    for seeded in (False, True):
        monkeypatch.setattr(solver, "SEED_FIRST", seeded)
        ans, score, retry = solver.best_of_k_with_retry(stage, src, tgt)
        torch.cuda.synchronize()
        solver.check_stage_status(wait=True)
        res[seeded] = (ans, score, retry)
    assert res[False][2].numel() == 2
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b) if a.dtype == torch.int64 else torch.equal(_bits(a), _bits(b))
