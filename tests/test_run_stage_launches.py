"""CPU: exactly which launches houv_amd.solver.run_stage makes -- the seed call and every ops.solve_iterate call with its cut
(steps_done, n_iters), output switches, workspace, ws_valid, kernel and stage arguments -- for the one-launch stage, the chunked
and the large-cloud form.  The launch functions are replaced by recorders (as in tests/test_solve_large_cabi.py); the sequences
are stated literally.  Also: the five solve entries of _lib._SIGNATURES share their 26 leading argument types."""
import ctypes

import numpy as np
import pytest
import torch


class _Props:
    multi_processor_count = 256


@pytest.fixture
def recorded(monkeypatch):
    """run_stage with every launch recorded instead of run.  Per ops.solve_seed call ("seed", hypotheses); per ops.solve_iterate
    call (hypotheses, steps_done, n_iters, want_grad, want_cd, nn_ws given, ws_valid, large, chunk_iters, sched_ws.numel() | None).
    ``calls.seen`` holds the state[:, :8] each solve_iterate call found."""
    from houv_amd import _lib, ops, solver

    class Calls(list):
        pass
    calls = Calls()
    calls.seen, calls.total = [], None                                 # total: P*K of the stage under way (_stage sets it)

    def fake_solve_seed(src, tgt, state, K, angle_base, trans_mode, use_views, nn_ws):
        assert nn_ws is not None and state.shape == (src.shape[0] * K, 24)
        calls.append(("seed", src.shape[0] * K))
        return 1

    def fake_solve_iterate(src, tgt, state, K, *, steps_done, n_iters, want_grad=False, want_cd=False, nn_ws=None,
                           ws_valid=False, large=False, chunk_iters=None, sched_ws=None, **kw):
        n = src.shape[0] * K
        assert state.shape == (n, 24) and tgt.shape[0] == src.shape[0]
        assert kw["loss_scale"] == 1.0 / calls.total and kw["k_full"] == src.shape[1] // 2 and kw["k_view"] == src.shape[1]
        calls.seen.append(state[:, :8].clone())
        state[:, 0] += n_iters                                         # marks the iterations each hypothesis received
        calls.append((n, steps_done, n_iters, want_grad, want_cd, nn_ws is not None, ws_valid, large, chunk_iters,
                      None if sched_ws is None else sched_ws.numel()))
        return dict(score=state[:, 7].float(), loss=torch.zeros(n), R=torch.zeros(n, 3, 3), T=torch.zeros(n, 3))
    monkeypatch.setattr(ops, "solve_iterate", fake_solve_iterate)
    monkeypatch.setattr(ops, "solve_seed", fake_solve_seed)
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: _Props())
    monkeypatch.setattr(solver, "PRUNED", True)
    monkeypatch.setattr(solver, "SEED_FIRST", True)
    monkeypatch.setattr(solver, "LARGE_IMPL", "fused")
    assert solver.LAUNCH_LOG is None and solver.ITERS_PER_LAUNCH == 50
    return calls


def _stage(calls, N=300, P=1, K=26, n_iters=8, **kw):
    """run_stage on CPU clouds; checks what holds after every case.  Returns out."""
    from houv_amd import solver
    g = torch.Generator().manual_seed(N)
    src, tgt = (torch.rand(P, N, 3, generator=g), torch.rand(P, N, 3, generator=g)) if N <= 4096 else \
               (torch.zeros(P, N, 3), torch.zeros(P, N, 3))
    params = np.zeros((P * K, 8))
    params[:, 7] = np.arange(P * K)                                    # the hypothesis' number: the fake's score
    del calls[:], calls.seen[:]
    calls.total = P * K
    out, state = solver.run_stage(src, tgt, params, K, n_iters, angle_base=0, trans_mode=0, use_views=True, f64_params=False,
                                  lr=0.01, want_grad=True, want_cd=True, **kw)
    assert state.shape == (P * K, 24) and bool((state[:, 0] == n_iters).all())
    assert torch.equal(out["score"], torch.arange(P * K, dtype=torch.float32))
    assert ("last_params" in out) == bool(kw.get("want_last_params"))
    if kw.get("want_last_params"):
        assert out["last_params"].dtype == torch.float64 and torch.equal(out["last_params"], calls.seen[-1])
        assert bool((out["last_params"][:, 0] == n_iters - 1).all())
    return out


SEED = ("seed", 26)


def test_default_stage_is_one_seeded_launch(recorded):
    _stage(recorded)
    assert recorded == [SEED, (26, 0, 8, True, True, True, True, False, 50, 30)]


def test_chunked_launches(recorded):
    _stage(recorded, iters_per_launch=3)
    assert recorded == [SEED,
                        (26, 0, 3, False, False, True, True, False, None, None),
                        (26, 3, 3, False, False, True, True, False, None, None),
                        (26, 6, 2, True, True, True, True, False, None, None)]


def test_chunked_launches_with_last_params(recorded):
    _stage(recorded, iters_per_launch=3, want_last_params=True)
    assert recorded == [SEED,
                        (26, 0, 3, False, False, True, True, False, None, None),
                        (26, 3, 3, False, False, True, True, False, None, None),
                        (26, 6, 1, False, False, True, True, False, None, None),
                        (26, 7, 1, True, True, True, True, False, None, None)]


def test_last_params_alone_takes_the_chunked_form(recorded):
    _stage(recorded, want_last_params=True)
    assert recorded == [SEED,
                        (26, 0, 7, False, False, True, True, False, None, None),
                        (26, 7, 1, True, True, True, True, False, None, None)]


def test_verify_mode_is_never_seeded(recorded):
    _stage(recorded, pruned="verify")
    assert recorded == [(26, 0, 8, True, True, True, "verify", False, 50, 30)]
    _stage(recorded, pruned="verify", iters_per_launch=3)
    assert recorded == [(26, 0, 3, False, False, True, "verify", False, None, None),
                        (26, 3, 3, False, False, True, "verify", False, None, None),
                        (26, 6, 2, True, True, True, "verify", False, None, None)]


def test_brute_force_stage_has_no_workspace_and_no_seed(recorded):
    _stage(recorded, pruned=False)
    assert recorded == [(26, 0, 8, True, True, False, False, False, 50, 30)]
    _stage(recorded, N=200)                                            # up to 256 points: brute force under any switch
    assert recorded == [(26, 0, 8, True, True, False, False, False, 50, 30)]


def test_unseeded_chunks_validate_the_workspace_after_the_first(recorded, monkeypatch):
    from houv_amd import solver
    monkeypatch.setattr(solver, "SEED_FIRST", False)
    _stage(recorded, iters_per_launch=3)
    assert recorded == [(26, 0, 3, False, False, True, False, False, None, None),
                        (26, 3, 3, False, False, True, True, False, None, None),
                        (26, 6, 2, True, True, True, True, False, None, None)]


def test_large_launches_with_last_params(recorded):
    _stage(recorded, N=5000, iters_per_launch=3, want_last_params=True)
    assert recorded == [(26, 0, 3, False, False, False, False, True, None, None),
                        (26, 3, 3, False, False, False, False, True, None, None),
                        (26, 6, 1, False, False, False, False, True, None, None),
                        (26, 7, 1, True, True, False, False, True, None, None)]


def test_large_launches_split_along_pairs(recorded):
    _stage(recorded, N=16384, P=256, K=64, n_iters=2)                  # score in hypothesis order: checked in _stage
    assert recorded == [(2048, 0, 1, False, False, False, False, True, None, None),
                        (2048, 1, 1, True, True, False, False, True, None, None)] * 8


def test_solve_signatures_share_their_common_arguments():
    from houv_amd import _lib
    P, I = ctypes.c_void_p, ctypes.c_int
    names = ("iterate", "iterate_large", "iterate_pruned", "stage", "stage_pruned")
    args = [_lib._SIGNATURES["houv_solve_" + n][1] for n in names]
    assert [len(a) for a in args] == [27, 27, 30, 29, 32]
    assert all(_lib._SIGNATURES["houv_solve_" + n][0] is ctypes.c_int for n in names)
    assert all(a[:26] == args[0][:26] for a in args)
    assert args[0][26:] == [P] and args[1][26:] == [P]                 # the stream
    assert args[2][26:] == [P, I, I, P]
    assert args[3][26:] == [I, P, P]
    assert args[4][26:] == [P, I, I, I, P, P]
