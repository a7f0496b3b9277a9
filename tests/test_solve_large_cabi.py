"""CPU: houv_solve_iterate_large (the fused loop for clouds of 4097..16384 points) is declared, exported and bound; it refuses
every bad argument on the host, before any launch; its kernels run without scratch inside the 1024-thread register budget and
160 KiB of LDS; and houv_amd.solver routes clouds to it, to the in-LDS kernels or to the un-fused path by size and switch."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_kd_sort_cabi import _kernel_metadata, _library
from tests.test_kernel_resources import LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_iterate_large_is_declared_exported_and_bound():
    _lib = _library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "houv_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+houv_solve_iterate_large\s*\(([^)]*)\)", header)
    plain = re.search(r"\bint\s+houv_solve_iterate\s*\(([^)]*)\)", header)
    norm = lambda m: re.sub(r"\s+", " ", m.group(1)).strip()
    assert decl and plain and norm(decl) == norm(plain)                     # the same arguments as houv_solve_iterate
    assert re.search(r"#define\s+HOUV_LARGE_MAX_POINTS\s+16384\b", header)
    assert "houv_solve_iterate_large" in _lib.exported_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "houv_solve_iterate_large")
    fn, ref = _lib.load().houv_solve_iterate_large, _lib.load().houv_solve_iterate
    assert fn.restype is ctypes.c_int and fn.argtypes == ref.argtypes and len(fn.argtypes) == 27
    assert _lib.load().houv_abi_version() == _lib.ABI_VERSION == 2          # additive: the ABI version stays


# Child process with no visible device: every call below must be refused by the host-side checks on fake, never dereferenced
# addresses.  Were a check missing, the call would get as far as reserving LDS and fail for want of a device instead -- which is
# what the last call (valid arguments at the largest size) does, reporting the LDS the kernel asks for.
_ARGS_CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
P, I, D, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
f = lib.houv_solve_iterate_large
f.restype = I
f.argtypes = [P, P, I, I, I, I, P, I, I, I, I, I, I, I, I, D, D, D, D, F, P, P, P, P, P, P, P]
lib.houv_last_error.restype = ctypes.c_char_p
x = 0x10000
#        src, tgt, N, M, views, k_full, k_view, state
cases = ((x, x, 0, 5000, 0, 1, 1, x), (x, x, 16385, 5000, 0, 100, 1, x), (x, x, 5000, 0, 0, 1, 1, x),
         (x, x, 5000, 16385, 0, 100, 1, x), (x, x, 5000, 4999, 1, 2499, 5000, x), (x, x, 6000, 6000, 1, 3000, 5999, x),
         (x, x, 5000, 4000, 0, 4001, 1, x), (x, x, 5000, 5000, 0, 0, 1, x), (None, x, 5000, 5000, 1, 2500, 5000, x),
         (x, None, 5000, 5000, 1, 2500, 5000, x), (x, x, 5000, 5000, 1, 2500, 5000, None),
         (x, x, 16384, 16384, 1, 8192, 16384, x))
for src, tgt, N, M, views, kf, kv, state in cases:
    ok = f(src, tgt, 1, N, M, 64, state, 0, 1, 0, 0, views, 0, kf, kv, 0.01, 0.9, 0.999, 1e-8, 1.0,
           None, None, None, None, None, None, None)
    print(ok, lib.houv_last_error().decode())
"""


def _child_lines():
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="999", ROCR_VISIBLE_DEVICES="999")
    out = subprocess.run([sys.executable, "-c", _ARGS_CHILD, LIB], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.strip().splitlines()


def test_solve_iterate_large_rejects_bad_arguments_before_any_launch():
    lines = _child_lines()
    expect = ["cloud sizes out of range", "cloud sizes out of range", "cloud sizes out of range", "cloud sizes out of range",
              "need N == M and k_view == N", "need N == M and k_view == N", "top-k size out of range",
              "top-k size out of range", "null pointer", "null pointer", "null pointer", "cannot reserve"]
    assert len(lines) == len(expect), lines
    for line, msg in zip(lines, expect):
        assert line.startswith("0 houv_solve_iterate_large: ") and msg in line, (line, msg)


def test_solve_large_kernels_have_no_scratch_and_fit_lds(tmp_path):
    kernels = _kernel_metadata(tmp_path, re.compile(r"solve_large_kernel"))
    assert len(kernels) == 2, sorted(kernels)                               # with and without the view terms
    # the LDS is dynamic: what the host reserves at the largest size (reported by the probe above) + any static LDS
    reserve = int(re.search(r"cannot reserve (\d+) B", _child_lines()[-1]).group(1))
    assert reserve == 40048 + 6 * 16384                                     # the size include/houv_hip.h documents
    for name, f in sorted(kernels.items()):
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["vgpr_count"]) <= 128, f"{name}: {f['vgpr_count']} VGPRs (1024 threads = 4 waves per SIMD need <= 128)"
        assert int(f["max_flat_workgroup_size"]) == 1024
        assert int(f["group_segment_fixed_size"]) + reserve <= 160 * 1024


# ---- routing in houv_amd.solver (host-side: the launch functions are replaced by recorders) ------------------------------
class _Props:
    multi_processor_count = 256


@pytest.fixture
def recorded(monkeypatch):
    """run_stage with every launch recorded instead of run: ("fused" | "large", hypotheses, iterations, steps_done) per
    ops.solve_iterate call, ("unfused", P*K) per _run_stage_unfused call."""
    from houv_amd import _lib, ops, solver
    calls = []

    def fake_solve_iterate(src, tgt, state, K, *, steps_done, n_iters, large=False, **kw):
        n = src.shape[0] * K
        assert state.shape == (n, 24) and tgt.shape[0] == src.shape[0]
        state[:, 0] += n_iters                                         # marks the iterations each hypothesis received
        calls.append(("large" if large else "fused", n, n_iters, steps_done))
        return dict(score=state[:, 7].float(), loss=torch.zeros(n),                       # the hypothesis' number (_stage)
                    R=torch.zeros(n, 3, 3), T=torch.zeros(n, 3))

    def fake_unfused(src, tgt, params, K, n_iters, **kw):
        calls.append(("unfused", src.shape[0] * K))
        return {}, None
    monkeypatch.setattr(ops, "solve_iterate", fake_solve_iterate)
    monkeypatch.setattr(solver, "_run_stage_unfused", fake_unfused)
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: _Props())
    return calls


def _stage(N, M=None, P=1, K=26, n_iters=3, **kw):
    from houv_amd import solver
    M = N if M is None else M
    src, tgt = torch.zeros(P, N, 3), torch.zeros(P, M, 3)
    params = np.zeros((P * K, 8))
    params[:, 7] = np.arange(P * K)
    return solver.run_stage(src, tgt, params, K, n_iters, angle_base=0, trans_mode=0, use_views=(N == M),
                            f64_params=False, lr=0.01, pruned=False, **kw)


def test_solver_routes_large_clouds_to_the_new_kernel(recorded, monkeypatch):
    from houv_amd import solver
    assert solver.LARGE_IMPL == "fused" and (solver.LARGE_MIN_POINTS, solver.LARGE_MAX_POINTS) == (4097, 16384)
    for N, M, want in ((4096, 4096, "fused"), (4097, 4097, "large"), (6000, 5000, "large"), (100, 8192, "large"),
                       (16384, 16384, "large"), (16385, 16385, "unfused"), (16385, 100, "unfused")):
        recorded.clear()
        _stage(N, M)
        assert recorded and {c[0] for c in recorded} == {want}, (N, M, recorded)
    # FUSED_MAX_POINTS keeps its meaning: 0 forces small clouds onto the un-fused path, and does not move the large bounds
    monkeypatch.setattr(solver, "FUSED_MAX_POINTS", 0)
    for N, want in ((600, "unfused"), (4096, "unfused"), (8192, "large")):
        recorded.clear()
        _stage(N)
        assert {c[0] for c in recorded} == {want}, (N, recorded)
    monkeypatch.setattr(solver, "FUSED_MAX_POINTS", 4096)
    # the A/B switch restores the old behaviour
    monkeypatch.setattr(solver, "LARGE_IMPL", "unfused")
    for N, want in ((8192, "unfused"), (4096, "fused")):
        recorded.clear()
        _stage(N)
        assert {c[0] for c in recorded} == {want}, (N, recorded)
    assert not solver.uses_large(8192, 8192)
    monkeypatch.setattr(solver, "LARGE_IMPL", "fused")
    assert solver.uses_large(8192, 8192) and not solver.uses_pruned(8192, 8192, True)   # no spatial sort on this path


def test_houv_large_environment_switch():
    code = "from houv_amd import solver; print(solver.LARGE_IMPL, solver.uses_large(8192, 8192), solver.uses_large(4096, 4096))"
    for value, want in (("unfused", "unfused False False"), ("fused", "fused True False"), (None, "fused True False")):
        env = dict(os.environ)
        env.pop("HOUV_LARGE", None)
        if value:
            env["HOUV_LARGE"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().splitlines()[-1] == want


def test_large_launches_stay_within_the_stated_bound(recorded):
    """256 pairs x 64 restarts of 16384-point clouds: every launch's estimated duration (solver.large_launch_seconds: rounds x
    iterations x point pairs / the measured per-CU rate) is within LARGE_LAUNCH_BUDGET_S, launches are split along pairs, every
    hypothesis receives every iteration exactly once, and the outputs come back in hypothesis order."""
    from houv_amd import solver
    P, K, N, iters = 256, 64, 16384, 3
    out, state = _stage(N, P=P, K=K, n_iters=iters)
    for kind, n, it, _ in recorded:
        est = solver.large_launch_seconds(n, it, N, N, _Props.multi_processor_count)
        assert kind == "large" and est <= solver.LARGE_LAUNCH_BUDGET_S, (n, it, est)
    assert max(c[1] for c in recorded) < P * K and all(c[1] % K == 0 for c in recorded)    # split along whole pairs
    assert bool((state[:, 0] == iters).all())
    assert torch.equal(out["score"], torch.arange(P * K, dtype=torch.float32))
    # smaller problems: split along iterations only, up to ITERS_PER_LAUNCH
    recorded.clear()
    _stage(8192, P=2, K=64, n_iters=120)
    assert [c[1] for c in recorded] == [128] * len(recorded) and sum(c[2] for c in recorded) == 120
    assert all(c[2] <= solver.ITERS_PER_LAUNCH for c in recorded)
    assert [c[3] for c in recorded] == list(np.cumsum([0] + [c[2] for c in recorded[:-1]]))


def test_large_launch_plan_bounds():
    from houv_amd import solver
    for P, K, N, M in ((256, 64, 16384, 16384), (256, 64, 8192, 8192), (1, 64, 16384, 16384), (4, 64, 4097, 4097),
                       (3, 1000, 16384, 16384), (256, 64, 6000, 5000)):
        pairs, iters = solver.large_launch_plan(P, K, N, M, 256)
        assert 1 <= pairs <= P and 1 <= iters <= solver.ITERS_PER_LAUNCH
        est = solver.large_launch_seconds(pairs * K, iters, N, M, 256)
        assert est >= -(-pairs * K // 256) * iters * 2.0 * N * M / solver.LARGE_PAIRS_PER_S_PER_CU * (1 - 1e-12)   # idle lanes count
        # within the budget, unless a single pair's single iteration is already over it (then one of each)
        assert est <= solver.LARGE_LAUNCH_BUDGET_S or (pairs, iters) == (1, 1), (P, K, N, M, pairs, iters, est)
