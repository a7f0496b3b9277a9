"""CPU: the C-ABI library loads and exports every symbol include/houv_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "houv_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(houv_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from houv_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = _declared()
    assert "houv_chamfer_forward" in names and "houv_solve_iterate" in names and "houv_kabsch" in names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/houv_hip.h but not exported"
    assert sorted(_lib.exported_symbols()) == names          # the Python binding covers the whole header
    assert _lib.load().houv_abi_version() == _lib.ABI_VERSION


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from houv_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.HouvHipError):
        _lib.load()


def test_cpu_tensors_are_refused():
    import torch
    from houv_amd import _lib
    from houv_amd.metrics import cd
    with pytest.raises(_lib.HouvHipError):
        cd()(torch.rand(1, 4, 3), torch.rand(1, 5, 3))


def test_debug_switch_table_rejects_removed_switches_and_bad_gemm_split():
    """houv_debug_set accepts only the switches that still select something, and gemm_split only the part-product counts the
    GEMM has kernels for (0, 3, 6): anything else fails with houv_last_error set instead of silently running another kernel."""
    from houv_amd import _lib
    # the retired switches, each with a value the old table accepted
    retired = {"prune": {"refresh": 4, "cap_slack": 1, "owner_walk": 1, "min_points": 300},
               "chamfer": {"direct": 1, "q": 4}, "gemm": {"4w": 1, "guarded": 1}}
    for prefix, switches in retired.items():
        for suffix, value in switches.items():
            name = f"{prefix}_{suffix}"
            with pytest.raises(_lib.HouvHipError):
                _lib.debug_set(name, value)
            assert name in _lib.last_error()
    try:
        for value in (1, 2, 4, 5):
            with pytest.raises(_lib.HouvHipError):
                _lib.debug_set("gemm_split", value)
            assert f"gemm_split = {value}" in _lib.last_error()
        for value in (0, 3, 6):
            _lib.debug_set("gemm_split", value)
    finally:
        _lib.debug_set("gemm_split", 6)
