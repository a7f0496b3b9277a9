"""CPU: what the term masks of the pruned solve may cost in kernel resources, read from the built library.

Every pruned solve_kernel instantiation (PRUNE = 2 / 3, NMET = 1 / 4) still has no scratch and at most 128 VGPRs, and the
512-thread kernel bench.py times, solve_kernel<512, 4, 4, 2> at 2048 points, still fits two workgroups into a CU's 160 KiB of
LDS with the 96 bytes of anchor state added (houv_solve_lds_bytes; the LDS of these kernels is dynamic, so it is not in the code
object's metadata)."""
import os

import pytest

from tests.test_kernel_resources import LIB, _kernel_metadata

LDS_PER_CU = 160 * 1024


def test_every_pruned_solve_kernel_has_no_scratch_and_at_most_128_vgprs(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    pruned = {k: v for k, v in kernels.items() if k[3] != 0}
    expected = {(256, 2), (256, 3), (256, 4), (512, 3), (512, 4)}
    assert {(k[0], k[1]) for k in pruned if k[3] == 2 and k[2] == 4} == expected, sorted(pruned)
    assert {(k[0], k[1]) for k in pruned if k[3] == 2 and k[2] == 1} == expected, sorted(pruned)
    assert {k for k in pruned if k[3] == 3} == {(1024, 3, 1, 3), (1024, 3, 4, 3), (1024, 4, 1, 3), (1024, 4, 4, 3)}, sorted(pruned)
    for k, f in sorted(pruned.items()):
        name = "solve_kernel<%s>" % ", ".join(map(str, k))
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["vgpr_count"]) <= 128, f"{name}: {f['vgpr_count']} VGPRs"
        assert int(f["group_segment_fixed_size"]) == 0, f"{name}: static LDS besides the dynamic segment"


def test_two_workgroups_of_the_bench_kernel_share_a_cu_in_lds():
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    from houv_amd import _lib
    lib = _lib.load()
    assert _lib.solve_variant(2048, 2048, True, with_mode=True) == (512, 4, 2)
    pruned, brute = lib.houv_solve_lds_bytes(2048, 2048, 1), lib.houv_solve_lds_bytes(2048, 2048, 0)
    assert 0 < brute < pruned and 2 * pruned <= LDS_PER_CU, (pruned, brute)
    assert pruned - brute == 2 * 128 * 16 + 2048 * 2 + 132 * 4 + 96       # boxes, sort staging, anchor state
    # the 1536-point variant shares the shape; the largest cloud of the super-tile walk fits a CU once
    assert 2 * lib.houv_solve_lds_bytes(1536, 1536, 1) <= LDS_PER_CU
    assert 0 < lib.houv_solve_lds_bytes(4096, 4096, 1) <= LDS_PER_CU
    assert lib.houv_solve_lds_bytes(4097, 4097, 1) == -1 and "4096" in _lib.last_error()
