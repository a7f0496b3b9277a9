"""CPU: what the group cull of the box tests (prune_masks: a group verdict per k, then a scalar loop over the surviving boxes) may
cost in kernel resources, read from the built library's gfx950 code objects without a device: every pruned solve_kernel
instantiation still has no scratch, no VGPR spills and at most 128 VGPRs, and houv_solve_lds_bytes is what it was -- the cull
reads the boxes that were already in LDS and adds none."""
import os

import pytest

from tests.test_kernel_resources import LIB, _kernel_metadata

# houv_solve_lds_bytes(n, n, pruned = 1) of the commit before the cull
PARENT_LDS_BYTES = {257: 20656, 320: 21680, 512: 27824, 768: 36528, 1024: 45232, 1536: 64320, 2048: 81728, 2500: 103520, 4096: 154720}


def test_every_pruned_solve_kernel_with_the_group_cull_has_no_scratch_no_spills_and_at_most_128_vgprs(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    pruned = {k: v for k, v in kernels.items() if k[3] != 0}
    shapes = {(256, 2), (256, 3), (256, 4), (512, 3), (512, 4)}
    assert {k for k in pruned} == {(b, q, m, 2) for b, q in shapes for m in (1, 4)} | {(1024, q, m, 3) for q in (3, 4) for m in (1, 4)}
    for k, f in sorted(pruned.items()):
        name = "solve_kernel<%s>" % ", ".join(map(str, k))
        print(f"{name}: {f['vgpr_count']} VGPRs, {f['vgpr_spill_count']} VGPR spills, {f['sgpr_spill_count']} SGPR spills, "
              f"{f['private_segment_fixed_size']} B of scratch")
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["vgpr_count"]) <= 128, f"{name}: {f['vgpr_count']} VGPRs"
        assert int(f["group_segment_fixed_size"]) == 0, f"{name}: static LDS besides the dynamic segment"


def test_lds_bytes_of_the_pruned_solve_are_unchanged_to_the_byte():
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    from houv_amd import _lib
    lib = _lib.load()
    for n, bytes_ in PARENT_LDS_BYTES.items():
        assert lib.houv_solve_lds_bytes(n, n, 1) == bytes_, n
