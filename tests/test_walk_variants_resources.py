"""CPU: what the walk variants of the pruned solve (box tests and walk compiled per metric set; houv::walk_variant) may cost in
kernel resources, read from the built library's gfx950 code objects without a device: every pruned solve_kernel instantiation
-- the variants live inside it, under its name -- still has no scratch, no VGPR spills and at most 128 VGPRs, and
houv_solve_lds_bytes is what it was.  The exported table is the header's."""
import os

import pytest

from tests.test_kernel_resources import LIB, _kernel_metadata

# houv_solve_lds_bytes(n, n, pruned = 1) of the commit before the walk variants: they add code, not LDS
PARENT_LDS_BYTES = {320: 21680, 512: 27824, 768: 36528, 1024: 45232, 1536: 64320, 2048: 81728, 2500: 103520, 4096: 154720}


def test_every_pruned_solve_kernel_with_walk_variants_has_no_scratch_no_spills_and_at_most_128_vgprs(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    pruned = {k: v for k, v in kernels.items() if k[3] != 0}
    shapes = {(256, 2), (256, 3), (256, 4), (512, 3), (512, 4)}
    assert {k for k in pruned} == {(b, q, m, 2) for b, q in shapes for m in (1, 4)} | {(1024, q, m, 3) for q in (3, 4) for m in (1, 4)}
    for k, f in sorted(pruned.items()):
        name = "solve_kernel<%s>" % ", ".join(map(str, k))
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["vgpr_count"]) <= 128, f"{name}: {f['vgpr_count']} VGPRs"
        assert int(f["group_segment_fixed_size"]) == 0, f"{name}: static LDS besides the dynamic segment"


def test_the_library_exports_the_headers_table_and_lds_bytes_are_unchanged():
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    from houv_amd import _lib
    from tests import walkvariants
    variant, _, _, _ = walkvariants.table()
    assert [_lib.solve_walk_variant(m) for m in range(16)] == variant
    with pytest.raises(_lib.HouvHipError):
        _lib.solve_walk_variant(16)
    lib = _lib.load()
    for n, bytes_ in PARENT_LDS_BYTES.items():
        assert lib.houv_solve_lds_bytes(n, n, 1) == bytes_, n
