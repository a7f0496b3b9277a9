"""CPU: the kernels of edge_pool.hip (houv_edge_pool, houv_edge_pool_backward) use no scratch and keep the register and static-LDS
figures DESIGN.md section 9.15 states, read from the built library's gfx950 code objects the way
test_vrcnet_grad_kernel_resources.py reads vrcnet_grad.hip's."""
import test_ecg_grad_kernel_resources as ecg

# (VGPRs, static LDS bytes); one allocation granule of 8 registers is allowed either way.  Lb1 is the
# vector form (16-byte accesses), Lb0 the scalar one.
BUDGET = {"edge_pool_kernelILb1E": (52, 0), "edge_pool_kernelILb0E": (45, 0), "edge_pool_bw_kernelILb1E": (45, 0),
          "edge_pool_bw_kernelILb0E": (47, 0), "edge_pool_keys_kernel": (17, 0)}


def test_edge_pool_kernels_use_no_scratch_and_keep_their_register_and_lds_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(ecg, "BUDGET", BUDGET)                                    # _kernels collects the names of ecg.BUDGET
    kernels = ecg._kernels(tmp_path)
    assert sorted(kernels) == sorted(BUDGET), sorted(kernels)
    for name, (vgpr, lds) in BUDGET.items():
        f = kernels[name]
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert abs(int(f["vgpr_count"]) - vgpr) <= 8, f"{name}: {f['vgpr_count']} VGPRs, DESIGN states {vgpr}"
        assert int(f["group_segment_fixed_size"]) == lds, f"{name}: {f['group_segment_fixed_size']} B of LDS, DESIGN states {lds}"
