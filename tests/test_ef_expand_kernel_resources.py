"""CPU: the kernels of ef_expand.hip (houv_ef_expand, houv_ef_expand_backward) use no scratch and keep the register and static-LDS
figures DESIGN.md section 9.16 states, read from the built library's gfx950 code objects the way
test_edge_pool_kernel_resources.py reads edge_pool.hip's."""
import test_ecg_grad_kernel_resources as ecg

# (VGPRs, static LDS bytes); one allocation granule of 8 registers is allowed either way.  ILi<O>E is the
# instance for O output channels.
BUDGET = {"ef_expand_kernelILi64E": (84, 8768), "ef_expand_kernelILi128E": (88, 16960), "ef_expand_kernelILi256E": (132, 33344),
          "ef_expand_bw_kernelILi64E": (112, 13120), "ef_expand_bw_kernelILi128E": (219, 25408),
          "ef_expand_bw_kernelILi256E": (243, 49984), "ef_keys_kernel": (7, 0), "ef_pad_kernel": (23, 0), "ef_gproj_kernel": (32, 0),
          "ef_gb3_kernel": (12, 1024), "ef_fold_kernel": (6, 0)}


def test_ef_expand_kernels_use_no_scratch_and_keep_their_register_and_lds_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(ecg, "BUDGET", BUDGET)                                    # _kernels collects the names of ecg.BUDGET
    kernels = ecg._kernels(tmp_path)
    assert sorted(kernels) == sorted(BUDGET), sorted(kernels)
    for name, (vgpr, lds) in BUDGET.items():
        f = kernels[name]
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert abs(int(f["vgpr_count"]) - vgpr) <= 8, f"{name}: {f['vgpr_count']} VGPRs, DESIGN states {vgpr}"
        assert int(f["group_segment_fixed_size"]) == lds, f"{name}: {f['group_segment_fixed_size']} B of LDS, DESIGN states {lds}"
