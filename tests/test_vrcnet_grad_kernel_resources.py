"""CPU: the kernels of vrcnet_grad.hip (houv_sa_attn_backward) use no scratch and keep the register and static-LDS figures
DESIGN.md section 9.14 states, read from the built library's gfx950 code objects the way test_ecg_grad_kernel_resources.py reads
ecg_grad.hip's."""
import test_ecg_grad_kernel_resources as ecg

# (VGPRs incl. AGPRs, static LDS bytes); one allocation granule of 8 registers is allowed either way
BUDGET = {"sa_attn_bw_point_kernelILi64E": (52, 1312), "sa_attn_bw_point_kernelILi128E": (78, 4736),
          "sa_attn_bw_point_kernelILi256E": (158, 17920), "sa_attn_bw_point_kernelILi512E": (282, 36864),
          "sa_attn_bw_scatter_kernelILi64E": (32, 0), "sa_attn_bw_scatter_kernelILi128E": (32, 0),
          "sa_attn_bw_scatter_kernelILi256E": (33, 0), "sa_attn_bw_scatter_kernelILi512E": (34, 0),
          "sa_attn_bw_reduce_kernelILi2E": (21, 0), "sa_attn_bw_reduce_kernelILi4E": (23, 0), "sa_attn_bw_reduce_kernelILi8E": (27, 0),
          "sa_attn_bw_reduce_kernelILi16E": (35, 0), "sa_attn_bw_fold_kernel": (8, 0)}


def test_vrcnet_grad_kernels_use_no_scratch_and_keep_their_register_and_lds_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(ecg, "BUDGET", BUDGET)                                    # _kernels collects the names of ecg.BUDGET
    kernels = ecg._kernels(tmp_path)
    assert sorted(kernels) == sorted(BUDGET), sorted(kernels)
    for name, (vgpr, lds) in BUDGET.items():
        f = kernels[name]
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert abs(int(f["vgpr_count"]) - vgpr) <= 8, f"{name}: {f['vgpr_count']} VGPRs, DESIGN states {vgpr}"
        assert int(f["group_segment_fixed_size"]) == lds, f"{name}: {f['group_segment_fixed_size']} B of LDS, DESIGN states {lds}"
