"""CPU: the kernels of houv_cd_loss_backward (cd_loss.hip's cd_loss_bw_kernel and the clamping form of the counting sort it shares
with houv_scatter_points_grad) use no scratch and keep the register and static-LDS figures DESIGN.md section 9.17 states, read
from the built library's gfx950 code objects the way test_edge_pool_kernel_resources.py reads edge_pool.hip's."""
import test_ecg_grad_kernel_resources as ecg

# (VGPRs, static LDS bytes); one allocation granule of 8 registers is allowed either way.  The sort's
# LDS is its 8192 cursors and 16 wave totals; Lb1 is the form that clamps its keys.
BUDGET = {"cd_loss_bw_kernel": (59, 0), "scatter_index_kernelILb1E": (50, 32832)}


def test_cd_loss_kernels_use_no_scratch_and_keep_their_register_and_lds_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(ecg, "BUDGET", BUDGET)                                    # _kernels collects the names of ecg.BUDGET
    kernels = ecg._kernels(tmp_path)
    assert sorted(kernels) == sorted(BUDGET), sorted(kernels)
    for name, (vgpr, lds) in BUDGET.items():
        f = kernels[name]
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert abs(int(f["vgpr_count"]) - vgpr) <= 8, f"{name}: {f['vgpr_count']} VGPRs, DESIGN states {vgpr}"
        assert int(f["group_segment_fixed_size"]) == lds, f"{name}: {f['group_segment_fixed_size']} B of LDS, DESIGN states {lds}"
