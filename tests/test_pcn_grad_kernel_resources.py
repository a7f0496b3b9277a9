"""CPU: the kernels of PCN's backward pass -- the arg-max forward and the fold's backward in pcn.hip, the PointNet block's backward in
pcn_grad.hip;
DESIGN.md section 9.12 -- use no scratch and spill nothing, and keep the register and LDS figures that section states, read from
the built library's gfx950 code objects by test_pcn_kernel_resources.py's reader (its name list swapped for this file's)."""
import test_pcn_kernel_resources as forward


# (VGPRs, LDS bytes); one allocation granule of 8 registers is allowed either way
BUDGET = {"mlp2_argmax_kernelILi3ELi128ELi256": (69, 53024), "mlp2_argmax_kernelILi256ELi512ELi1024": (247, 123904),
          "tile_argmax_fold_kernel": (13, 0),
          # pcn_grad.hip (gh and gW2: 1 and 4 hidden channels per thread for H = 128 and 512)
          "pcn_bw_rows_kernel": (19, 1024), "pcn_bw_gather_kernel": (16, 0), "pcn_bw_gh_kernelILi1E": (9, 0),
          "pcn_bw_gh_kernelILi4E": (14, 0), "pcn_bw_gw2_kernelILi1E": (10, 0), "pcn_bw_gw2_kernelILi4E": (16, 0),
          "pcn_bw_fold_kernel": (6, 0), "pcn_bw_gshift_kernel": (13, 0),
          # pcn.hip, the folding stage's backward
          "pcn_fold_bw_kernel": (251, 74496), "fold_bw_sum_kernel": (17, 0), "fold_bw_chunks_kernel": (6, 0),
          "fold_bw_coarse_kernel": (10, 0), "fold_bw_transpose_kernel": (6, 0)}


def _kernels(tmp_path, monkeypatch):
    monkeypatch.setattr(forward, "NAMES", tuple(BUDGET))
    return forward._kernels(tmp_path)


def test_pcn_grad_kernels_use_no_scratch_and_keep_their_budget(tmp_path, monkeypatch):
    kernels = _kernels(tmp_path, monkeypatch)
    assert sorted(kernels) == sorted(BUDGET), sorted(kernels)
    for name, (vgpr, lds) in BUDGET.items():
        f = kernels[name]
        print(name, "VGPRs", f["vgpr_count"], "LDS", f["group_segment_fixed_size"], "SGPRs", f.get("sgpr_count"))
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["sgpr_spill_count"]) == 0, f"{name}: {f['sgpr_spill_count']} SGPR spills"
        assert abs(int(f["vgpr_count"]) - vgpr) <= 8 and int(f["vgpr_count"]) <= 256, f"{name}: {f['vgpr_count']} VGPRs, DESIGN states {vgpr}"
        assert int(f["group_segment_fixed_size"]) == lds, f"{name}: {f['group_segment_fixed_size']} B of LDS, DESIGN states {lds}"
