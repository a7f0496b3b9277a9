"""CPU: the four instantiations of solve_seed_kernel (houv_solve_seed, csrc/solve_seed.hip) use no scratch, spill nothing and
stay within the registers of eight waves per SIMD, read from the built library's gfx950 code objects the way
test_cd_loss_kernel_resources.py reads cd_loss.hip's.  Their LDS is dynamic (both clouds and their boxes), so the static figure
is 0."""
import test_ecg_grad_kernel_resources as ecg

# <threads per workgroup, metrics>: (VGPRs the compiler reports today); what is asserted is the occupancy bound of 64
KERNELS = {"solve_seed_kernelILi512ELi4E": 33, "solve_seed_kernelILi512ELi1E": 43, "solve_seed_kernelILi1024ELi4E": 33,
           "solve_seed_kernelILi1024ELi1E": 43}


def test_solve_seed_kernels_use_no_scratch_and_spill_nothing(tmp_path, monkeypatch):
    monkeypatch.setattr(ecg, "BUDGET", KERNELS)                                   # _kernels collects the names of ecg.BUDGET
    kernels = ecg._kernels(tmp_path)
    assert sorted(kernels) == sorted(KERNELS), sorted(kernels)
    for name in KERNELS:
        f = kernels[name]
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, name
        assert int(f["vgpr_count"]) <= 64, f"{name}: {f['vgpr_count']} VGPRs, eight waves per SIMD need <= 64"
        assert int(f["group_segment_fixed_size"]) == 0, f"{name}: {f['group_segment_fixed_size']} B of static LDS"
