"""CPU: the PCN kernels (pcn.hip) use no scratch and spill nothing, and keep the register and LDS figures DESIGN.md section 9.9
states, read from the built library's gfx950 code objects the way test_idam_kernel_resources.py reads the IDAM kernels'."""
import os
import re
import subprocess

from test_kernel_resources import BUNDLE_MAGIC, LIB, TARGET, _tool

NAMES = ("mlp2_max_kernelILi3ELi128ELi256", "mlp2_max_kernelILi256ELi512ELi1024", "tile_max_fold_kernel", "pcn_fold_kernel")
# (VGPRs, LDS bytes); one allocation granule of 8 registers is allowed either way
BUDGET = {"mlp2_max_kernelILi3ELi128ELi256": (69, 53024), "mlp2_max_kernelILi256ELi512ELi1024": (249, 123904),
          "tile_max_fold_kernel": (17, 0), "pcn_fold_kernel": (199, 73728)}


def _kernels(tmp_path):
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert all(tools.values()), f"LLVM tools not found (they ship with the compiler that built the library): {[n for n, p in tools.items() if not p]}"
    fat = tmp_path / "fatbin"
    subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", LIB, str(tmp_path / "lib_copy")])
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)] + [len(data)]
    kernels = {}
    for i, (a, b) in enumerate(zip(starts, starts[1:])):
        bundle, co = tmp_path / f"bundle{i}", tmp_path / f"bundle{i}.co"
        bundle.write_bytes(data[a:b])
        subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--targets={TARGET}",
                               f"--input={bundle}", f"--output={co}"])
        notes = subprocess.check_output([tools["llvm-readelf"], "--notes", str(co)], text=True)
        for item in re.split(r"\n  - ", notes)[1:]:
            fields = dict(re.findall(r"^\s*\.([a-z_]+):\s+(\S+)\s*$", item, re.M))
            for n in NAMES:
                if n in fields.get("name", ""):
                    kernels[n] = fields
    return kernels


def test_pcn_kernels_use_no_scratch(tmp_path):
    kernels = _kernels(tmp_path)
    assert sorted(kernels) == sorted(NAMES), sorted(kernels)
    for name, f in kernels.items():
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["sgpr_spill_count"]) == 0, f"{name}: {f['sgpr_spill_count']} SGPR spills"


def test_pcn_kernels_keep_their_register_and_lds_budget(tmp_path):
    """The 64 x 1024 accumulators of the second PointNet block fill half of the 512-register file: 8 waves per CU, i.e. two per
    SIMD at <= 256 registers each, is what the kernel is built for; its LDS leaves no room for a second workgroup anyway."""
    kernels = _kernels(tmp_path)
    for name, (vgpr, lds) in BUDGET.items():
        f = kernels[name]
        assert abs(int(f["vgpr_count"]) - vgpr) <= 8 and int(f["vgpr_count"]) <= 256, f"{name}: {f['vgpr_count']} VGPRs, DESIGN states {vgpr}"
        assert int(f["group_segment_fixed_size"]) == lds, f"{name}: {f['group_segment_fixed_size']} B of LDS, DESIGN states {lds}"
