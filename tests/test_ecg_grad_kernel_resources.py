"""CPU: the kernels of ecg_grad.hip (houv_dense_conv_arg, houv_dense_conv_backward) use no scratch and keep the register and
static-LDS figures DESIGN.md section 9.13 states, read from the built library's gfx950 code objects the way
test_ecg_kernel_resources.py reads the forward kernels'.  The edge and point kernels of the backward take their LDS dynamically
(123584 / 75776 B at C = 48, above the 64 KB a static allocation may have), so their static figure is 0."""
import os
import re
import subprocess

from test_kernel_resources import BUNDLE_MAGIC, LIB, TARGET, _tool

# (VGPRs, static LDS bytes); one allocation granule of 8 registers is allowed either way
BUDGET = {"dense_conv_arg_kernelILi24E": (321, 16416), "dense_conv_arg_kernelILi48E": (344, 25632),
          "dense_conv_bw_edge_kernelILi24E": (308, 0), "dense_conv_bw_edge_kernelILi48E": (348, 0),
          "dense_conv_bw_point_kernelILi24E": (182, 0), "dense_conv_bw_point_kernelILi48E": (246, 0),
          "dense_conv_bw_fold_kernel": (6, 0)}


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
            for n in BUDGET:
                if n in fields.get("name", ""):
                    kernels[n] = fields
    return kernels


def test_ecg_grad_kernels_use_no_scratch_and_keep_their_register_and_lds_budget(tmp_path):
    kernels = _kernels(tmp_path)
    assert sorted(kernels) == sorted(BUDGET), sorted(kernels)
    for name, (vgpr, lds) in BUDGET.items():
        f = kernels[name]
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert abs(int(f["vgpr_count"]) - vgpr) <= 8, f"{name}: {f['vgpr_count']} VGPRs, DESIGN states {vgpr}"
        assert int(f["group_segment_fixed_size"]) == lds, f"{name}: {f['group_segment_fixed_size']} B of LDS, DESIGN states {lds}"
