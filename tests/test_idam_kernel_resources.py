"""CPU: the IDAM kernels (idam.hip) use no scratch and spill nothing, read from the built library's gfx950 code objects the way
test_deepgmr_kernel_resources.py reads the DeepGMR kernels'.  Skips when the library or the LLVM tools are absent."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import BUNDLE_MAGIC, LIB, TARGET, _tool

NAMES = ("idam_simmat_kernel", "edge_diff_kernelILi4", "edge_diff_kernelILi1")


def _kernels(tmp_path):
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    if not all(tools.values()):
        pytest.skip(f"LLVM tools not found: {[n for n, p in tools.items() if not p]}")
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


def test_idam_kernels_use_no_scratch(tmp_path):
    kernels = _kernels(tmp_path)
    assert sorted(kernels) == sorted(NAMES), sorted(kernels)
    for name, f in kernels.items():
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["sgpr_spill_count"]) == 0, f"{name}: {f['sgpr_spill_count']} SGPR spills"


def test_idam_simmat_keeps_two_waves_per_simd(tmp_path):
    """206 VGPRs (one allocation granule of 8 allowed on top: a compiler that hoists the per-channel table
    out of the column loop lands far above), i.e. two waves per SIMD, and the LDS of one workgroup leaves room for four."""
    f = _kernels(tmp_path)["idam_simmat_kernel"]
    assert int(f["vgpr_count"]) <= 208 and int(f["group_segment_fixed_size"]) <= 40 * 1024
