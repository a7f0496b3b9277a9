"""CPU: the DeepGMR training kernels (bn_rows.hip, and the two backward kernels of rri.hip) use no scratch and spill nothing, read
from the built library's gfx950 code objects the way test_deepgmr_kernel_resources.py reads the forward kernels'.  Skips when the
library or the LLVM tools are absent."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import BUNDLE_MAGIC, LIB, TARGET, _tool

# every instantiation (VEC = 4 and VEC = 1) of a templated kernel is checked: the mangled names all contain the plain name
NAMES = ("bn_stats_chunk_kernel", "bn_stats_combine_kernel", "bn_relu_rows_kernel", "bn_max_combine_kernel", "bn_bwd_sums_kernel",
         "bn_bwd_combine_kernel", "bn_bwd_apply_kernel", "gmm_params_bwd_kernel", "gmm_register_bwd_kernel")
TEMPLATED = ("bn_stats_chunk_kernel", "bn_relu_rows_kernel", "bn_bwd_sums_kernel", "bn_bwd_apply_kernel")


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
                    kernels.setdefault(n, []).append(fields)
    return kernels


def test_deepgmr_grad_kernels_use_no_scratch(tmp_path):
    kernels = _kernels(tmp_path)
    assert sorted(kernels) == sorted(NAMES), sorted(kernels)
    for name, variants in kernels.items():
        assert len(variants) == (2 if name in TEMPLATED else 1), f"{name}: {len(variants)} instantiations"
        for f in variants:
            assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
            assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
            assert int(f["sgpr_spill_count"]) == 0, f"{name}: {f['sgpr_spill_count']} SGPR spills"
            print(name, f.get("name"), "vgpr", f.get("vgpr_count"), "sgpr", f.get("sgpr_count"), "lds",
                  f.get("group_segment_fixed_size"))
