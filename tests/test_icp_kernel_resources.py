"""CPU: the six icp_kernel<BLOCK, Q> instantiations houv_icp_refine dispatches are in the built library's gfx950 code object, use no
scratch and spill nothing, and keep the register figures DESIGN.md section 9.1 states (read the way test_pcn_kernel_resources.py reads
the PCN kernels'); and every refusal of the host entry happens before anything touches a device."""
import os
import re
import subprocess
import sys

import pytest

import icp_host as host
from test_kernel_resources import BUNDLE_MAGIC, LIB, TARGET, _tool

KERNEL_RE = re.compile(r"icp_kernelILi(\d+)ELi(\d+)EE")
# (threads, points per lane) -> VGPRs; one allocation granule of 8 registers is allowed either way
VGPRS = {(256, 1): 64, (256, 2): 67, (256, 4): 92, (512, 4): 92, (1024, 4): 92, (1024, 8): 121}


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
            m = KERNEL_RE.search(fields.get("name", ""))
            if m:
                kernels[(int(m.group(1)), int(m.group(2)))] = fields
    return kernels


def test_all_six_icp_kernels_are_built_without_scratch(tmp_path):
    kernels = _kernels(tmp_path)
    assert sorted(kernels) == sorted(VGPRS), sorted(kernels)
    for k, f in sorted(kernels.items()):
        name = "icp_kernel<%d, %d>" % k
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["sgpr_spill_count"]) == 0, f"{name}: {f['sgpr_spill_count']} SGPR spills"
        assert int(f["group_segment_fixed_size"]) == 0, f"{name}: static LDS on top of what icp_smem_bytes asks for"
        assert int(f["max_flat_workgroup_size"]) == k[0], name


def test_icp_kernels_keep_their_register_budget(tmp_path):
    """A 1024-thread workgroup is 4 waves per SIMD: above 128 VGPRs it cannot be launched at all."""
    kernels = _kernels(tmp_path)
    for k, vgpr in VGPRS.items():
        n = int(kernels[k]["vgpr_count"])
        assert abs(n - vgpr) <= 8, f"icp_kernel<{k[0]}, {k[1]}>: {n} VGPRs, DESIGN states {vgpr}"
        if k[0] == 1024:
            assert n <= 128, f"icp_kernel<{k[0]}, {k[1]}>: {n} VGPRs"


# Child process with no visible device: the refusals of houv_icp_refine on fake, never dereferenced addresses.  Were a check
# missing, the call would fail for want of a device (another message) instead of being refused for its arguments.
_REFUSAL_CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
f = lib.houv_icp_refine
f.restype = I
f.argtypes = [P, P, I, I, I, P, F, I, F, F, P, P, P, P, P]
lib.houv_last_error.restype = ctypes.c_char_p
fake, limit = 0x10000, int(sys.argv[2])
calls = [(fake, fake, 1, 0, 64, 0.1, 30, fake), (fake, fake, 1, 64, 0, 0.1, 30, fake), (fake, fake, 1, 64, 64, 0.1, -1, fake),
         (fake, fake, 1, 64, 64, 0.0, 30, fake), (fake, fake, 1, 64, 64, -1.0, 30, fake), (fake, fake, 1, 64, 64, float("nan"), 30, fake),
         (fake, fake, -1, 64, 64, 0.1, 30, fake), (fake, fake, 1, 8193, 64, 0.1, 30, fake), (fake, fake, 1, 64, limit + 1, 0.1, 30, fake),
         (None, fake, 1, 64, 64, 0.1, 30, fake), (fake, None, 1, 64, 64, 0.1, 30, fake), (fake, fake, 1, 64, 64, 0.1, 30, None)]
for src, tgt, p, n, m, d, cap, out in calls:
    ok = f(src, tgt, p, n, m, None, d, cap, 1e-6, 1e-6, out, None, None, None, None)
    print(ok, lib.houv_last_error().decode())
print(f(None, None, 0, 64, 64, None, 0.1, 30, 1e-6, 1e-6, None, None, None, None, None), "empty batch")
"""


def test_icp_refusals_need_no_device():
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="999", ROCR_VISIBLE_DEVICES="999")
    out = subprocess.run([sys.executable, "-c", _REFUSAL_CHILD, LIB, str(host.largest_m())], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 13, lines
    for line in lines[:7]:
        assert line.startswith("0 ") and "bad argument" in line, line
    for line in lines[7:9]:
        assert line.startswith("0 ") and "too large" in line, line
    for line in lines[9:12]:
        assert line.startswith("0 ") and "null pointer" in line, line
    assert lines[12].startswith("1 "), lines[12]                      # P = 0 is not an error, and launches nothing either


def test_icp_refine_refuses_cpu_tensors_without_a_device():
    import torch
    from houv_amd import _lib, ops
    src, tgt = torch.zeros(2, 8, 3), torch.zeros(2, 9, 3)
    with pytest.raises(_lib.HouvHipError, match="CPU tensor"):
        ops.icp_refine(src, tgt, None, 0.1, 3)
