"""CPU test: the register budget of the fused loop's pruned kernels, read from the built library's gfx950 code objects.

The pruned solve_kernel<BLOCK, Q, 4, 2> variants (the product default for clouds of 257..2048 points; <512, 4, 4, 2> is
what bench.py times) run at 4 waves per SIMD with 128 VGPRs and must not spill: a spilled value is reloaded from scratch in
front of a global or LDS access on every iteration.  The metadata of every kernel is in the AMDGPU notes of the code objects
in the library's .hip_fatbin section (one offload bundle per translation unit).  Skips when the library or the LLVM tools
are absent."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "houv_amd", "lib", "libhouv_hip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNEL_RE = re.compile(r"solve_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE")

def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def _kernel_metadata(tmp_path):
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
        # one YAML list item per kernel ("  - .agpr_count: ..."); keys of interest are scalars at the item's level
        for item in re.split(r"\n  - ", notes)[1:]:
            fields = dict(re.findall(r"^\s*\.([a-z_]+):\s+(\S+)\s*$", item, re.M))
            m = KERNEL_RE.search(fields.get("name", ""))
            if m:
                kernels[tuple(int(x) for x in m.groups())] = fields
    return kernels


def test_pruned_four_argument_solve_kernels_do_not_spill(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    pruned = {k: v for k, v in kernels.items() if k[2] == 4 and k[3] == 2}
    assert (512, 4, 4, 2) in pruned and (256, 3, 4, 2) in pruned, sorted(kernels)
    for k, f in sorted(pruned.items()):
        name = "solve_kernel<%s>" % ", ".join(map(str, k))
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["vgpr_count"]) <= 128, f"{name}: {f['vgpr_count']} VGPRs (4 waves per SIMD need <= 128)"


def test_every_pruned_four_argument_solve_kernel_is_spill_free(tmp_path):
    """The rest of the pruned family -- the single-metric twins (NMET = 1) and the 1024-thread super-tile walk (PRUNE = 3) for
    2049..4096 points -- has no scratch either.  The brute-force sweeps
    (PRUNE = 0) are not checked: the one-point-per-lane variants run 8 waves per SIMD on 64 VGPRs and spill by design."""
    kernels = _kernel_metadata(tmp_path)
    others = {k: v for k, v in kernels.items() if k[3] != 0 and not (k[2] == 4 and k[3] == 2)}
    assert (1024, 4, 4, 3) in others and (512, 4, 1, 2) in others, sorted(kernels)
    for k, f in sorted(others.items()):
        name = "solve_kernel<%s>" % ", ".join(map(str, k))
        assert int(f["private_segment_fixed_size"]) == 0, f"{name}: {f['private_segment_fixed_size']} B of scratch per lane"
        assert int(f["vgpr_spill_count"]) == 0, f"{name}: {f['vgpr_spill_count']} VGPR spills"
        assert int(f["vgpr_count"]) <= 128, f"{name}: {f['vgpr_count']} VGPRs"


# Child process with no visible device: the host-side argument checks of houv_solve_iterate_pruned on fake, never dereferenced
# addresses.  Were a check missing, the launch would fail for want of a device instead of reaching one.
_ALIGN_CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
P, I, D, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
f = lib.houv_solve_iterate_pruned
f.restype = I
f.argtypes = [P, P, I, I, I, I, P, I, I, I, I, I, I, I, I, D, D, D, D, F, P, P, P, P, P, P, P, I, I, P]
lib.houv_last_error.restype = ctypes.c_char_p
fake, N = 0x10000, 600
for nn_ws, stride in ((fake + 8, 600), (fake + 8, 601)):
    ok = f(fake, fake, 1, N, N, 1, fake, 0, 1, 0, 0, 1, 0, N // 2, N, 0.01, 0.9, 0.999, 1e-8, 1.0,
           None, None, None, None, None, None, nn_ws, 0, stride, None)
    print(ok, lib.houv_last_error().decode())
"""


def test_pruned_workspace_must_be_16_byte_aligned():
    """houv_solve_iterate_pruned reads a query's NN record as one 8-byte load and its minima record as one 16-byte load, so it
    refuses an nn_ws base that is not 16-byte aligned, on the host, before any launch."""
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="999", ROCR_VISIBLE_DEVICES="999")
    out = subprocess.run([sys.executable, "-c", _ALIGN_CHILD, LIB], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    aligned, stride = out.stdout.strip().splitlines()
    assert aligned.startswith("0 ") and "16-byte aligned" in aligned, aligned
    assert stride.startswith("0 ") and "multiple of 8" in stride, stride        # the stride check comes first
