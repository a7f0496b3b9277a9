"""CPU: houv_kd_sort (the device-side k-d leaf sort) is declared, exported and bound; it refuses every bad argument on the host,
before any launch; its kernel runs without scratch inside the 1024-thread register budget."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from tests.test_kernel_resources import BUNDLE_MAGIC, LIB, TARGET, _tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library():
    from houv_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_kd_sort_is_declared_exported_and_bound():
    _lib = _library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "houv_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+houv_kd_sort\s*\(\s*const float\s*\*\s*xyz,\s*int P,\s*int N,\s*int leaf,\s*int rule,\s*"
                     r"float\s*\*\s*out,\s*int32_t\s*\*\s*order_or_null,\s*void\s*\*\s*stream\s*\)", header)
    assert "houv_kd_sort" in _lib.exported_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "houv_kd_sort")
    fn = _lib.load().houv_kd_sort
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert _lib.load().houv_abi_version() == _lib.ABI_VERSION == 2          # additive: the ABI version stays


# Child process with no visible device: every call below must be refused by the host-side checks on fake, never dereferenced
# addresses.  Were a check missing, the call would fail for want of a device (another message) instead.
_ARGS_CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
P, I = ctypes.c_void_p, ctypes.c_int
f = lib.houv_kd_sort
f.restype = I
f.argtypes = [P, I, I, I, I, P, P, P]
lib.houv_last_error.restype = ctypes.c_char_p
x, o = 0x10000, 0x100000
for args in ((x, 1, 0, 32, 0, o), (x, 1, 4097, 32, 0, o), (x, 1, 600, 0, 0, o), (x, 1, 600, 32, 2, o), (x, 1, 600, 32, 0, None), (x, 0, 600, 32, 3, o),
             (x, 1, 600, 32, 0, x), (x, 1, 600, 32, 1, x + 12 * 599), (None, 1, 600, 32, 0, o), (x, -1, 600, 32, 0, o)):
    print(f(*args, None, None), lib.houv_last_error().decode())
"""


def test_kd_sort_rejects_bad_arguments_before_any_launch():
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="999", ROCR_VISIBLE_DEVICES="999")
    out = subprocess.run([sys.executable, "-c", _ARGS_CHILD, LIB], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    expect = ["bad shape P=1 N=0", "bad shape P=1 N=4097", "leaf must be >= 1", "unknown rule 2", "null pointer", "unknown rule 3",
              "out overlaps xyz", "out overlaps xyz", "null pointer", "bad shape P=-1"]
    assert len(lines) == len(expect), out.stdout
    for line, msg in zip(lines, expect):
        assert line.startswith("0 houv_kd_sort: ") and msg in line, (line, msg)


def _kernel_metadata(tmp_path, pattern):
    """AMDGPU metadata of every kernel whose name matches ``pattern``, from the library's gfx950 code objects (the method of
    tests/test_kernel_resources.py::_kernel_metadata)."""
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
            if pattern.search(fields.get("name", "")):
                kernels[fields["name"]] = fields
    return kernels


def test_kd_sort_kernel_has_no_scratch_and_fits_1024_threads(tmp_path):
    kernels = _kernel_metadata(tmp_path, re.compile(r"kd_sort_kernel"))
    assert len(kernels) == 1, sorted(kernels)
    f = next(iter(kernels.values()))
    assert int(f["private_segment_fixed_size"]) == 0, f"{f['private_segment_fixed_size']} B of scratch per lane"
    assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0
    assert int(f["vgpr_count"]) <= 128, f"{f['vgpr_count']} VGPRs (1024 threads = 4 waves per SIMD need <= 128)"
    assert int(f["max_flat_workgroup_size"]) == 1024
    assert int(f["group_segment_fixed_size"]) <= 160 * 1024
