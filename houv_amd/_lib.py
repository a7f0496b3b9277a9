"""ctypes binding of libhouv_hip.so (include/houv_hip.h).

There is NO fallback: if the HIP library is missing or a call fails, this raises.  The oracle under
``oracle/`` is never imported from here.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# HOUV_HIP_LIB lets the A/B scripts load another build of the library; the default is the product library
LIB_PATH = os.environ.get("HOUV_HIP_LIB") or os.path.join(_HERE, "lib", "libhouv_hip.so")
ABI_VERSION = 2

_c_f = ctypes.c_void_p     # device pointers travel as plain addresses
_int = ctypes.c_int
_dbl = ctypes.c_double
_flt = ctypes.c_float

# the fused solve's entries: 26 common arguments (clouds, sizes, state, iteration window, switches, top-k sizes, Adam constants,
# loss scale, six outputs), then the pruned search's workspace (nn_ws, ws_valid, stride) and / or the stage's schedule
# (chunk_iters, sched_ws) as the entry has them, then the stream
_SOLVE_COMMON = [_c_f, _c_f, _int, _int, _int, _int, _c_f, _int, _int, _int, _int, _int, _int, _int, _int, _dbl, _dbl, _dbl, _dbl,
                 _flt, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]
_SOLVE_WS = [_c_f, _int, _int]
_SOLVE_SCHED = [_int, _c_f]

_SIGNATURES = {
    "houv_abi_version": (ctypes.c_int, []),
    "houv_last_error": (ctypes.c_char_p, []),
    "houv_build_id": (ctypes.c_char_p, []),
    "houv_debug_set": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_longlong]),
    "houv_chamfer_forward": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    "houv_chamfer_backward": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    "houv_kabsch": (ctypes.c_int, [_c_f, _c_f, _c_f, _int, _int, _c_f, _c_f, _c_f]),
    "houv_solve_iterate": (ctypes.c_int, _SOLVE_COMMON + [_c_f]),
    "houv_solve_iterate_large": (ctypes.c_int, _SOLVE_COMMON + [_c_f]),
    "houv_solve_iterate_pruned": (ctypes.c_int, _SOLVE_COMMON + _SOLVE_WS + [_c_f]),
    "houv_solve_stage": (ctypes.c_int, _SOLVE_COMMON + _SOLVE_SCHED + [_c_f]),
    "houv_solve_stage_pruned": (ctypes.c_int, _SOLVE_COMMON + _SOLVE_WS + _SOLVE_SCHED + [_c_f]),
    "houv_solve_seed": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _int, _c_f, _int, _int, _int, _c_f, _int, _c_f]),
    "houv_solve_variant": (ctypes.c_int, [_int, _int, _int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int)]),
    "houv_solve_lds_bytes": (ctypes.c_longlong, [_int, _int, _int]),
    "houv_solve_walk_variant": (ctypes.c_int, [_int]),
    "houv_kd_sort": (ctypes.c_int, [_c_f, _int, _int, _int, _int, _c_f, _c_f, _c_f]),
    "houv_icp_refine": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _c_f, _flt, _int, _flt, _flt, _c_f, _c_f, _c_f, _c_f, _c_f]),
    "houv_knn": (ctypes.c_int, [_c_f, _int, _int, _int, _c_f, _c_f]),
    "houv_edgeconv1": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    "houv_max_over_k": (ctypes.c_int, [_c_f, ctypes.c_longlong, _int, _int, _c_f, _int, _c_f]),
    "houv_gemm_f32": (ctypes.c_int, [_c_f, _c_f, _c_f, _int, _int, _int, _int, _int, _int, _int, _int, _int] +
                      [ctypes.c_longlong] * 6 + [_flt, _c_f, _c_f, _c_f, _int, ctypes.c_longlong, ctypes.c_longlong,
                                                 _int, _c_f]),
    "houv_attention_f32": (ctypes.c_int, [_c_f, _c_f, _c_f, _c_f, _int, _int, _int, _int, _int, _int, _int, _int, _int] +
                           [ctypes.c_longlong] * 4 + [_flt, _c_f]),
    "houv_layernorm": (ctypes.c_int, [_c_f, ctypes.c_longlong, _int, _c_f, _c_f, _flt, _c_f, _c_f, _c_f]),
    "houv_softmax_rows": (ctypes.c_int, [_c_f, ctypes.c_longlong, _int, _c_f]),
    "houv_softmax_corr": (ctypes.c_int, [_c_f, _int, _int, _int, _c_f, _c_f, _c_f]),
    "houv_furthest_point_sample": (ctypes.c_int, [_c_f, _int, _int, _int, _c_f, _c_f]),
    "houv_knn_cross": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _int, _c_f, _c_f, _c_f]),
    "houv_gather_points": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _int, _c_f, _c_f]),
    "houv_ball_query": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _flt, _flt, _int, _c_f, _c_f, _c_f]),
    "houv_three_interpolate": (ctypes.c_int, [_c_f, _c_f, _c_f, _int, _int, _int, _int, _c_f, _c_f]),
    "houv_scatter_points_grad": (ctypes.c_int, [_c_f, _c_f, _c_f, _int, _int, _int, _int, _int, _c_f, _c_f, _c_f]),
    "houv_scatter_points_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int]),
    "houv_emd_forward": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _flt, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    "houv_emd_workspace_bytes": (ctypes.c_longlong, [_int, _int]),
    "houv_emd_backward": (ctypes.c_int, [_c_f, _c_f, _int, _int, _c_f, _c_f, _c_f, _c_f]),
    "houv_rri_features": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _int, _int, _c_f, _c_f]),
    "houv_gmm_params": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f, _c_f]),
    "houv_gmm_register": (ctypes.c_int, [_c_f, _c_f, _c_f, _c_f, _int, _int, _c_f, _c_f]),
    "houv_gmm_params_backward": (ctypes.c_int, [_c_f] * 8 + [_int, _int, _int, _c_f, _c_f]),
    "houv_gmm_register_backward": (ctypes.c_int, [_c_f] * 5 + [_int, _int] + [_c_f] * 5),
    "houv_bn_rows_workspace_bytes": (ctypes.c_longlong, [ctypes.c_longlong, _int, _int]),
    "houv_bn_rows_stats": (ctypes.c_int, [_c_f, ctypes.c_longlong, _int, ctypes.c_longlong, _c_f, _c_f, _c_f, ctypes.c_longlong, _c_f]),
    "houv_bn_relu_rows": (ctypes.c_int, [_c_f, ctypes.c_longlong, _int, ctypes.c_longlong, _c_f, _c_f, _c_f, _c_f, _flt, _int, _int,
                                         _c_f, ctypes.c_longlong, _c_f, _c_f, _c_f, ctypes.c_longlong, _c_f]),
    "houv_bn_relu_rows_backward": (ctypes.c_int, [_c_f, ctypes.c_longlong, _c_f, ctypes.c_longlong, _int, ctypes.c_longlong, _c_f, _c_f,
                                                  _c_f, _c_f, _flt, _int, _c_f, ctypes.c_longlong, _c_f, _c_f, _c_f, ctypes.c_longlong,
                                                  _c_f]),
    "houv_idam_simmat": (ctypes.c_int, [_c_f] * 4 + [_int] * 4 + [_c_f] * 15),
    "houv_edge_diff": (ctypes.c_int, [_c_f, _c_f, _int, _int, _int, _int, _int, _int, _c_f, _c_f]),
    "houv_mlp2_max": (ctypes.c_int, [_c_f, _int, _int, _int, _c_f, _int, _c_f, ctypes.c_longlong, _c_f, _c_f, _int, _c_f, _c_f, _c_f, _c_f]),
    "houv_mlp2_max_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int]),
    "houv_mlp2_max_arg": (ctypes.c_int, [_c_f, _int, _int, _int, _c_f, _int, _c_f, ctypes.c_longlong, _c_f, _c_f, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    "houv_mlp2_max_arg_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int]),
    "houv_mlp2_max_backward": (ctypes.c_int, [_c_f, _int, _int, _int, _c_f, _int, _c_f, ctypes.c_longlong, _c_f, _int, _c_f, _c_f,
                                              _c_f, _c_f, _c_f, _int] + [_c_f] * 9),
    "houv_mlp2_max_backward_workspace_bytes": (ctypes.c_longlong, [_int] * 6),
    "houv_mlp2_max_backward_rows": (ctypes.c_int, [_int, _int, _int]),
    "houv_pcn_fold": (ctypes.c_int, [_c_f, _c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    "houv_pcn_fold_backward": (ctypes.c_int, [_c_f, _c_f, _c_f, _int, _int, _int] + [_c_f] * 14 + [ctypes.c_longlong, _c_f]),
    "houv_pcn_fold_backward_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int]),
    "houv_knn_feat": (ctypes.c_int, [_c_f, _int, _int, _int, _int, _int, _c_f, _c_f, _c_f]),
    "houv_dense_conv": (ctypes.c_int, [_c_f, _int, _c_f, _int, _int, _int, _int] + [_c_f] * 6 + [_int, _c_f, _int, _c_f]),
    "houv_dense_conv_arg": (ctypes.c_int, [_c_f, _int, _c_f, _int, _int, _int, _int] + [_c_f] * 6 + [_int, _c_f, _int, _c_f, _c_f]),
    "houv_dense_conv_backward": (ctypes.c_int, [_c_f, _int, _c_f, _int, _int, _int, _int] + [_c_f] * 6 +
                                 [_int, _c_f, _c_f, _int, _c_f, _int, _c_f, _int] + [_c_f] * 7 + [ctypes.c_longlong, _c_f]),
    "houv_dense_conv_backward_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int, _int]),
    "houv_sa_attn": (ctypes.c_int, [_c_f, _int, _c_f, _int, _c_f, _int, _int, _int, _int] + [_c_f] * 5 + [_int, _c_f, _int, _c_f]),
    "houv_sa_attn_backward": (ctypes.c_int, [_c_f, _int, _c_f, _int, _int, _int, _int, _c_f, _c_f, _c_f, _c_f, _int, _c_f, _int, _c_f, _int,
                                             _c_f, _c_f, _c_f, _c_f, ctypes.c_longlong, _c_f]),
    "houv_sa_attn_backward_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int, _int]),
    "houv_edge_pool": (ctypes.c_int, [_c_f, _int, _c_f, _c_f, _int, _int, _int, _int, _int, _c_f, _int, _c_f, _c_f]),
    "houv_edge_pool_backward": (ctypes.c_int, [_c_f, _int, _c_f, _c_f, _c_f, _int, _int, _int, _int, _int, _c_f, _int, _c_f,
                                               ctypes.c_longlong, _c_f]),
    "houv_edge_pool_backward_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int, _int]),
    "houv_ef_expand": (ctypes.c_int, [_c_f, _int, _c_f, _int, _int, _int, _int, _int, _c_f, _int, _c_f, _c_f, _c_f, _int, _c_f, _c_f]),
    "houv_ef_expand_backward": (ctypes.c_int, [_c_f, _int, _c_f, _c_f, _int, _int, _int, _int, _int, _c_f, _int, _c_f, _c_f, _int, _c_f,
                                               _int, _c_f, _c_f, _c_f, _c_f, ctypes.c_longlong, _c_f]),
    "houv_ef_expand_backward_workspace_bytes": (ctypes.c_longlong, [_int] * 5),
    "houv_cd_loss_backward": (ctypes.c_int, [_c_f] * 8 + [_int, _int, _int, _c_f, _c_f, ctypes.c_longlong, _c_f]),
    "houv_cd_loss_backward_workspace_bytes": (ctypes.c_longlong, [_int, _int, _int]),
    "houv_pose_forward": (ctypes.c_int,[_c_f, _int, _int, _int, _c_f, _int, _c_f, _c_f, _c_f, _c_f]),
}


def _addresses(kinds):
    """A function compiled for one entry: its arguments in, the same out with the tensors of the pointer slots as addresses.
    Generated source, not a loop over the pointer slots' indices: on a stub library the loop cost houv_knn's launch 2.96 us
    against 2.7 us for this form and 2.5 us for the four inline lines it replaces, and this form is the one whose per-call and
    bench.py figures lie inside the parent's spread (profiles/r17_ops_call_path.txt)."""
    names = [f"a{i}" for i in range(len(kinds))]
    items = [f"{n} if {n} is None else {n}.data_ptr()" if k is None else n for n, k in zip(names, kinds)]
    return eval(f"lambda {', '.join(names)}: ({', '.join(items)},)")


# What `call` needs of every launching entry, worked out once: the kind of each slot before the stream (None: pointer, int,
# float) and the entry's _addresses.  INVARIANT of _SIGNATURES: an entry launches if and only if its last slot is a c_void_p,
# and that slot is the stream; size and variant queries end in a scalar or a typed POINTER and are called directly.
_SLOTS = {}
for _name, (_, _args) in _SIGNATURES.items():
    if _args and _args[-1] is _c_f:
        _kinds = tuple(None if c is _c_f else float if c in (_flt, _dbl) else int for c in _args[:-1])
        _SLOTS[_name] = (_kinds, _addresses(_kinds))
_PLAIN = frozenset((int, float, bool, type(None)))      # what ctypes converts by itself once the tensors are addresses

_lib = None


class HouvHipError(RuntimeError):
    pass


def exported_symbols():
    return sorted(_SIGNATURES)


def load():
    """Load libhouv_hip.so once; raise (never fall back) when it is absent or ABI-mismatched."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HouvHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C houv_amd/csrc`). houv_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = symbol missing from the build
        fn.restype = res
        fn.argtypes = args
    if lib.houv_abi_version() != ABI_VERSION:
        raise HouvHipError(f"libhouv_hip.so ABI {lib.houv_abi_version()} != expected {ABI_VERSION}")
    _lib = lib
    return lib


def solve_variant(N, M, pruned=False, with_mode=False):
    """(threads per workgroup, points per lane[, prune mode]) of the solve_kernel that serves clouds of N and M points."""
    b, q, m = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(load().houv_solve_variant(int(N), int(M), int(bool(pruned)), ctypes.byref(b), ctypes.byref(q), ctypes.byref(m)),
          "houv_solve_variant")
    return (b.value, q.value, m.value) if with_mode else (b.value, q.value)


def solve_walk_variant(need):
    """The compiled metric set (4 bits) that a pruned sweep with term mask `need` (0..15) runs on (houv_solve_walk_variant)."""
    v = load().houv_solve_walk_variant(int(need))
    if v < 0:
        raise HouvHipError(f"houv_solve_walk_variant failed: {last_error()}")
    return v


def build_id():
    """Hash of the sources the loaded library was built from (houv_build_id)."""
    return load().houv_build_id().decode()


def debug_set(name, value):
    """Diagnostic switch of the library (houv_debug_set; see houv_amd/csrc/houv_common.h `DebugKnobs`)."""
    check(load().houv_debug_set(name.encode(), int(value)), "houv_debug_set")


def last_error():
    return load().houv_last_error().decode("utf-8", "replace")


def check(ok, what):
    if ok != 1:
        raise HouvHipError(f"{what} failed: {last_error()}")


def ptr(t):
    """Device address of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_of(t):
    """The torch current stream of t's device as a raw hipStream_t."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def call(name, on, *args):
    """Launch entry `name` on the torch current stream of tensor `on`'s device and check its result.  Each argument is converted
    by its slot's type in _SIGNATURES: a pointer slot takes a tensor (its address), None (NULL) or a c_void_p; an integer slot
    int() (True / False arrive as 1 / 0; a value with a fraction is refused); a float slot float().  The stream is appended
    here.  This is the host cost of every launch, so the usual case -- tensors or None in the pointer slots, plain Python
    numbers elsewhere -- touches the pointer slots only and leaves the numbers to ctypes; anything else takes _checked."""
    kinds, addresses = _SLOTS[name]
    if len(args) != len(kinds):
        raise TypeError(f"{name}: takes {len(kinds)} arguments before the stream, got {len(args)}")
    try:
        conv = addresses(*args)
        if not _PLAIN.issuperset(map(type, conv)):      # a tensor in a scalar slot, a numpy number, a c_void_p, ...
            conv = _checked(name, kinds, args)
    except AttributeError:                              # something else than a tensor in a pointer slot
        conv = _checked(name, kinds, args)
    fn = getattr(_lib or load(), name)
    with torch.cuda.device(on.device):
        stream = stream_of(on)
        try:
            ok = fn(*conv, stream)
        except ctypes.ArgumentError:                    # a float in an integer slot
            ok = fn(*_checked(name, kinds, args), stream)
    if ok != 1:
        check(ok, name)


def _checked(name, kinds, args):
    """call's arguments converted one by one, every refusal naming the entry and the slot."""
    conv = []
    for i, (kind, a) in enumerate(zip(kinds, args)):
        if kind is None:
            if isinstance(a, torch.Tensor):
                a = a.data_ptr()
            elif a is not None and not isinstance(a, ctypes.c_void_p):
                raise TypeError(f"{name}: argument {i} is a pointer: expected a tensor, None or a c_void_p, got {type(a).__name__}")
        elif isinstance(a, torch.Tensor):
            raise TypeError(f"{name}: argument {i} is a scalar ({kind.__name__}), got a tensor")
        elif kind is int and int(a) != a:
            raise TypeError(f"{name}: argument {i} is an integer, got {a!r}")
        else:
            a = kind(a)
        conv.append(a)
    return conv


def workspace(bytes_entry, device, *dims, floor=16):
    """(workspace, nbytes) for the size query `bytes_entry`(*dims): a fresh uint8 allocation of max(nbytes, floor) bytes.
    floor=0 is what selects NULL: the allocation is then exactly nbytes, and None (the library's NULL) when the query says 0;
    with the default floor there is always an allocation.  nbytes is what the query returned: the figure the entries that
    take one are told."""
    nbytes = getattr(load(), bytes_entry)(*map(int, dims))
    size = max(nbytes, floor)
    return (torch.empty(size, dtype=torch.uint8, device=device) if size > 0 else None), nbytes


def require_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HouvHipError("houv_amd ops run on an MI355X only: got a CPU tensor (there is no CPU fallback)")
        if not t.is_contiguous():
            raise HouvHipError("houv_amd ops need contiguous tensors")
    dev = [t.device for t in tensors if t is not None]
    if any(d != dev[0] for d in dev):
        raise HouvHipError("all tensors must live on the same device")


def require_gpu_any(*tensors):
    """Like require_gpu but allows strided (row-major, inner-contiguous) views."""
    ts = [t for t in tensors if t is not None]
    for t in ts:
        if not t.is_cuda:
            raise HouvHipError("houv_amd ops run on an MI355X only: got a CPU tensor (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise HouvHipError(f"expected float32, got {t.dtype}")
    if any(t.device != ts[0].device for t in ts):
        raise HouvHipError("all tensors must live on the same device")
