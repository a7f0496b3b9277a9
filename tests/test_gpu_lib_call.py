"""GPU: houv_amd._lib.call, the one place the Python bindings launch from.  A recording proxy stands in for the loaded library
where the arguments are what is checked (nothing is launched there); the refusal is the library's own, made on the host before
any launch.  Cloud [1, 8, 3]."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


class _Recorder:
    """Stands in for the ctypes library: every entry is a ctypes callback of the entry's real signature that records
    (name, arguments as the C side receives them: addresses as int, NULL as None) and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        from houv_amd import _lib
        res, argtypes = _lib._SIGNATURES[name]

        def entry(*args):
            self.calls.append((name, args))
            return 1
        fn = ctypes.CFUNCTYPE(res, *argtypes)(entry)
        setattr(self, name, fn)                                            # keeps the callback alive
        return fn


@pytest.fixture
def cloud():
    g = torch.Generator().manual_seed(8)
    return torch.rand(1, 8, 3, generator=g).cuda()


@pytest.fixture
def recorder(monkeypatch):
    from houv_amd import _lib
    _lib.load()
    rec = _Recorder()
    monkeypatch.setattr(_lib, "_lib", rec)
    return rec


def _stream(a):
    """A recorded stream argument as torch names it: the default stream is NULL there and 0 here."""
    return a or 0


def test_wrapper_passes_addresses_null_and_the_current_stream(cloud, recorder):
    from houv_amd import ops
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = ops.kd_sort(cloud)
        out2, order = ops.kd_sort(cloud, leaf=4, rule="extent", return_order=True)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    (n1, a1), (n2, a2) = recorder.calls
    assert n1 == n2 == "houv_kd_sort"
    assert a1[6] is None                                               # the optional output left out: NULL
    assert a1 == (cloud.data_ptr(), 1, 8, 32, 0, out.data_ptr(), None, s.cuda_stream)
    assert a2 == (cloud.data_ptr(), 1, 8, 4, 1, out2.data_ptr(), order.data_ptr(), s.cuda_stream)
    ops.kd_sort(cloud)                                                 # outside the block: the default stream again
    assert _stream(recorder.calls[2][1][-1]) == torch.cuda.current_stream().cuda_stream


def test_call_converts_by_slot_type(cloud, recorder):
    from houv_amd import _lib
    idx = torch.empty((1, 8, 2), dtype=torch.int32, device=cloud.device)
    given = ctypes.c_void_p(idx.data_ptr())
    # houv_ball_query: xyz, centres, B, N, M, float min_radius, float max_radius, int sample_num, idx, count
    _lib.call("houv_ball_query", cloud, cloud, cloud, True, 8, 8, 0, 1, 2.0, given, None)
    (name, args), = recorder.calls
    assert name == "houv_ball_query" and len(args) == 11
    assert args[2] == 1 and type(args[2]) is int                       # True -> 1
    assert (args[5], args[6]) == (0.0, 1.0) and type(args[5]) is float and type(args[6]) is float
    assert args[7] == 2 and type(args[7]) is int                       # 2.0 -> 2
    assert args[8] == idx.data_ptr() and args[9] is None               # a c_void_p passes through
    assert args[0] == cloud.data_ptr() and _stream(args[10]) == torch.cuda.current_stream().cuda_stream
    import numpy as np
    _lib.call("houv_ball_query", cloud, cloud, cloud, np.int64(1), np.int32(8), 8, np.float32(0.5), 1, 2, idx, None)
    args = recorder.calls[1][1]
    assert args[2:8] == (1, 8, 8, 0.5, 1.0, 2) and [type(a) for a in args[2:8]] == [int, int, int, float, float, int]


def test_library_refusal_carries_its_message_and_the_entry(cloud):
    from houv_amd import _lib, ops
    with pytest.raises(_lib.HouvHipError) as e:
        ops.kd_sort(cloud, leaf=0)                                     # refused on the host, before any launch
    assert str(e.value) == "houv_kd_sort failed: houv_kd_sort: leaf must be >= 1 (got 0)"


def test_misplaced_arguments_never_reach_the_library(cloud, recorder):
    from houv_amd import _lib
    out = torch.empty_like(cloud)
    good = (cloud, 1, 8, 32, 0, out, None)
    with pytest.raises(TypeError, match=r"houv_kd_sort: argument 2 is a scalar \(int\), got a tensor"):
        _lib.call("houv_kd_sort", cloud, cloud, 1, torch.tensor(8), 32, 0, out, None)
    with pytest.raises(TypeError, match=r"houv_kd_sort: argument 5 is a pointer: expected a tensor, None or a c_void_p, got float"):
        _lib.call("houv_kd_sort", cloud, cloud, 1, 8, 32, 0, 1.5, None)
    with pytest.raises(TypeError, match=r"houv_kd_sort: argument 2 is a scalar \(int\), got a tensor"):
        _lib.call("houv_kd_sort", cloud, cloud, 1, torch.tensor(8, device=cloud.device), 32, 0, out, None)
    with pytest.raises(TypeError, match=r"houv_kd_sort: argument 3 is an integer, got 2.7"):
        _lib.call("houv_kd_sort", cloud, cloud, 1, 8, 2.7, 0, out, None)
    with pytest.raises(TypeError, match=r"houv_kd_sort: argument 0 is a pointer: expected a tensor, None or a c_void_p, got int"):
        _lib.call("houv_kd_sort", cloud, cloud.data_ptr(), 1, 8, 32, 0, out, None)
    with pytest.raises(TypeError, match=r"houv_kd_sort: takes 7 arguments before the stream, got 6"):
        _lib.call("houv_kd_sort", cloud, *good[:-1])
    with pytest.raises(TypeError, match=r"houv_kd_sort: takes 7 arguments before the stream, got 8"):
        _lib.call("houv_kd_sort", cloud, *good, None)
    assert recorder.calls == []
    _lib.call("houv_kd_sort", cloud, *good)
    assert len(recorder.calls) == 1
