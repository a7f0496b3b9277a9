"""Cost of one binding call: wall time per call of ops.knn on a [1,64,3] cloud and of ops.solve_iterate_out on its cheapest
launch (one pair, one hypothesis, 64 points, n_iters = 1; the entry refuses n_iters = 0).

  default   on the device: CALLS calls, synchronised once at the end, REPS times; the median is the figure.  Back-to-back
            launches run at the device's pace once its queue is full, so this shows what a caller sees, not the host's share.
  --stub    the host's share alone, no device needed: the library is replaced by ctypes callbacks of the real signatures that
            return at once, torch.cuda.device by a null context, the stream by NULL, and the tensors live on the CPU; the
            lowest of REPS x CALLS calls is the figure (pin the process to one core).

--tree names the checkout whose houv_amd is measured (default: this one), so that one copy of the script serves both sides of an
A/B; HOUV_HIP_LIB lets both load one library build.  Prints one JSON line.  -> profiles/r17_ops_call_path.txt"""
import argparse, contextlib, ctypes, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--stub", action="store_true")
ap.add_argument("--calls", type=int, default=None)
ap.add_argument("--reps", type=int, default=None)
args = ap.parse_args()
calls = args.calls or (300 if args.stub else 4000)
reps = args.reps or (400 if args.stub else 5)
sys.path.insert(0, os.path.abspath(args.tree))
import torch
from houv_amd import _lib, ops


class _Stub:
    """Every entry of _SIGNATURES as a ctypes callback that returns 1: ctypes converts the arguments as it does for the library."""

    def __getattr__(self, name):
        res, argtypes = _lib._SIGNATURES[name]
        fn = ctypes.CFUNCTYPE(res, *argtypes)(lambda *a: 1)
        setattr(self, name, fn)
        return fn


if args.stub:
    _lib._lib = _Stub()
    _lib.require_gpu = lambda *a, **k: None
    _lib.stream_of = lambda t: ctypes.c_void_p(0)
    torch.cuda.device = lambda d: contextlib.nullcontext()
    sync = lambda: None
    dev = torch.device("cpu")
else:
    sync = torch.cuda.synchronize
    dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(64)
cloud = torch.rand(1, 64, 3, generator=g).to(dev)
tgt = torch.rand(1, 64, 3, generator=g).to(dev)
state = torch.zeros(1, 24, dtype=torch.float64, device=dev)
outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((1,), (1,), (1, 3, 3), (1, 3))]


def knn():
    ops.knn(cloud, 8)


def solve():
    ops.solve_iterate_out(cloud, tgt, state, 1, 0, 1, 0, 0, True, False, 32, 64, 0.01, 0.9, 0.999, 1e-8, 1.0, *outs)


def per_call_us(fn):
    for _ in range(200):
        fn()
    sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        times.append((time.perf_counter() - t0) / calls * 1e6)
    return times


res = {"tree": os.path.abspath(args.tree), "mode": "stub" if args.stub else "device", "calls": calls, "reps": reps}
if not args.stub:
    res["build"] = _lib.build_id()
for name, fn in (("knn", knn), ("solve_iterate_out", solve)):
    t = per_call_us(fn)
    res[name] = {"lowest_us": round(min(t), 3)} if args.stub else \
        {"median_us": round(statistics.median(t), 3), "runs_us": [round(x, 3) for x in t]}
print(json.dumps(res))
