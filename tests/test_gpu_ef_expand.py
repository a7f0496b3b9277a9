"""GPU: houv_ef_expand / houv_ef_expand_backward against the NumPy restatement of tests/ef_expand_host.py.
The tolerance is the project's own for this block (tests/test_gpu_ecg.py): the largest error against the float64 restatement is
at most 4x the float32 restatement's error against float64 on the same case -- for `out` and, under the device's own arg, for
gproj, gW2a, gW3 and gb3.  Every arg is a maximum of its column in float64 to within 2x that spread.  Then the exact cases (ties,
NaN, out-of-range lists), leading dimensions and offset bases, run-to-run bits, B = 0, the refusals, and the memory condition:
the node's forward + backward raises the allocator's peak by less than the torch composition's."""
import ctypes

import numpy as np
import pytest
import torch

import ef_expand_host as host
from ef_expand_cases import SWEEP, composed_rows, make_case

pytestmark = pytest.mark.gpu
T = torch.tensor
GRADS = ("gproj", "gW2a", "gW3", "gb3")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(dev, c, idx=None):
    """-> (out, arg, {gradients}) from the device as NumPy."""
    from houv_amd import ops
    d = {n: T(c[n]).to(dev) for n in ("proj", "W2a", "W3", "b3", "g")}
    ix = T(c["idx"] if idx is None else idx).to(dev)
    out, arg = ops.ef_expand(d["proj"], ix, d["W2a"], d["W3"], d["b3"], c["r"], want_arg=True)
    g = ops.ef_expand_backward(d["proj"], ix, arg, d["W2a"], d["W3"], d["g"], c["r"])
    return out.cpu().numpy(), arg.cpu().numpy(), {n: v.cpu().numpy() for n, v in g.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check(c, out, arg, grads, label):
    """The 4x rule on out and on every gradient, and the 2x rule on arg."""
    a = (c["proj"], c["idx"], c["W2a"], c["W3"], c["b3"], c["r"])
    e64 = host.slots(*a, np.float64)
    o64, _ = host.forward(*a, np.float64)
    o32, _ = host.forward(*a, np.float32)
    err, spread = float(np.abs(out - o64).max()), float(np.abs(o32 - o64).max())
    print(f"{label} out: device vs float64 {err:.3e}, float32 restatement vs float64 {spread:.3e}")
    assert out.shape == o64.shape and arg.shape == o64.shape and arg.dtype == np.int8
    assert err <= 4 * spread
    B, N, k, r, O = e64.shape
    assert arg.min() >= 0 and arg.max() < k
    picked = np.take_along_axis(e64, arg.reshape(B, N, 1, r, O).astype(np.int64), axis=2)[:, :, 0]
    assert (picked >= e64.max(axis=2) - 2 * spread).all()
    b = (c["proj"], c["idx"], arg, c["W2a"], c["W3"], c["g"], c["r"])
    g64, g32 = host.backward(*b, np.float64), host.backward(*b, np.float32)
    for n in GRADS:
        err, spread = float(np.abs(grads[n] - g64[n]).max()), float(np.abs(g32[n] - g64[n]).max())
        print(f"{label} {n}: device vs float64 {err:.3e}, float32 restatement vs float64 {spread:.3e}")
        assert grads[n].shape == g64[n].shape
        assert err <= 4 * spread, n


@pytest.mark.parametrize("C,O,r,k,N,B", SWEEP)
def test_sweep(dev, C, O, r, k, N, B):
    c = make_case(C, O, r, k, N, B)
    out, arg, grads = _run(dev, c)
    _check(c, out, arg, grads, f"C={C} O={O} r={r} k={k} N={N} B={B}")


def test_more_than_one_group_of_clouds(dev):
    """The backward takes the clouds in groups of about 32768 edges: 5 clouds of 1100 x 8 edges are a group of 3 and one of 2
    (the second leaves rows of the first behind in the workspace, past its own)."""
    c = make_case(64, 64, 2, 8, 1100, 5, seed=6)
    out, arg, grads = _run(dev, c)
    _check(c, out, arg, grads, "groups of 3 + 2 clouds")
    again = _run(dev, c)
    assert _same(out, again[0]) and all(_same(grads[n], again[2][n]) for n in GRADS)


def test_one_point_k_times_gives_slot_zero(dev):
    c = make_case(64, 64, 2, 4, 37, 2, seed=1)
    c["idx"][:] = c["idx"][:, :, 1:2]                                             # every list is one point four times
    out, arg, _ = _run(dev, c)
    assert (arg == 0).all()


def test_nan_row(dev):
    c = make_case(64, 64, 2, 4, 37, 2, seed=2)
    c["proj"][1, 5, :] = np.nan
    c["idx"][1, 7, :] = 5                                                         # point 7 lists only the NaN row
    out, arg, grads = _run(dev, c)
    r = c["r"]
    dead = np.zeros(arg.shape[:2], dtype=bool)
    dead[1, 5 * r:6 * r] = dead[1, 7 * r:8 * r] = True
    assert (arg[dead] == -1).all() and np.isnan(out[dead]).all()
    assert (arg[~dead] >= 0).all() and not np.isnan(out[~dead]).any()
    lists = c["idx"][1] == 5
    for n in range(37):
        for j in np.nonzero(lists[n])[0]:
            assert (arg[1, n * r:(n + 1) * r] != j).all()
    want_o, want_a = host.forward(c["proj"], c["idx"], c["W2a"], c["W3"], c["b3"], r, np.float32)
    assert np.array_equal(want_a == -1, arg == -1)
    assert all(np.isfinite(v).all() for v in grads.values())
    O = c["W3"].shape[0]
    assert (grads["gproj"][1, 5, :O] == 0).all() and (grads["gproj"][1, 7, :O] == 0).all()       # no gradient from all-NaN columns
    g64 = host.backward(c["proj"], c["idx"], arg, c["W2a"], c["W3"], c["g"], r, np.float64)
    g32 = host.backward(c["proj"], c["idx"], arg, c["W2a"], c["W3"], c["g"], r, np.float32)
    for n in GRADS:
        assert np.abs(grads[n] - g64[n]).max() <= 4 * np.abs(g32[n] - g64[n]).max(), n


def test_out_of_range_lists_are_clamped(dev):
    c = make_case(64, 64, 3, 4, 21, 2, seed=3)
    wild = c["idx"].copy()
    wild[0, 1, 3], wild[1, 2, 0], wild[0, 20, 2], wild[1, 0, 1] = 21, -1, 2 ** 31 - 1, -2 ** 31
    a = _run(dev, c, idx=wild)
    b = _run(dev, c, idx=np.clip(wild, 0, 20))
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and all(_same(a[2][n], b[2][n]) for n in GRADS)


@pytest.mark.parametrize("O,r,pad,off", [(64, 2, 0, 0), (64, 3, 7, 1), (128, 1, 4, 1), (256, 2, 13, 3)])
def test_leading_dimensions_and_offset_bases(dev, O, r, pad, off):
    """proj, out, g and gproj as column slices of wider buffers (odd widths) at bases 4 * off bytes past a 16-byte boundary: the
    same bits as the dense call, and the sentinels around them untouched."""
    from houv_amd import ops
    c = make_case(64, O, r, 4, 21, 2, seed=4)
    B, N, W = c["proj"].shape
    dense = _run(dev, c)

    def wide(a):
        buf = torch.full((a.shape[0], a.shape[1], a.shape[2] + pad + off), -7.5, device=dev)
        view = buf[:, :, off:off + a.shape[2]]
        view.copy_(T(a).to(dev))
        return buf, view

    pbuf, proj = wide(c["proj"])
    gbuf, g = wide(c["g"])
    obuf, out = wide(np.zeros_like(c["g"]))
    qbuf, gproj = wide(np.zeros_like(c["proj"]))
    obuf.fill_(-7.5), qbuf.fill_(-7.5)
    w2buf = torch.full((O * r, O + 2 * 64 + pad), -7.5, device=dev)             # W2a as the first columns of a wider weight
    w2buf[:, :O] = T(c["W2a"]).to(dev)
    ix, W3, b3 = T(c["idx"]).to(dev), T(c["W3"]).to(dev), T(c["b3"]).to(dev)
    o, arg = ops.ef_expand(proj, ix, w2buf[:, :O], W3, b3, r, out=out, want_arg=True)
    res = ops.ef_expand_backward(proj, ix, arg, w2buf[:, :O], W3, g, r, gproj=gproj)
    assert o.data_ptr() == out.data_ptr() and (out.data_ptr() - obuf.data_ptr()) == 4 * off
    assert _same(out.cpu().numpy(), dense[0]) and _same(arg.cpu().numpy(), dense[1])
    assert _same(gproj.cpu().numpy(), dense[2]["gproj"])
    for n in GRADS[1:]:
        assert _same(res[n].cpu().numpy(), dense[2][n]), n
    for buf, width in ((obuf, O), (qbuf, W)):
        assert (buf[:, :, :off] == -7.5).all() and (buf[:, :, off + width:] == -7.5).all()
    assert _same(pbuf[:, :, off:off + W].cpu().numpy(), c["proj"]) and _same(gbuf[:, :, off:off + O].cpu().numpy(), c["g"])


def test_run_to_run_zero_gradient_and_empty_batch(dev):
    from houv_amd import ops
    c = make_case(256, 64, 2, 4, 130, 3, seed=5)
    a, b = _run(dev, c), _run(dev, c)
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and all(_same(a[2][n], b[2][n]) for n in GRADS)
    z = dict(c, g=np.zeros_like(c["g"]))
    grads = _run(dev, z)[2]
    assert all((grads[n] == 0).all() and not np.signbit(grads[n]).any() for n in GRADS)
    O, r = 64, 2
    e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)
    out, arg = ops.ef_expand(e(0, 9, 2 * O + 2 * O * r), e(0, 9, 4, dt=torch.int32), T(c["W2a"]).to(dev), T(c["W3"]).to(dev),
                             T(c["b3"]).to(dev), r, want_arg=True)
    assert tuple(out.shape) == (0, 9 * r, O) and tuple(arg.shape) == (0, 9 * r, O)
    res = ops.ef_expand_backward(e(0, 9, 2 * O + 2 * O * r), e(0, 9, 4, dt=torch.int32), arg, T(c["W2a"]).to(dev), T(c["W3"]).to(dev),
                                 e(0, 9 * r, O), r)
    assert tuple(res["gproj"].shape) == (0, 9, 2 * O + 2 * O * r)
    assert all((res[n] == 0).all() for n in GRADS[1:])


def test_refusals(dev):
    from houv_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=dev)
    ibuf = torch.zeros(1 << 12, dtype=torch.int32, device=dev)
    abuf = torch.zeros(1 << 14, dtype=torch.int8, device=dev)
    wbuf = torch.zeros(1 << 16, device=dev)
    p, ip, ap, wp, null = _lib.ptr(buf), _lib.ptr(ibuf), _lib.ptr(abuf), _lib.ptr(wbuf), None
    st = _lib.stream_of(buf)

    def fw(B=1, N=4, O=64, k=4, r=1, ldp=None, ldw=None, ldo=None, proj=p, idx=ip, W2a=p, W3=p, b3=p, out=p):
        W = 2 * O + 2 * O * r
        return lib.houv_ef_expand(proj, W if ldp is None else ldp, idx, B, N, O, k, r, W2a, O if ldw is None else ldw, W3, b3, out,
                                  O if ldo is None else ldo, null, st)

    def bw(B=1, N=4, O=64, k=4, r=1, ldp=None, ldw=None, ldg=None, ldgp=None, ws=wp, nbytes=None, **ptrs):
        W = 2 * O + 2 * O * r
        a = dict(proj=p, idx=ip, arg=ap, W2a=p, W3=p, g=p, gproj=p, gW2a=p, gW3=p, gb3=p)
        a.update(ptrs)
        need = lib.houv_ef_expand_backward_workspace_bytes(B, N, O, k, r)
        return lib.houv_ef_expand_backward(a["proj"], W if ldp is None else ldp, a["idx"], a["arg"], B, N, O, k, r, a["W2a"],
                                           O if ldw is None else ldw, a["W3"], a["g"], O if ldg is None else ldg, a["gproj"],
                                           W if ldgp is None else ldgp, a["gW2a"], a["gW3"], a["gb3"], ws,
                                           need if nbytes is None else nbytes, st)

    def refused(ok, *words):
        err = _lib.last_error()
        assert ok == 0 and all(w in err for w in words), err

    assert fw() == 1 and bw() == 1
    shapes = (dict(O=32), dict(O=96), dict(O=512), dict(r=0), dict(r=9), dict(k=0), dict(k=9), dict(N=0), dict(N=16385), dict(B=-1))
    words = (("O=32",), ("O=96",), ("O=512",), ("r=0",), ("r=9",), ("k=0",), ("k=9",), ("N=0",), ("N=16385",), ("B=-1",))
    for kw, w in zip(shapes, words):
        refused(fw(**kw), "houv_ef_expand:", *w)
        refused(bw(**kw), "houv_ef_expand_backward:", *w)
        assert lib.houv_ef_expand_backward_workspace_bytes(kw.get("B", 1), kw.get("N", 4), kw.get("O", 64), kw.get("k", 4),
                                                           kw.get("r", 1)) == 0
    assert lib.houv_ef_expand_backward_workspace_bytes(0, 4, 64, 4, 1) == 0
    refused(fw(ldp=255), "ldp=255"); refused(fw(ldw=63), "ldw=63"); refused(fw(ldo=63), "ldo=63")
    refused(bw(ldp=255), "ldp=255"); refused(bw(ldw=63), "ldw=63"); refused(bw(ldg=63), "ldg=63"); refused(bw(ldgp=255), "ldgp=255")
    for name in ("proj", "idx", "W2a", "W3", "b3", "out"):
        refused(fw(**{name: null}), f"{name} is a null pointer")
    for name in ("proj", "idx", "arg", "W2a", "W3", "g", "gproj", "gW2a", "gW3", "gb3"):
        refused(bw(**{name: null}), f"{name} is a null pointer")
    need = lib.houv_ef_expand_backward_workspace_bytes(1, 4, 64, 4, 1)
    assert need > 0
    refused(bw(ws=null), "workspace"); refused(bw(nbytes=need - 1), "workspace", str(need))
    refused(bw(ws=ctypes.c_void_p(wbuf.data_ptr() + 4)), "workspace", "aligned")
    assert fw(B=0, proj=null, idx=null, out=null) == 1                           # B = 0 launches nothing and reads nothing


def test_node_uses_less_memory_than_the_composition(dev):
    """B = 2, N = 512, k = 4, 256 -> 64, r = 2: one forward + backward of each, the allocator's peak above what was allocated."""
    from houv_amd import model_utils_completion as muc, ops
    torch.manual_seed(0)
    B, N, C = 2, 512, 256
    net = muc.EF_expansion(C, 64, step_ratio=2, k=4, trainable=True).to(dev)
    rows = torch.randn(B, N, C, device=dev).requires_grad_(True)
    idx = ops.knn_feat(rows.detach(), 4)
    G = torch.randn(B, N * 2, 64, device=dev)

    def peak(forward):
        for p in list(net.parameters()) + [rows]:
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = forward()
        (out * G).sum().backward()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out.detach(), rows.grad.clone()

    for f in (lambda: net.forward_rows(rows, idx=idx), lambda: composed_rows(net, rows, idx)):      # warm the allocator and the library
        peak(f)
    node, out_a, gx_a = peak(lambda: net.forward_rows(rows, idx=idx))
    comp, out_b, gx_b = peak(lambda: composed_rows(net, rows, idx))
    print(f"peak of forward + backward: node {node:.1f} MiB, composition {comp:.1f} MiB")
    assert node < comp
    assert float((out_a - out_b).abs().max()) <= 1e-4 * float(out_b.abs().max())
    assert float((gx_a - gx_b).norm()) <= 1e-4 * float(gx_b.norm())
