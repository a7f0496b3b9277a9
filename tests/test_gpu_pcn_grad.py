"""GPU: the encoder half of PCN's backward pass.

houv_mlp2_max_arg, the PointNet block that also reports where each maximum was found, has no tolerance: pooled and y are compared
with houv_mlp2_max's bits, and arg with the lowest n at which the STORED y equals the stored pooled (torch.max's rule on the CPU),
computed on the host.

houv_mlp2_max_backward is compared with the float64 NumPy restatement in the reference's materialising form (tests/pcn_grad_host.py)
under the same injected arg; the bound of each output is 4x the float32 restatement's own largest error on the same inputs (the
kernel-level factor of test_gpu_pcn.py), computed and printed per case."""
import numpy as np
import pytest
import torch

import pcn_cases as cases

pytestmark = pytest.mark.gpu

T = torch.tensor
ARG_N = [1, cases.T - 1, cases.T, cases.T + 1, 2 * cases.T + 5]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _lowest_match(y, pooled):
    """arg by its definition, from what the kernel stored: the lowest n with y[b,n,c] == pooled[b,c], -1 when there is none."""
    hit = y.cpu().numpy() == pooled.cpu().numpy()[:, None, :]
    return np.where(hit.any(1), hit.argmax(1), -1).astype(np.int32)


def _run(dev, case, want_y=True):
    from houv_amd import ops
    return ops.mlp2_max_arg(*(T(a).to(dev) for a in case), want_y=want_y)


def _plain(dev, case):
    from houv_amd import ops
    return ops.mlp2_max(*(T(a).to(dev) for a in case), want_y=True)


def _check(dev, case):
    """The whole contract on one case; returns (pooled, arg, y) for what a test wants to say on top."""
    pooled, arg, y = _run(dev, case)
    torch.cuda.synchronize()
    B, N = case[0].shape[:2]
    Cout = case[3].shape[0]
    assert pooled.shape == (B, Cout) and arg.shape == (B, Cout) and arg.dtype == torch.int32 and y.shape == (B, N, Cout)
    p0, y0 = _plain(dev, case)
    assert np.array_equal(_bits(pooled), _bits(p0)) and np.array_equal(_bits(y), _bits(y0))       # mlp2_max's bits
    want = _lowest_match(y, pooled)
    got = arg.cpu().numpy()
    assert np.array_equal(got, want), ("columns that differ", np.argwhere(got != want)[:8].tolist())
    p1, a1, none = _run(dev, case, want_y=False)
    assert none is None and np.array_equal(_bits(p1), _bits(pooled)) and torch.equal(a1, arg)     # y stored or not
    p2, a2, y2 = _run(dev, case)
    assert np.array_equal(_bits(p2), _bits(pooled)) and torch.equal(a2, arg) and np.array_equal(_bits(y2), _bits(y))
    return pooled, arg, y


@pytest.mark.parametrize("N", ARG_N)
@pytest.mark.parametrize("B", cases.MLP_B)
@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_arg_is_the_lowest_row_of_the_stored_maximum(dev, Cin, H, Cout, B, N):
    _, arg, _ = _check(dev, cases.mlp_case(B, N, Cin, H, Cout))
    assert int(arg.min()) >= 0 and int(arg.max()) < N
    if N > 2 * cases.T:
        assert len(torch.unique(arg // cases.T)) == 3                                 # every row tile owns some column


@pytest.mark.parametrize("N", [cases.T, 2 * (cases.T + 3)])
@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_arg_of_a_tie_is_the_first_index(dev, Cin, H, Cout, N):
    """Every point twice, x[n + N/2] = x[n]: each maximum is attained at two rows with identical bits, N/2 apart -- in the
    other 32-row half of the tile at N = 64, in another tile (and at another row of it) at N = 134.  The first one wins."""
    x, W1, s1, W2, b2 = cases.mlp_case(2, N, Cin, H, Cout, seed=4)
    x[:, N // 2:] = x[:, :N // 2]
    _, arg, y = _check(dev, (x, W1, s1, W2, b2))
    assert np.array_equal(_bits(y[:, N // 2:]), _bits(y[:, :N // 2]))                 # the ties are exact
    assert int(arg.max()) < N // 2 and int(arg.min()) >= 0


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_arg_in_the_last_row_of_a_partial_tile(dev, Cin, H, Cout):
    """N = T + 3 with the last valid row 8x larger than any other (test_gpu_pcn.py's case): it owns about 0.38 of the columns,
    and the rows past it, which repeat it inside the kernel, must never be reported."""
    N = cases.T + 3
    x, W1, s1, W2, b2 = cases.mlp_case(2, N, Cin, H, Cout, seed=2)
    x[:, N - 1] *= np.float32(8)
    _, arg, _ = _check(dev, (x, W1, s1, W2, b2))
    share = float((arg == N - 1).float().mean())
    print((Cin, H, Cout), "columns owned by the last row", share)
    assert share > 0.3 and int(arg.max()) == N - 1


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_arg_all_negative_columns(dev, Cin, H, Cout):
    x, W1, s1, W2, b2 = cases.mlp_case(3, cases.T + 1, Cin, H, Cout, seed=1)
    case = (x, W1, s1, (W2 * np.float32(0.25)).astype(np.float32), (b2 - np.float32(50)).astype(np.float32))
    pooled, arg, _ = _check(dev, case)
    assert bool((pooled < -10).all()) and int(arg.min()) >= 0


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_arg_nan_and_infinite_columns(dev, Cin, H, Cout):
    """Column 0 is NaN in every row (b2 = NaN): pooled -inf, arg -1.  Column 1 is -inf in every row: its first row.  Hidden
    unit 0 is relu(x[n,0]) and columns 2 and 3 weigh it with +inf and -inf: a row with x[n,0] > 0 holds +inf / -inf there and
    every other row NaN (inf * 0), which the maximum skips.  Cloud 1 has x[n,0] > 0 in row T + 4 alone, so its first tile
    reports no row for these columns and the fold has to take the second tile's -- for column 3 on an equal value, -inf."""
    N = cases.T + 9
    x, W1, s1, W2, b2 = cases.mlp_case(2, N, Cin, H, Cout, seed=5)
    b2[0], b2[1] = np.nan, -np.inf
    W1[0], s1[:, 0] = 0, 0
    W1[0, 0] = 1
    W2[2, 0], W2[3, 0] = np.inf, -np.inf
    x[1, :, 0] = -0.5
    x[1, cases.T + 4, 0] = 0.5
    first = int(np.argmax(x[0, :, 0] > 0))
    pooled, arg, y = _check(dev, (x, W1, s1, W2, b2))
    arg, pooled = arg.cpu().numpy(), pooled.cpu().numpy()
    assert (arg[:, 0] == -1).all() and (pooled[:, 0] == -np.inf).all() and bool(torch.isnan(y[:, :, 0]).all())
    assert (arg[:, 1] == 0).all() and (pooled[:, 1] == -np.inf).all()
    assert bool(torch.isnan(y[1, :cases.T, 2:4]).all())
    assert (pooled[:, 2] == np.inf).all() and (pooled[:, 3] == -np.inf).all()
    assert (arg[0, 2:4] == first).all() and (arg[1, 2:4] == cases.T + 4).all()
    assert (arg[:, 4:] >= 0).all()


def test_mlp2_max_arg_error_paths(dev):
    from houv_amd import _lib, ops
    lib = _lib.load()
    d = [T(a).to(dev) for a in cases.mlp_case(2, 5, 3, 128, 256)]
    x, W1, s1, W2, b2 = (_lib.ptr(t) for t in d)
    pooled, arg = torch.empty(2, 256, device=dev), torch.empty(2, 256, dtype=torch.int32, device=dev)

    def call(N=5, Cin=3, H=128, Cout=256, stride=128, x=x, pooled=_lib.ptr(pooled), arg=_lib.ptr(arg), ws=None):
        return lib.houv_mlp2_max_arg(x, 2, N, Cin, W1, H, s1, stride, W2, b2, Cout, pooled, arg, None, ws, None)
    assert call() == 1
    for kw, msg in ((dict(N=0), "N=0"), (dict(Cin=4), "(4, 128, 256)"), (dict(H=256), "(3, 256, 256)"), (dict(Cout=512), "(3, 128, 512)"),
                    (dict(stride=64), "shift1_stride=64"), (dict(x=None), "x is a null pointer"),
                    (dict(pooled=None), "pooled is a null pointer"), (dict(arg=None), "arg is a null pointer"),
                    (dict(N=cases.T + 1), "workspace is a null pointer: N=65 spans 2 row tiles (houv_mlp2_max_arg_workspace_bytes)")):
        assert call(**kw) == 0, kw
        assert _lib.last_error().startswith("houv_mlp2_max_arg: ") and msg in _lib.last_error(), (kw, _lib.last_error())
    assert lib.houv_mlp2_max_arg_workspace_bytes(2, cases.T, 256) == 0
    assert lib.houv_mlp2_max_arg_workspace_bytes(2, cases.T + 1, 256) == 2 * lib.houv_mlp2_max_workspace_bytes(2, cases.T + 1, 256) \
        == 2 * 2 * 2 * 256 * 4
    torch.cuda.synchronize()
    with pytest.raises(_lib.HouvHipError, match="CPU tensor"):
        ops.mlp2_max_arg(*(T(a) for a in cases.mlp_case(2, 5, 3, 128, 256)))
    with pytest.raises(_lib.HouvHipError, match=r"houv_mlp2_max_arg: \(Cin, H, Cout\) = \(4, 128, 256\)"):
        ops.mlp2_max_arg(torch.zeros(1, 5, 4, device=dev), torch.zeros(128, 4, device=dev), d[2][0].contiguous(), d[3], d[4])
    with pytest.raises(_lib.HouvHipError, match="mlp2_max_arg: shift1 must be"):
        ops.mlp2_max_arg(d[0], d[1], torch.zeros(3, 128, device=dev), d[3], d[4])
    with pytest.raises(_lib.HouvHipError, match="expected torch.float32"):
        ops.mlp2_max_arg(d[0].double(), *d[1:])


def test_mlp2_max_arg_torch_op(dev):
    from houv_amd import ops
    ops.register_torch_ops()
    d = [T(a).to(dev) for a in cases.mlp_case(3, cases.T + 1, 256, 512, 1024)]
    a, b = torch.ops.houv.mlp2_max_arg(*d), ops.mlp2_max_arg(*d, want_y=True)
    assert len(a) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------- mlp2_max_backward
import pcn_grad_host as ghost  # noqa: E402
import pcn_host as host  # noqa: E402

_BW = {}
KEYS = ("gW1", "gshift1", "gW2", "gb2", "gx")


def _bw_case(Cin, H, Cout, B, N, rows_kind="none", per_cloud=True, same_arg=False):
    """Inputs, the float64 restatement's gradients under the injected arg, and per output 4x the float32 restatement's own
    largest error: computed once per case and shared.  The inputs are the first of the seeds 0, 1, ... (cap 64) whose ReLU
    inputs all clear zero by pcn_grad_host.clear_of_kinks' margin; arg is the float64 forward's (or one row for every column)."""
    key = (Cin, B, N, rows_kind, per_cloud, same_arg)
    if key in _BW:
        return _BW[key]
    for seed in range(64):
        x, W1, s1, W2, b2 = cases.mlp_case(B, N, Cin, H, Cout, per_cloud=per_cloud, seed=10 + seed)
        if ghost.clear_of_kinks(x, W1, s1):
            break
    else:
        raise AssertionError(f"no seed below 64 keeps every ReLU input of {key} clear of zero")
    rng = np.random.default_rng(977 * N + 13 * B + Cin)
    arg = host.mlp2_max(x, W1, s1, W2, b2)[1].argmax(1).astype(np.int32)
    if same_arg:
        arg[:] = min(5, N - 1)
    gpooled = rng.uniform(-1, 1, (B, Cout)).astype(np.float32)
    rows = nrows = gy_rows = gy = None
    if rows_kind != "none":
        picked = np.arange(N) if rows_kind == "all" else np.unique(np.clip([0, cases.T - 1, cases.T, N - 1], 0, N - 1))
        R = len(picked) + (rows_kind == "few")                                        # "few": one unused entry at the end
        rows = np.full((B, R), -7, dtype=np.int32)
        rows[:, :len(picked)] = picked
        nrows = np.full(B, len(picked), dtype=np.int32)
        if rows_kind == "few" and len(picked) > 1:
            nrows[1::2] -= 1                                                          # odd clouds list one row fewer
        gy_rows = rng.uniform(-0.1, 0.1, (B, R, Cout)).astype(np.float32)
        gy = np.zeros((B, N, Cout), dtype=np.float32)
        for b in range(B):
            gy[b, rows[b, :nrows[b]]] = gy_rows[b, :nrows[b]]
    r64 = ghost.mlp2_max_backward(x, W1, s1, W2, arg, gpooled, gy, np.float64)
    r32 = ghost.mlp2_max_backward(x, W1, s1, W2, arg, gpooled, gy, np.float32)
    bounds = {k: 4 * float(np.abs(r32[k] - r64[k]).max()) for k in KEYS}
    active = [np.unique(np.concatenate([arg[b], rows[b, :nrows[b]] if rows is not None else arg[b]])) for b in range(B)]
    _BW[key] = dict(inputs=(x, W1, s1, W2), arg=arg, gpooled=gpooled, rows=rows, nrows=nrows, gy_rows=gy_rows, r64=r64, bounds=bounds,
                    active=active)
    return _BW[key]


def _run_bw(dev, c, want_gx=True, **over):
    from houv_amd import ops
    d = lambda a: None if a is None else T(a).to(dev)
    a = dict(arg=c["arg"], gpooled=c["gpooled"], rows=c["rows"], nrows=c["nrows"], gy_rows=c["gy_rows"])
    a.update(over)
    return ops.mlp2_max_backward(*(d(v) for v in c["inputs"]), d(a["arg"]), d(a["gpooled"]), d(a["rows"]), d(a["nrows"]),
                                 d(a["gy_rows"]), want_gx=want_gx)


def _check_bw(dev, c, label):
    out = _run_bw(dev, c)
    torch.cuda.synchronize()
    x = c["inputs"][0]
    B, N, Cin = x.shape
    Cout = c["arg"].shape[1]
    rcap = min(N, Cout + (0 if c["rows"] is None else c["rows"].shape[1]))
    act, nact, gxr = out["act_rows"].cpu().numpy(), out["nact"].cpu().numpy(), out["gx_rows"].cpu().numpy()
    assert act.shape == (B, rcap) and gxr.shape == (B, rcap, Cin)
    gx = np.zeros((B, N, Cin), dtype=np.float32)
    for b in range(B):
        want = c["active"][b]
        assert nact[b] == len(want) and np.array_equal(act[b, :nact[b]], want) and (act[b, nact[b]:] == -1).all()
        assert not gxr[b, nact[b]:].any()                                             # padding slots: exact zeros
        gx[b, want] = gxr[b, :nact[b]]
    got = dict(gW1=out["gW1"], gshift1=out["gshift1"], gW2=out["gW2"], gb2=out["gb2"])
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got["gx"] = gx
    for k in KEYS:
        err = float(np.abs(got[k] - c["r64"][k]).max())
        print(label, k, "error", err, "bound", c["bounds"][k], "largest", float(np.abs(c["r64"][k]).max()))
        assert got[k].shape == c["r64"][k].shape and err <= c["bounds"][k], (label, k)
    again = _run_bw(dev, c)
    for k in ("gW1", "gshift1", "gW2", "gb2", "gx_rows", "act_rows", "nact"):
        assert np.array_equal(_bits(again[k]), _bits(out[k])), k                      # two calls: identical bits
    return out


@pytest.mark.parametrize("N", ARG_N)
@pytest.mark.parametrize("B", cases.MLP_B)
@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_backward_vs_float64(dev, Cin, H, Cout, B, N):
    """The first block as the model uses it (a few rows carry a gradient on y, in different tiles), the second with the
    pooled gradient alone."""
    kind = "few" if Cin == 3 else "none"
    _check_bw(dev, _bw_case(Cin, H, Cout, B, N, kind), f"{(Cin, H, Cout)} B {B} N {N} rows {kind}")


@pytest.mark.parametrize("Cin,H,Cout,kind", [(3, 128, 256, "none"), (3, 128, 256, "all"), (256, 512, 1024, "few"), (256, 512, 1024, "all")])
def test_mlp2_max_backward_row_lists(dev, Cin, H, Cout, kind):
    """No list, a few rows, and every row (the dense case: A_b is the whole cloud), on two tiles and a bit."""
    _check_bw(dev, _bw_case(Cin, H, Cout, 2, cases.T + 1, kind), f"{(Cin, H, Cout)} rows {kind}")


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_backward_one_active_row_and_shared_shift(dev, Cin, H, Cout):
    """Every column's maximum in the same row: |A_b| = 1.  With one shift1 for all clouds, gshift1 still has a row per cloud."""
    out = _check_bw(dev, _bw_case(Cin, H, Cout, 3, cases.T + 1, "none", same_arg=True), f"{(Cin, H, Cout)} one row")
    assert out["nact"].tolist() == [1, 1, 1]
    c = _bw_case(Cin, H, Cout, 3, cases.T + 1, "none", per_cloud=False)
    assert c["inputs"][2].shape == (H,)
    out = _check_bw(dev, c, f"{(Cin, H, Cout)} shared shift")
    assert out["gshift1"].shape == (3, H)


@pytest.mark.parametrize("Cin,H,Cout", cases.MLP_SHAPES)
def test_mlp2_max_backward_of_a_zero_gradient_is_zero(dev, Cin, H, Cout):
    c = _bw_case(Cin, H, Cout, 2, cases.T + 1, "none")
    out = _run_bw(dev, c, gpooled=np.zeros_like(c["gpooled"]))
    for k in ("gW1", "gshift1", "gW2", "gb2", "gx_rows"):
        assert not out[k].cpu().numpy().any(), k
    none = _run_bw(dev, c, want_gx=False)
    assert none["gx_rows"] is None and np.array_equal(_bits(none["gW1"]), _bits(_run_bw(dev, c)["gW1"]))
    dead = c["arg"].copy()
    dead[:, ::2] = -1                                                                 # all-NaN columns pass nothing
    half = _run_bw(dev, c, arg=dead)
    kept = _run_bw(dev, c, gpooled=np.where(dead < 0, 0, c["gpooled"]).astype(np.float32))
    assert np.array_equal(_bits(half["gW2"])[1::2], _bits(kept["gW2"])[1::2]) and not half["gW2"][::2].cpu().numpy().any()
    assert np.array_equal(_bits(half["gb2"]), _bits(kept["gb2"]))


@pytest.mark.parametrize("Cin,H,Cout,kind,same_arg", [(3, 128, 256, "few", True), (256, 512, 1024, "none", True),
                                                      (3, 128, 256, "few", False)])
def test_mlp2_max_backward_writes_every_output_over_sentinels(dev, Cin, H, Cout, kind, same_arg):
    """The C entry on buffers that were filled beforehand (floats with NaN, integers with 0x7f7f7f7f, the workspace with NaN
    too): every output element is written, the slots past nact[b] hold -1 and exact zeros, and the values are those of a call
    on fresh buffers, bit for bit.  B = 3, N = T + 1, so Rcap = N; with one row owning every maximum (same_arg) all but 1 .. 4 slots of a cloud are
    padding."""
    from houv_amd import _lib
    lib = _lib.load()
    c = _bw_case(Cin, H, Cout, 3, cases.T + 1, kind, same_arg=same_arg)
    want = _run_bw(dev, c)
    d = lambda a: None if a is None else T(a).to(dev)
    x, W1, s1, W2 = (d(a) for a in c["inputs"])
    arg, gp, rows, nrows, gy = d(c["arg"]), d(c["gpooled"]), d(c["rows"]), d(c["nrows"]), d(c["gy_rows"])
    B, N = 3, cases.T + 1
    R = 0 if rows is None else rows.shape[1]
    rcap = lib.houv_mlp2_max_backward_rows(N, Cout, R)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    junk = lambda *shape: torch.full(shape, 0x7f7f7f7f, dtype=torch.int32, device=dev)
    out = dict(gW1=nan(H, Cin), gshift1=nan(B, H), gW2=nan(Cout, H), gb2=nan(Cout), act_rows=junk(B, rcap), nact=junk(B),
               gx_rows=nan(B, rcap, Cin))
    ws = nan(lib.houv_mlp2_max_backward_workspace_bytes(B, N, Cin, H, Cout, R) // 4)
    p = _lib.ptr
    with torch.cuda.device(dev):
        ok = lib.houv_mlp2_max_backward(p(x), B, N, Cin, p(W1), H, p(s1), H, p(W2), Cout, p(arg), p(gp), p(rows), p(nrows), p(gy), R,
                                        p(out["gW1"]), p(out["gshift1"]), p(out["gW2"]), p(out["gb2"]), p(out["act_rows"]),
                                        p(out["nact"]), p(out["gx_rows"]), p(ws), _lib.stream_of(x))
    assert ok == 1, _lib.last_error()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert np.array_equal(_bits(v), _bits(want[k])), k
    act, nact, gxr = out["act_rows"].cpu().numpy(), out["nact"].cpu().numpy(), out["gx_rows"].cpu().numpy()
    for b in range(B):
        assert nact[b] == len(c["active"][b]) and (nact[b] < rcap or not same_arg)    # same_arg: there is padding to look at
        assert (act[b, nact[b]:] == -1).all() and (gxr[b, nact[b]:].view(np.int32) == 0).all()
    assert not any(bool(torch.isnan(out[k]).any()) for k in ("gW1", "gshift1", "gW2", "gb2", "gx_rows"))


def test_mlp2_max_backward_refusals_and_torch_op(dev):
    from houv_amd import _lib, ops
    lib = _lib.load()
    c = _bw_case(3, 128, 256, 2, cases.T + 1, "few")
    d = lambda a: T(a).to(dev)
    x, W1, s1, W2 = (d(a) for a in c["inputs"])
    arg, gp, rows, nrows, gy = d(c["arg"]), d(c["gpooled"]), d(c["rows"]), d(c["nrows"]), d(c["gy_rows"])
    N, R = cases.T + 1, c["rows"].shape[1]
    assert lib.houv_mlp2_max_backward_rows(N, 256, R) == N and lib.houv_mlp2_max_backward_rows(2048, 256, 100) == 356
    nbytes = lib.houv_mlp2_max_backward_workspace_bytes(2, N, 3, 128, 256, R)
    assert nbytes > 0 and nbytes % 16 == 0 and lib.houv_mlp2_max_backward_workspace_bytes(2, N, 3, 128, 512, R) == 0
    ws = torch.empty(nbytes // 4, device=dev)
    o = [torch.empty(128, 3, device=dev), torch.empty(2, 128, device=dev), torch.empty(256, 128, device=dev), torch.empty(256, device=dev),
         torch.empty(2, N, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)]
    p = _lib.ptr

    def call(N=N, Cin=3, H=128, Cout=256, stride=128, R=R, x=p(x), arg=p(arg), rows=p(rows), gW1=p(o[0]), ws=p(ws)):
        return lib.houv_mlp2_max_backward(x, 2, N, Cin, p(W1), H, p(s1), stride, p(W2), Cout, arg, p(gp), rows, p(nrows), p(gy), R,
                                          gW1, p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(o[5]), None, ws, None)
    assert call() == 1
    for kw, msg in ((dict(N=0), "N=0"), (dict(Cin=4), "(4, 128, 256)"), (dict(Cout=512), "(3, 128, 512)"), (dict(stride=64), "shift1_stride=64"),
                    (dict(R=-1), "R=-1"), (dict(x=None), "x is a null pointer"),
                    (dict(arg=None), "arg is a null pointer"), (dict(gW1=None), "gW1 is a null pointer"),
                    (dict(ws=None), "workspace is a null pointer"), (dict(rows=None), f"R={R} but rows, nrows or gy_rows")):
        assert call(**kw) == 0, kw
        assert _lib.last_error().startswith("houv_mlp2_max_backward: ") and msg in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    with pytest.raises(_lib.HouvHipError, match="come together"):
        ops.mlp2_max_backward(x, W1, s1, W2, arg, gp, rows=rows)
    with pytest.raises(_lib.HouvHipError, match="expected torch.int32"):
        ops.mlp2_max_backward(x, W1, s1, W2, arg.long(), gp)
    with pytest.raises(_lib.HouvHipError, match="CPU tensor"):
        ops.mlp2_max_backward(x.cpu(), W1, s1, W2, arg, gp)
    ops.register_torch_ops()
    a = torch.ops.houv.mlp2_max_backward(x, W1, s1, W2, arg, gp, rows, nrows, gy)
    b = ops.mlp2_max_backward(x, W1, s1, W2, arg, gp, rows, nrows, gy, want_gx=True)
    assert all(torch.equal(u, b[k]) for u, k in zip(a, ("gW1", "gshift1", "gW2", "gb2", "act_rows", "nact", "gx_rows")))


# ------------------------------------------------------------------------------------------------------- the encoder
def _encoder_case():
    """Seeded encoder weights (tests/golden/pcn_weights.py), B = 2, N = 65, and the first cloud seed below 64 for which, in the
    float64 forward, every ReLU input and every pool's lead over its runner-up is at least 4x that quantity's float32-vs-float64
    spread: the masks and both arg-max decisions are then the same in any careful float32 evaluation."""
    if "enc" in _BW:
        return _BW["enc"]
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import pcn_weights
    state = {k[len("encoder."):]: v for k, v in pcn_weights.make_state(16).items() if k.startswith("encoder.")}
    w = {k: np.asarray(v).reshape(v.shape[0], -1) if k.endswith("weight") else np.asarray(v) for k, v in state.items()}
    G = np.random.default_rng(5).uniform(-1, 1, (2, 1024)).astype(np.float32)
    for seed in range(64):
        x = np.random.default_rng(seed).uniform(-0.5, 0.5, (2, 65, 3)).astype(np.float32)
        f64, _, a1, a2, q64 = ghost.encoder_backward(w, x, G, np.float64, backward=False)
        f32, _, b1, b2, q32 = ghost.encoder_backward(w, x, G, np.float32, backward=False)
        ok = np.array_equal(a1, b1) and np.array_equal(a2, b2)
        for u, v in zip(q64[2:], q32[2:]):
            ok = ok and float(np.abs(u).min()) >= 4 * float(np.abs(u - v).max())
        for u, v in zip(q64[:2], q32[:2]):
            top = np.sort(u, 1)
            ok = ok and float((top[:, -1] - top[:, -2]).min()) >= 4 * float(np.abs(u - v).max())
        if ok:
            break
    else:
        raise AssertionError("no cloud seed below 64 keeps the encoder clear of its kinks")
    g64, g32 = (ghost.encoder_backward(w, x, G, t)[1] for t in (np.float64, np.float32))
    _BW["enc"] = dict(state=state, x=x, G=G, feat=f64, grads=g64, bounds={k: 8 * float(np.abs(g32[k] - g64[k]).max()) for k in g64},
                      feat_bound=8 * float(np.abs(f32 - f64).max()), seed=seed)
    return _BW["enc"]


def test_encoder_trainable_gradients_vs_float64(dev):
    """PCN_encoder(trainable=True): the feature keeps the inference path's bits, and the eight parameter gradients of <G, feat>
    are within 8x the float32 restatement's own error (the model-level factor of test_gpu_pcn.py) of the float64 restatement
    in the reference's un-split, materialising form.  trainable=False, and no_grad, still give a feature without a graph."""
    from houv_amd.models.pcn import PCN_encoder
    c = _encoder_case()
    nets = {t: PCN_encoder(trainable=t) for t in (False, True)}
    for net in nets.values():
        net.load_state_dict({k: T(v) for k, v in c["state"].items()}, strict=True)
        net.to(dev)
    x, G = T(c["x"]).to(dev), T(c["G"]).to(dev)
    plain = nets[False](x)
    feat = nets[True](x)
    assert not plain.requires_grad and feat.requires_grad and np.array_equal(_bits(feat.detach()), _bits(plain))
    with torch.no_grad():
        assert not nets[True](x).requires_grad
    assert float(np.abs(plain.cpu().numpy() - c["feat"]).max()) <= c["feat_bound"]
    (feat * G).sum().backward()
    first = {}
    for name, p in nets[True].named_parameters():
        got = p.grad.cpu().numpy().reshape(c["grads"][name].shape)
        err = float(np.abs(got - c["grads"][name]).max())
        print("encoder seed", c["seed"], name, "error", err, "bound", c["bounds"][name], "largest", float(np.abs(c["grads"][name]).max()))
        assert err <= c["bounds"][name], name
        first[name] = p.grad.clone()
        p.grad = None
    (nets[True](x) * G).sum().backward()
    for name, p in nets[True].named_parameters():
        assert np.array_equal(_bits(p.grad), _bits(first[name])), name                # two passes: identical bits
    with pytest.raises(ValueError, match="requires_grad"):
        nets[True](x.clone().requires_grad_())


def test_encoder_trains_under_adam(dev):
    """20 Adam steps (lr 1e-3) pulling the feature of one fixed batch towards a fixed target lower the loss; a state-dict round
    trip after the steps loads strictly (the packed weight copies are remade once the optimizer has written the weights).
    The target lies 2 G away from the present feature (a mean square of 4/3): Adam's first steps move every weight by about lr
    whatever the gradient's size, 2.5 % of a conv3 weight's range per step, so a target closer than the feature moves under
    such a step cannot be approached at this rate (measured with 0.1 G: 0.0034 -> 0.0045)."""
    from houv_amd.models.pcn import PCN_encoder
    c = _encoder_case()
    net = PCN_encoder(trainable=True)
    net.load_state_dict({k: T(v) for k, v in c["state"].items()}, strict=True)
    net.to(dev)
    x = T(c["x"]).to(dev)
    target = T(c["feat"].astype(np.float32)).to(dev) + 2 * T(c["G"]).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = ((net(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("encoder loss before", losses[0], "after", losses[-1])
    assert losses[-1] < losses[0]
    other = PCN_encoder()
    other.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad():
        assert np.array_equal(_bits(other.to(dev)(x)), _bits(net(x)))
