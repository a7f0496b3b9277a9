"""CPU: the NumPy backward passes of tests/vrcnet_grad_host.py (the yardsticks of houv_sa_attn_backward and of the trainable
SA_module / SK_SA_module / SKN_Res_unit) against central differences in float64 (clamped out-of-range
indices included), their forwards against vrcnet_host, and the fixtures g30_vrcnet_grad*.npz against the float64 restatement."""
import os

import numpy as np
import pytest

import vrcnet_grad_host as gh
import vrcnet_host as vh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lists(rng, B, N, k, wild=False):
    idx = rng.integers(0, N, (B, N, k))
    if wild:                                                                      # clamped to 0 and to N - 1
        idx[:, ::3, 0] = -3
        idx[:, 1::4, k - 1] = N + 5
    return idx


def _central(loss, arrays, grads, rng, n=6, eps=1e-6, tol=2e-6):
    """d loss / d arrays[name][entry] by central differences at n seeded entries per array against grads[name]."""
    for name, a in arrays.items():
        flat = a.reshape(-1)
        for e in rng.choice(flat.size, min(n, flat.size), replace=False):
            keep = flat[e]
            flat[e] = keep + eps
            up = loss()
            flat[e] = keep - eps
            down = loss()
            flat[e] = keep
            num, ana = (up - down) / (2 * eps), grads[name].reshape(-1)[e]
            assert abs(num - ana) <= tol * max(1.0, abs(ana), np.abs(grads[name]).max()), (name, int(e), num, ana)


@pytest.mark.parametrize("C,k,wild", [(64, 4, False), (64, 5, True), (128, 3, True)])
def test_sa_attn_backward_against_central_differences(C, k, wild):
    rng = np.random.default_rng(C + k)
    B, N = 2, 9
    c = gh.op_case(3, B, N, C, k, idx=_lists(rng, B, N, k, wild))
    c64 = {n: (np.asarray(v, np.float64) if n != "idx" else v) for n, v in c.items()}
    r = gh.sa_attn_backward(**c64)
    # L = <G, relu(o)>: ro's gradient is G, which is what the call is given
    loss = lambda: float((c64["G"] * gh.sa_attn_backward(**c64)["ro"]).sum())
    arrays = {"gP": c64["P"], "gWw1": c64["Ww1"], "gWw2": c64["Ww2"], "gbw2": c64["bw2"]}
    _central(loss, arrays, r, rng)
    if wild:                                                                      # the same as the clamped lists, bit for bit
        cl = dict(c64, idx=np.clip(c["idx"], 0, N - 1))
        r2 = gh.sa_attn_backward(**cl)
        assert all(np.array_equal(r[n], r2[n]) for n in gh.OP_GRADS)


def _module_case(kind, seed, wild=False):
    rng = np.random.default_rng(seed)
    B, N = 2, 9
    if kind == "sa":
        C, ks = 64, (4,)
        state = gh.sa_state(rng, "", C, 4)
        fn = lambda st, x, idxs, **kw: gh.sa_module(st, "", x, idxs[0], **kw)
        host = lambda st, x, idxs: vh.sa_module(st, "", x, idxs[0])
    elif kind == "sa_relu":
        C, ks = 64, (3,)
        state = gh.sa_state(rng, "", C, 3)
        fn = lambda st, x, idxs, **kw: gh.sa_module(st, "", x, idxs[0], relu_out=True, **kw)
        host = lambda st, x, idxs: vh.relu(vh.sa_module(st, "", x, idxs[0]))
    elif kind == "sk":
        C, ks = 64, (3, 5)
        state = gh.sk_state(rng, "", C, ks)
        fn = lambda st, x, idxs, **kw: gh.sk_sa_module(st, "", x, idxs, **kw)
        host = lambda st, x, idxs: vh.sk_sa_module(st, "", x, idxs)
    else:
        C, ks = 64, (3, 4)
        state = gh.unit_state(rng, "u.", 5 if kind == "unit" else 64, C, ks, 2 if kind == "unit" else 1)
        fn = lambda st, x, idxs, **kw: gh.skn_res_unit(st, "u.", x, idxs, **kw)
        host = lambda st, x, idxs: vh.skn_res_unit(st, "u.", x, idxs)
    cin = state["u.conv1.weight"].shape[1] if kind.startswith("unit") else C
    x = rng.standard_normal((B, cin, 1, N))
    idxs = [_lists(rng, B, N, k, wild) for k in ks]
    G = rng.standard_normal((B, C, 1, N))
    return state, x, idxs, G, fn, host


@pytest.mark.parametrize("kind,wild", [("sa", False), ("sa", True), ("sa_relu", True), ("sk", False), ("sk", True), ("unit", False),
                                       ("unit1", True)])
def test_module_backward_against_central_differences_and_forward_against_vrcnet_host(kind, wild):
    for seed in range(16):                                                        # inputs whose ReLU inputs stay clear of 0
        state, x, idxs, G, fn, host = _module_case(kind, 100 * seed + len(kind) + wild, wild)
        st64 = {n: np.asarray(v, np.float64) for n, v in state.items()}
        kinks = []
        out, bw = fn(st64, x, idxs, kinks=kinks)
        if gh.margin(kinks) >= 1e-5:
            break
    assert gh.margin(kinks) >= 1e-5, "a ReLU input is too close to 0 for central differences"
    if not wild:                                                                  # vrcnet_host does not clamp
        assert np.array_equal(out, host(st64, x, idxs))
    out32 = fn(state, x, idxs, dtype=np.float32)[0]
    assert out32.dtype == np.float32 and np.abs(out32 - out).max() <= 1e-4 * max(1.0, np.abs(out).max())
    gx, grads = bw(G)
    assert set(grads) == set(state)
    loss = lambda: float((G * fn(st64, x, idxs)[0]).sum())
    _central(loss, dict(st64, x=x), dict(grads, x=gx), np.random.default_rng(5), n=4)


def test_af_is_the_identity_on_value_and_gradient():
    """SKN_Res_unit's self.af meets an SK_SA_module's output, which is >= 0; dropping the ReLU changes neither the value nor the
    gradient: where the output is 0 every branch is 0 and the branch masks have dropped the element already."""
    state, x, idxs, G, fn, _ = _module_case("unit", 3)
    st64 = {n: np.asarray(v, np.float64) for n, v in state.items()}
    kinks = []
    fn(st64, x, idxs, kinks=kinks)
    af = dict(kinks)["u.af"]
    assert af.min() >= 0 and (af == 0).any(), "the case should contain exact zeros at af"
    out, bw = fn(st64, x, idxs)
    gx, grads = bw(G)
    out2, bw2 = fn(st64, x, idxs, af_mask=False)
    gx2, grads2 = bw2(G)
    assert np.array_equal(out, out2) and np.array_equal(gx, gx2) and all(np.array_equal(grads[n], grads2[n]) for n in grads)


def _fixture(name):
    path = os.path.join(GOLDEN, name)
    assert os.path.exists(path), f"{name} is missing: python tests/golden/make_golden_vrcnet_grad.py"
    return np.load(path)


def check_entries(g, key, names, grads64):
    """Every stored entry of the fixture: the stored float64 value is the restatement's, and the reference lies within 4x the
    stored spread of it."""
    for n in names:
        at = g[f"{key}_at_{n}"].astype(np.int64)
        mine = np.asarray(grads64[n]).reshape(-1)[at]
        assert np.allclose(mine, g[f"{key}_f64_{n}"], rtol=1e-12, atol=1e-14), (key, n)
        assert (np.abs(g[f"{key}_ref_{n}"].astype(np.float64) - mine) <= 4 * float(g[f"{key}_spread_{n}"])).all(), (key, n)


@pytest.mark.parametrize("C", (64, 128, 256, 512))
@pytest.mark.parametrize("k", (10, 16))
def test_fixture_a_is_the_float64_restatement(C, k):
    import vrcnet_grad_cases as gc
    g = _fixture(gc.file_a(C))
    key = f"sa{C}_{k}"
    state, x, idx, G = gc.load_a(g, key)
    kinks = []
    out, bw = gh.sa_module({n: np.asarray(v, np.float64) for n, v in state.items()}, "", x, idx, kinks=kinks)
    gx, grads = bw(G)
    assert gh.margin(kinks) >= 4 * float(g[f"{key}_kink_spread"])
    check_entries(g, key, list(state) + ["x"], dict(grads, x=gx))


def test_fixture_b_is_the_float64_restatement():
    import vrcnet_grad_cases as gc
    g = _fixture(gc.FILE_B)
    state, x, idxs, G = gc.load_b(g)
    kinks = []
    out, bw = gh.skn_res_unit({n: np.asarray(v, np.float64) for n, v in state.items()}, "", x, idxs, kinks=kinks)
    gx, grads = bw(G)
    assert gh.margin(kinks) >= 4 * float(g["unit_kink_spread"])
    check_entries(g, "unit", list(state) + ["x"], dict(grads, x=gx))
