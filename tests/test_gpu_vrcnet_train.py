"""GPU: SA_module, SK_SA_module and SKN_Res_unit with trainable=True: the trainable path keeps the
inference path's bits, every parameter of a unit gets a finite non-zero gradient, two runs give the same bits, the REAL
reference's SKN_Res_unit gradients (g30_vrcnet_grad_b.npz) through the device module, a single-list unit against the float64
restatement, Adam lowers a loss on a fixed batch, and Model's "train" prefix still raises."""
import numpy as np
import pytest
import torch

import vrcnet_grad_cases as gc
import vrcnet_grad_host as gh

pytestmark = pytest.mark.gpu
T = torch.tensor


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows(a):
    """[B,C,1,N] -> rows [B,N,C]."""
    return np.ascontiguousarray(np.swapaxes(a[:, :, 0], 1, 2))


def _load(dev, net, state):
    net.load_state_dict({n: T(v) for n, v in state.items()}, strict=True)
    return net.to(dev)


def _unit(dev, state, trainable, cin=64, cout=64, ks=(10, 20), layers=2):
    from houv_amd.models.vrcnet import SKN_Res_unit
    return _load(dev, SKN_Res_unit(cin, cout, list(ks), layers, trainable=trainable), state)


def _grads(net, x, idxs, G, x_grad=True):
    """-> (out, {name: gradient} with 'x' for the input's) of L = <G, out>."""
    net.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(x_grad)
    out = net.forward_rows(x, idxs)
    (out * G).sum().backward()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()}
    grads["x"] = x.grad
    return out.detach(), grads


@pytest.fixture(scope="module")
def unit_case(dev, golden):
    g = golden(gc.FILE_B)
    state, x, idxs, G = gc.load_b(g)
    dv = lambda a: T(a).to(dev)
    return g, state, x, idxs, G, dv(_rows(x)), [dv(i.astype(np.int32)) for i in idxs], dv(_rows(G))


def test_trainable_keeps_the_bits_of_the_inference_path(dev, unit_case):
    from houv_amd.models.vrcnet import SA_module, SK_SA_module
    _, state, _, _, _, x, idxs, _ = unit_case
    sub = lambda prefix: {n[len(prefix):]: v for n, v in state.items() if n.startswith(prefix)}
    makers = {"SA_module": (lambda t: _load(dev, SA_module(64, 4, 16, 64, 8, 10, trainable=t), sub("sam.0.sams.0.")), lambda i: i[0]),
              "SK_SA_module": (lambda t: _load(dev, SK_SA_module(64, 4, 16, 64, 8, (10, 20), trainable=t), sub("sam.0.")), lambda i: i),
              "SK_SA_module, one list": (lambda t: _load(dev, SK_SA_module(64, 4, 16, 64, 8, (10,), trainable=t),
                                                         {n: v for n, v in sub("sam.0.").items() if "s.1." not in n}), lambda i: i[:1]),
              "SKN_Res_unit": (lambda t: _unit(dev, state, t), lambda i: i)}
    for name, (make, pick) in makers.items():
        plain = make(False).forward_rows(x, pick(idxs))
        assert not plain.requires_grad
        train = make(True)
        with_graph = train.forward_rows(x.clone().requires_grad_(True), pick(idxs))
        assert with_graph.requires_grad, name
        assert torch.equal(plain, with_graph.detach()), name
        with torch.no_grad():                                                     # grad mode off: the inference path itself
            out = train.forward_rows(x, pick(idxs))
        assert not out.requires_grad and torch.equal(plain, out), name
    unit = _unit(dev, state, True)
    assert torch.equal(unit.forward_rows(x, idxs, relu_out=True).detach(), _unit(dev, state, False).forward_rows(x, idxs, relu_out=True))
    with pytest.raises(ValueError, match="`out` is not served"):
        unit.forward_rows(x, idxs, out=torch.empty_like(x))


def test_every_parameter_gets_a_gradient_and_two_runs_give_the_same_bits(dev, unit_case):
    _, state, _, _, _, x, idxs, G = unit_case
    net = _unit(dev, state, True)
    _, a = _grads(net, x, idxs, G)
    _, b = _grads(net, x, idxs, G)
    assert set(a) == set(state) | {"x"}
    for n in a:
        assert a[n] is not None and bool(torch.isfinite(a[n]).all()) and bool(a[n].any()), n
        assert torch.equal(a[n], b[n]), n
    _, c = _grads(net, x, idxs, G, x_grad=False)                                  # the input needs no gradient: the same weights'
    assert c["x"] is None and all(torch.equal(a[n], c[n]) for n in state)


def test_reference_unit_gradients_through_the_device_module(dev, unit_case):
    """Fixture (b): the REFERENCE's SKN_Res_unit(64, 64, [10, 20], 2), float32 autograd on L = <G, out>, through the device
    module: every stored entry within 8x its stored float32-vs-float64 spread (the model-level margin of section 9.13)."""
    g, state, _, _, _, x, idxs, G = unit_case
    _, grads = _grads(_unit(dev, state, True), x, idxs, G)
    worst = ("", 0.0)
    for n in list(state) + ["x"]:
        got = grads[n].cpu().numpy()
        if n == "x":
            got = np.swapaxes(got, 1, 2)                                          # rows -> [B,C,1,N]'s flat order
        at = g[f"unit_at_{n}"].astype(np.int64)
        spread = float(g[f"unit_spread_{n}"])
        err = float(np.abs(got.reshape(-1)[at] - g[f"unit_f64_{n}"]).max())
        if err / spread > worst[1]:
            worst = (n, err / spread)
        assert err <= 8 * spread, (n, err, spread)
    print(f"fixture (b): largest error {worst[1]:.2f}x the spread ({worst[0]})")


def test_single_list_unit_against_the_float64_restatement(dev):
    """SKN_Res_unit(128, 128, [16], 1): one node with relu_out, fc / fcs not evaluated (the restatement gives them exact zeros)."""
    B, N, C, k = 2, 65, 128, 16
    for seed in range(16):
        rng = np.random.default_rng([33, seed])
        state = gh.unit_state(rng, "", C, C, (k,), 1)
        x = rng.standard_normal((B, C, 1, N)).astype(np.float32)
        idxs = [rng.integers(0, N, (B, N, k))]
        G = rng.standard_normal((B, C, 1, N)).astype(np.float32)
        kinks = []
        out64, bw = gh.skn_res_unit({n: np.asarray(v, np.float64) for n, v in state.items()}, "", x, idxs, kinks=kinks)
        if gh.margin(kinks) >= 1e-5:
            break
    assert gh.margin(kinks) >= 1e-5
    gx64, g64 = bw(G)
    gx32, g32 = gh.skn_res_unit(state, "", x, idxs, np.float32)[1](G)
    net = _unit(dev, state, True, C, C, (k,), 1)
    dv = lambda a: T(a).to(dev)
    out, grads = _grads(net, dv(_rows(x)), [dv(idxs[0].astype(np.int32))], dv(_rows(G)))
    assert np.abs(_rows(out64) - out.cpu().numpy()).max() <= 4 * np.abs(gh.skn_res_unit(state, "", x, idxs, np.float32)[0] - out64).max()
    r64, r32 = dict(g64, x=_rows(gx64)), dict(g32, x=_rows(gx32))
    for n in r64:
        if ".fc" in n:                                                            # the softmax over one branch is exactly 1
            assert not r64[n].any() and grads[n] is None, n
            continue
        own = np.abs(r32[n] - r64[n]).max()
        err = np.abs(grads[n].cpu().numpy().reshape(r64[n].shape) - r64[n]).max()
        print(f"single list {n}: error {err:.3e}, float32 restatement {own:.3e}, ratio {err / own:.2f}")
        assert err <= 4 * own, (n, err, own)


def test_adam_lowers_a_loss_on_a_fixed_batch(dev, unit_case):
    _, state, _, _, _, x, idxs, _ = unit_case
    net = _unit(dev, state, True)
    target = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        loss = ((net.forward_rows(x, idxs) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("MSE over 10 Adam steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_the_train_prefix_still_raises(dev):
    from houv_amd.models.vrcnet import Model
    from vrcnet_cases import vrcnet_weights as W
    with pytest.raises(NotImplementedError):
        Model(W.args()).to(dev)(torch.zeros((1, 3, 2048), device=dev), prefix="train")
