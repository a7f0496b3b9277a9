"""GPU: SA_SKN_Res_encoder(trainable=True): in eval() the graph-building path keeps the bits and the trace
of the inference path, every parameter and the input get a finite non-zero gradient, two runs give the same bits, train() applies
the reference's two dropouts reproducibly, the gradients match the float64 restatement of tests/vrcnet_enc_grad_host.py under the
model's own traced decisions within 8x the restatement's float32 spread (the project's model-level bound), the REAL reference's
fixture (g31_vrcnet_enc_grad.npz) goes through the encoder's own pooling and up-sampling nodes, Adam lowers a loss, `out=` is
refused on the graph path and Model's "train" prefix still raises."""
import numpy as np
import pytest
import torch

import vrcnet_cases as cases
import vrcnet_enc_grad_cases as ec
import vrcnet_enc_grad_host as egh
import vrcnet_grad_host as gh

pytestmark = pytest.mark.gpu
T = torch.tensor
ARGS = (cases.ENC_K, cases.ENC_PK, cases.ENC_PTS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _encoder(dev, trainable, state=None, **kw):
    from houv_amd.models.vrcnet import SA_SKN_Res_encoder
    kw = dict(dict(pts_num=list(cases.ENC_PTS), k=list(cases.ENC_K), pk=cases.ENC_PK), **kw)
    net = SA_SKN_Res_encoder(trainable=trainable, **kw)
    if state is not None:
        net.load_state_dict({n: T(v) for n, v in state.items()}, strict=True)
    return net.to(dev).eval()


def _grads(net, rows, G, trace=None):
    """-> (out, {name: gradient} with 'x' for the input's) of L = <G, out>."""
    net.zero_grad(set_to_none=True)
    x = rows.detach().clone().requires_grad_(True)
    out = net.forward_rows(x, trace)
    (out * G).sum().backward()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()}
    grads["x"] = x.grad
    return out.detach(), grads


@pytest.fixture(scope="module")
def case(dev):
    B, seed = ec.TRAIN_CASE
    x, G = ec.inputs_encoder(B, seed)
    rows = lambda a: T(np.ascontiguousarray(np.swapaxes(a, 1, 2))).to(dev)
    return cases.encoder_state(), x, G, rows(x), rows(G)


def test_eval_keeps_the_bits_and_the_trace_of_the_inference_path(dev, case):
    state, _, _, rows, _ = case
    t0, t1, t2 = {}, {}, {}
    plain = _encoder(dev, False, state).forward_rows(rows, t0)
    assert not plain.requires_grad
    net = _encoder(dev, True, state)
    assert all(u.trainable for u in (net.sam_res1, net.sam_res2, net.sam_res3, net.sam_res4))
    with_graph = net.forward_rows(rows.clone().requires_grad_(True), t1)
    assert with_graph.requires_grad and torch.equal(with_graph.detach(), plain)
    with torch.no_grad():                                                         # grad mode off: the inference path itself
        off = net.forward_rows(rows, t2)
    assert not off.requires_grad and torch.equal(off, plain)
    assert sorted(t0) == sorted(t1) == sorted(t2) == sorted(egh.decision_names(cases.ENC_K))
    assert all(torch.equal(t0[n], t1[n]) and torch.equal(t0[n], t2[n]) for n in t0)
    # the reference's layout: (B,C,N) in, (B,out,N) out, with a graph
    y = net(rows.transpose(1, 2).contiguous().requires_grad_(True))
    assert y.requires_grad and torch.equal(y.detach(), plain.transpose(1, 2).contiguous())
    assert not _encoder(dev, False, state)(rows.transpose(1, 2).contiguous().requires_grad_(True)).requires_grad
    assert sorted(net.state_dict()) == sorted(state)                              # dropout adds nothing to the state_dict
    buf = torch.empty_like(plain)
    assert _encoder(dev, False, state).forward_rows(rows, out=buf) is buf and torch.equal(buf, plain)
    with pytest.raises(ValueError, match="`out` is not served"):
        net.forward_rows(rows, out=buf)


def test_every_parameter_and_the_input_get_a_gradient_and_two_runs_give_the_same_bits(dev, case):
    _, _, _, rows, G = case
    torch.manual_seed(11)
    net = _encoder(dev, True, k=[10, 16], layers=(1, 1, 1, 1))                    # two lists: the branch softmax has a gradient
    _, a = _grads(net, rows, G)
    _, b = _grads(net, rows, G)
    assert set(a) == {n for n, _ in net.named_parameters()} | {"x"}
    for n in a:
        assert a[n] is not None and bool(torch.isfinite(a[n]).all()) and bool(a[n].any()), n
        assert torch.equal(a[n], b[n]), n


def test_train_mode_applies_dropout_reproducibly(dev, case):
    state, _, _, rows, G = case
    net = _encoder(dev, True, state)
    plain, ge = _grads(net, rows, G)
    net.train()
    torch.manual_seed(5)
    o1, g1 = _grads(net, rows, G)
    torch.manual_seed(5)
    o2, g2 = _grads(net, rows, G)
    assert torch.equal(o1, o2) and all((g1[n] is None and g2[n] is None) or torch.equal(g1[n], g2[n]) for n in g1)
    assert not torch.equal(o1, plain) and not torch.equal(g1["fc1.weight"], ge["fc1.weight"])
    with torch.no_grad():                                                         # no graph: the inference path, no dropout
        assert torch.equal(net.forward_rows(rows), plain)


def test_gradients_against_the_float64_restatement_under_the_models_decisions(dev, case):
    state, x, G, rows, Gr = case
    trace = {}
    out, grads = _grads(_encoder(dev, True, state), rows, Gr, trace)
    dec = {n: trace[n].cpu().numpy().astype(np.int64) for n in egh.decision_names(cases.ENC_K)}
    k64, k32, t64 = [], [], []
    o64, bw64 = egh.encoder(state, x, dec, *ARGS, np.float64, "", k64, t64, coords=x)
    o32, bw32 = egh.encoder(state, x, dec, *ARGS, np.float32, "", k32, None, coords=x)
    kink_spread = max(float(np.abs(a32.astype(np.float64) - a64).max()) for (_, a64), (_, a32) in zip(k64, k32))
    lead = min(float((gap if n.endswith("conv5") else np.where(gap == 0, np.inf, gap)).min()) for n, gap in t64)
    print(f"nearest ReLU input {gh.margin(k64):.3g}, smallest lead of a maximum {lead:.3g}, float32 spread {kink_spread:.3g}")
    assert gh.margin(k64) >= 2 * kink_spread and lead >= 2 * kink_spread          # vrcnet_enc_grad_cases.TRAIN_CASE
    assert np.abs(np.swapaxes(out.cpu().numpy(), 1, 2) - o64).max() <= 4 * egh.spread(o32, o64)
    gx64, g64 = bw64(G)
    gx32, g32 = bw32(G)
    r64, r32 = dict(g64, x=gx64), dict(g32, x=gx32)
    worst = ("", 0.0)
    for n in r64:
        if grads[n] is None:                                                      # fc / fcs of a single-list block: exactly 0
            assert ".fc" in n and not r64[n].any(), n
            continue
        got = grads[n].cpu().numpy()
        got = np.swapaxes(got, 1, 2) if n == "x" else got.reshape(r64[n].shape)
        own, err = egh.spread(r32[n], r64[n]), float(np.abs(got - r64[n]).max())
        if own > 0 and err / own > worst[1]:
            worst = (n, err / own)
        assert err <= 8 * own, (n, err, own)
    print(f"encoder gradients: largest error {worst[1]:.2f}x the float32 spread of the restatement ({worst[0]})")


def test_reference_fixture_through_the_encoders_pooling_and_upsampling(dev, golden):
    """g31_vrcnet_enc_grad.npz holds the narrower fixture (no seed qualified for the whole encoder): the REFERENCE's
    edge_preserve_sampling followed by three_nn_upsampling + three_interpolate, 128 -> 64 -> 128 points, and its feature gradient.
    It goes through the encoder's own _pool (the _EdgePoolFunction node) and up-sampling: the traced decisions must equal the
    stored ones, then every stored entry lies within 8x its stored spread."""
    from houv_amd.models.ecg import EF_encoder
    g = golden(ec.FILE)
    assert str(g["kind"]) == "pool_upsample"
    feat, pts, G = ec.inputs_narrow(int(g["seed"]))
    n = ec.NARROW
    net = _encoder(dev, True, pts_num=[n["N"], n["S"], 32, 16], pk=n["pk"])
    f = T(np.ascontiguousarray(np.swapaxes(feat, 1, 2))).to(dev).requires_grad_(True)
    p = T(pts).to(dev)
    trace = {}
    pooled, centres = net._pool(1, f, p, trace, train=True)
    up = EF_encoder._upsample_train(1, pooled, p, centres, trace)
    for name in ("fps1", "knn_pt1", "three_nn1"):
        assert np.array_equal(trace[name].cpu().numpy(), g[f"dec_{name}"]), name
    (up * T(np.ascontiguousarray(np.swapaxes(G, 1, 2))).to(dev)).sum().backward()
    got = np.swapaxes(f.grad.cpu().numpy(), 1, 2).reshape(-1)[g["at_feat"].astype(np.int64)]
    spread = float(g["spread_feat"])
    err64, err_ref = float(np.abs(got - g["f64_feat"]).max()), float(np.abs(got - g["ref_feat"]).max())
    print(f"fixture: device vs float64 {err64 / spread:.2f}x the spread, device vs the reference {err_ref / spread:.2f}x")
    assert err64 <= 8 * spread and err_ref <= 8 * spread


def test_adam_lowers_a_loss_on_a_fixed_batch(dev, case):
    state, _, _, rows, _ = case
    net = _encoder(dev, True, state)
    target = torch.randn(rows.shape[:2] + (ec.OUT_SIZE,), generator=torch.Generator().manual_seed(5)).to(dev)
    mse = lambda: ((net.forward_rows(rows) - target) ** 2).mean()
    with torch.no_grad():
        before = float(mse())
    net.train()
    torch.manual_seed(6)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        loss = mse()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        after = float(mse())
    print(f"MSE without dropout {before:.4f} -> {after:.4f}; with dropout over the 10 steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and after < before


def test_the_train_prefix_still_raises(dev):
    from houv_amd.models.vrcnet import Model
    from vrcnet_cases import vrcnet_weights as W
    with pytest.raises(NotImplementedError):
        Model(W.args()).to(dev)(torch.zeros((1, 3, 2048), device=dev), prefix="train")
