"""GPU: models.ecg.Model(trainable=True) on the golden case p512 of tests/golden/g26_ecg.npz (seeded
weights from tests/golden/ecg_weights.py): the trainable path keeps the inference path's bits, total_train_loss.backward() fills
a finite, non-zero gradient of every parameter, the gradients of a linear loss are bit-identical from run to run, Adam lowers
the loss on a fixed batch, the refusals, parity with the float64 restatement under the model's own decisions, and the REAL
reference's EF_encoder gradients (g29_ecg_grad_b.npz) through the device encoder."""
import numpy as np
import pytest
import torch

import ecg_cases as cases
from ecg_cases import ecg_weights

pytestmark = pytest.mark.gpu
T = torch.tensor
NAME = "p512"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, trainable, trace=None, **kw):
    from houv_amd.models.ecg import Model
    num_points, num_coarse, num_input = cases.GOLDEN_CASES[NAME]
    net = Model(ecg_weights.args(num_points, **kw), num_coarse=num_coarse, num_input=num_input, trace=trace, trainable=trainable)
    net.load_state_dict({k: T(v) for k, v in cases.state(NAME).items()}, strict=True)
    return net.to(dev)


@pytest.fixture(scope="module")
def cloud(dev, golden):
    x = T(golden("g26_ecg.npz")[f"{NAME}_x"]).to(dev)
    return x, x.transpose(1, 2).contiguous()


def _linear_loss_grads(net, x, seed=3):
    """The gradients of L = <G1, out1> + <G2, out2> for seeded G1, G2 (out1 from a forward hook on the decoder)."""
    kept = {}
    hook = net.decoder.register_forward_hook(lambda m, i, o: kept.update(out1=o[0], out2=o[1]))
    try:
        net.zero_grad(set_to_none=True)
        res = net(x, prefix="test")
    finally:
        hook.remove()
    assert res["result"] is kept["out2"]
    gen = torch.Generator().manual_seed(seed)
    G1 = torch.randn(kept["out1"].shape, generator=gen).to(x.device)
    G2 = torch.randn(kept["out2"].shape, generator=gen).to(x.device)
    ((kept["out1"] * G1).sum() + (kept["out2"] * G2).sum()).backward()
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}, kept


def test_trainable_keeps_the_bits_of_the_inference_path(dev, cloud):
    x, gt = cloud
    plain, trace_p, trace_t = _model(dev, False, trace={}), {}, {}
    plain.trace = trace_p
    train = _model(dev, True, trace=trace_t)
    a = plain(x, gt, prefix="train", alpha=0.5)
    b = train(x, gt, prefix="train", alpha=0.5)
    assert not a[2].requires_grad and b[2].requires_grad and b[0].requires_grad
    for u, v in zip(a, b):
        assert torch.equal(u, v.detach())
    assert sorted(trace_p) == sorted(trace_t) and all(torch.equal(trace_p[n], trace_t[n]) for n in trace_p)
    va, vb = plain(x, gt, prefix="val"), train(x, gt, prefix="val")
    assert torch.equal(va["out1"], vb["out1"].detach()) and torch.equal(va["out2"], vb["out2"].detach())
    with torch.no_grad():                                                         # grad mode off: no graph, the inference path itself
        c = train(x, gt, prefix="train", alpha=0.5)
    assert not c[2].requires_grad and torch.equal(c[0], a[0]) and torch.equal(c[2], a[2])
    d = _model(dev, False)(x, gt, prefix="train", alpha=0.5)                      # the default never builds a graph, grad mode on or off
    assert not d[2].requires_grad and torch.equal(d[0], a[0])


@pytest.mark.parametrize("loss", ["cd", "emd"])
def test_backward_fills_a_finite_nonzero_gradient_of_every_parameter(dev, cloud, loss):
    x, gt = cloud
    net = _model(dev, True, loss=loss)
    out2, loss2, total = net(x, gt, prefix="train", alpha=0.5)
    total.backward()
    names = [n for n, _ in net.named_parameters()]
    assert len(names) == len(cases.state(NAME)) and any(n.startswith("encoder.") for n in names)
    for n, p in net.named_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), n
        assert bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().max() > 0), n


def test_two_runs_give_the_same_gradient_bits(dev, cloud):
    x, _ = cloud
    net = _model(dev, True)
    a, kept = _linear_loss_grads(net, x)
    b, _ = _linear_loss_grads(net, x)
    assert sorted(a) == sorted(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n
        assert bool(torch.isfinite(a[n]).all()) and bool(a[n].abs().max() > 0), n


def test_adam_lowers_the_loss_on_a_fixed_batch(dev, cloud):
    x, gt = cloud
    net = _model(dev, True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        total = net(x, gt, prefix="train", alpha=0.5)[2]
        total.backward()
        opt.step()
        losses.append(float(total.detach()))
    with torch.no_grad():
        losses.append(float(net(x, gt, prefix="train", alpha=0.5)[2]))
    print("total_train_loss over 20 Adam steps:", " ".join(f"{v:.5f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_refusals(dev, cloud):
    from houv_amd.models.ecg import ECG_decoder, Model
    x, gt = cloud
    net = _model(dev, True)
    with pytest.raises(ValueError, match="x.requires_grad"):
        net(x.clone().requires_grad_(True), gt, prefix="train", alpha=0.5)
    with pytest.raises(NotImplementedError, match="EF_expansion"):
        ECG_decoder(512, 2048, 512, trainable=True)                               # scale 2
    with pytest.raises(NotImplementedError, match="EF_expansion"):
        Model(ecg_weights.args(2048), num_coarse=512, num_input=512, trainable=True)
    assert ECG_decoder(512, 2048, 512).scale == 2                                 # inference still builds it


def test_gradients_against_the_float64_restatement_under_the_traced_decisions(dev, cloud, golden):
    """The gradients of L = <G1, out1> + <G2, out2> against the float64 torch restatement (tests/ecg_grad_host.torch_model, the
    reference's materialising form) under the model's OWN traced decisions: per parameter the relative L2 error stays within 8x
    what the float32 restatement itself shows against float64 (g29_ecg_grad.npz, part (c)).  Measured ratios: DESIGN.md 9.13."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import ecg_grad_host as gh
    import ecg_host as host
    from make_golden_ecg_grad import linear_loss_weights
    x, _ = cloud
    g29 = golden("g29_ecg_grad.npz")
    num_points, num_coarse, _ = cases.GOLDEN_CASES[NAME]
    G1, G2 = linear_loss_weights((x.shape[0], num_coarse, 3), (x.shape[0], num_points, 3))
    trace = {}
    net = _model(dev, True, trace=trace)
    kept = {}
    hook = net.decoder.register_forward_hook(lambda m, i, o: kept.update(out1=o[0], out2=o[1]))
    net(x, prefix="test")
    hook.remove()
    ((kept["out1"] * T(G1).to(dev)).sum() + (kept["out2"] * T(G2).to(dev)).sum()).backward()
    dec = {n: trace[n].cpu().numpy().astype(np.int64) for n in host.DECISIONS if n in trace}
    o64, g64 = gh.torch_model_grads(cases.state(NAME), x.cpu().numpy(), num_points, num_coarse, dec, G1, G2, torch.float64)
    assert np.abs(kept["out2"].detach().cpu().numpy() - o64["out2"]).max() < 1e-3     # the same network under the same decisions
    worst, bad = 0.0, []
    for n, p in net.named_parameters():
        rel = float(np.linalg.norm(p.grad.cpu().numpy().astype(np.float64) - g64[n]) / np.linalg.norm(g64[n]))
        ratio = rel / float(g29[f"{NAME}_rel_{n}"])
        worst = max(worst, ratio)
        if ratio > 8:
            bad.append((n, rel, float(g29[f"{NAME}_rel_{n}"]), ratio))
    print(f"largest ratio of the relative L2 error to the float32 restatement's: {worst:.2f}")
    assert not bad, bad


def test_reference_ef_encoder_gradients_through_the_device_encoder(dev, golden):
    """Fixture (b), g29_ecg_grad_b.npz: the REFERENCE's EF_encoder (hierarchy (32, 24, 16), N = 48, float32 autograd on
    L = <G, out>) through the device EF_encoder(trainable=True).  Its thirteen traced decisions must equal the reference's; then
    every stored gradient entry lies within 8x the stored float32-vs-float64 spread of the float64 restatement."""
    from houv_amd.models.ecg import EF_encoder
    g = golden("g29_ecg_grad_b.npz")
    names = sorted(k[4:] for k in g.files if k.startswith("idx_"))
    net = EF_encoder(hierarchy=(32, 24, 16), trainable=True)
    assert sorted(n for n, _ in net.named_parameters()) == names
    state = {k_[len("decoder.encoder."):]: T(v) for k_, v in ecg_weights.make_state(512, 1).items() if k_.startswith("decoder.encoder.")}
    net.load_state_dict(state, strict=True)
    net.to(dev)
    trace = {}
    out = net.train_rows(T(g["x"]).to(dev).transpose(1, 2).contiguous(), trace)
    decisions = [k for k in g.files if k.startswith(("fps", "knn_", "three_nn"))]
    assert len(decisions) == 13
    for n in decisions:
        assert np.array_equal(trace[n].cpu().numpy().astype(np.int64), g[n].astype(np.int64)), n
    (out * T(g["G"]).to(dev).transpose(1, 2)).sum().backward()
    worst = 0.0
    for n, p in net.named_parameters():
        got = p.grad.cpu().numpy().reshape(-1)[g[f"idx_{n}"]]
        bound = 8 * float(g[f"spread_{n}"])
        assert np.abs(g[f"ref_{n}"] - g[f"f64_{n}"]).max() <= bound, (n, "the reference itself")
        err = float(np.abs(got - g[f"f64_{n}"]).max())
        worst = max(worst, err / float(g[f"spread_{n}"]))
        assert err <= bound, (n, err, bound)
    print(f"fixture (b): largest error / stored spread {worst:.2f} (bound 8)")
