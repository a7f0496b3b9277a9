"""GPU: models.deepgmr.Model(args, trainable=True) against the reference's own training step
(tests/golden/g2x_deepgmr_grad.npz: the real deepgmr.py in train() mode on the CPU, float64).  The reference's neighbour lists are
fed in, so the comparison starts from the same discrete decisions; the max-pool rows must then be the fixture's.  A gradient may
differ from the float64 golden by 8 x the fp32-vs-fp64 spread the reference itself shows for that parameter."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import deepgmr_grad_cases as cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import deepgmr_weights  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, trainable=True):
    from houv_amd.models.deepgmr import Model
    net = Model(deepgmr_weights.Args, trainable=trainable) if trainable else Model(deepgmr_weights.Args)
    state = {k: torch.tensor(v) for k, v in deepgmr_weights.make_state(cases.WEIGHT_SEED).items()}
    missing, unexpected = net.load_state_dict(state, strict=False)
    assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing)
    return net.to(dev)


def _step(net, g, name, dev):
    T = lambda k: torch.tensor(g[f"{name}_{k}"], device=dev)
    net.zero_grad(set_to_none=True)
    out = net(T("src"), T("tgt"), T("T_gt"), nbr=(T("knn1"), T("knn2")))
    out[0].backward()
    return out


@pytest.mark.parametrize("name", cases.FIXTURE_CASES)
def test_training_step_matches_the_reference(golden, dev, name):
    g = golden("g2x_deepgmr_grad.npz")
    net = _model(dev).train()
    B, N = g[f"{name}_src"].shape[:2]
    out = _step(net, g, name, dev)
    assert len(out) == 5 and out[0].requires_grad and all(not o.requires_grad for o in out[1:])

    # the rows the max-pool picked, as row indices within each cloud
    for mine, key in ((net.pool_rows1, "pool1"), (net.pool_rows2, "pool2")):
        assert np.array_equal(mine.cpu().numpy() - np.arange(B)[:, None] * N, g[f"{name}_{key}"]), key

    loss64 = float(g[f"{name}_loss_f64"])
    loss_tol = 8 * abs(float(g[f"{name}_loss_f32"]) - loss64)
    loss = out[0].item()
    print(name, "loss", loss, "golden", loss64, "tolerance", loss_tol)
    assert abs(loss - loss64) <= loss_tol

    grads = {k: p.grad for k, p in net.named_parameters()}
    names = [str(k) for k in g["param_names"]]
    assert sorted(grads) == names and len(names) == 23 and all(v is not None for v in grads.values())
    worst = 0.0
    for k in names:
        got, ref, scale = cases.against_golden(g, name, k, grads[k].cpu().numpy())
        ratio = float(np.abs(got - ref).max()) / (float(g[f"{name}_spread_{k}"]) * scale)
        worst = max(worst, ratio)
        print(f"{name} {k}: error {ratio:.2f} spreads (allowed {cases.GRAD_SPREADS})")
    assert worst <= cases.GRAD_SPREADS, worst

    # BatchNorm buffers after the step: two updates per layer (one per cloud), within 8 x the buffer's own recorded spread
    for key, want in cases.golden_buffers(g, name).items():
        got = net.state_dict()[key].cpu().numpy()
        if key.endswith("num_batches_tracked"):
            assert int(got) == int(want) == 2
        else:
            err, tol = float(np.abs(got - want).max()), cases.buffer_tolerance(g, name, key)
            print(f"{name} {key}: error {err:.3e} tolerance {tol:.3e}")
            assert err <= tol, key

    # a second backward pass over the same step gives the same bits
    first = {k: v.clone() for k, v in grads.items()}
    net2 = _model(dev).train()
    _step(net2, g, name, dev)
    for k, p in net2.named_parameters():
        assert torch.equal(p.grad, first[k]), k
    torch.cuda.synchronize()


def test_eval_mode_equals_the_inference_model_bit_for_bit(golden, dev):
    g = golden("g2x_deepgmr_grad.npz")
    src, tgt, T_gt = (torch.tensor(g[f"n64_{k}"], device=dev) for k in ("src", "tgt", "T_gt"))
    a, b = _model(dev, trainable=True).eval(), _model(dev, trainable=False).eval()
    assert torch.equal(a(src, tgt, prefix="test"), b(src, tgt, prefix="test"))
    for x, y in zip(a(src, tgt, T_gt), b(src, tgt, T_gt)):
        assert torch.equal(x, y)
    assert torch.equal(a.gamma1, b.gamma1) and torch.equal(a.sigma2, b.sigma2)
    # the inference model in train() mode is still the inference model: no graph, buffers untouched
    before = copy.deepcopy(b.state_dict())
    out = b.train()(src, tgt, T_gt)
    assert not out[0].requires_grad and all(torch.equal(v, before[k]) for k, v in b.state_dict().items())
    assert sorted(a.state_dict()) == [str(k) for k in g["state_keys"]]
    torch.cuda.synchronize()


def test_use_tnet_is_refused():
    from argparse import Namespace
    from houv_amd.models.deepgmr import Model
    with pytest.raises(NotImplementedError):
        Model(Namespace(use_rri=False, rri_size=20, num_groups=16, use_tnet=True), trainable=True)


def test_thirty_adam_steps_lower_the_loss(golden, dev):
    """30 Adam steps (lr 1e-3) on one fixed batch of 2 x 64 points, the fixture's n64 clouds, with the model's own neighbour lists.
    On this batch the reference itself (deepgmr.py in train() mode on the CPU, weights seed 2024) goes from a loss of 0.7046 to 0.0226."""
    g = golden("g2x_deepgmr_grad.npz")
    src, tgt, T_gt = (torch.tensor(g[f"n64_{k}"], device=dev) for k in ("src", "tgt", "T_gt"))
    net = _model(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = net(src, tgt, T_gt)[0]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("loss", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    torch.cuda.synchronize()
