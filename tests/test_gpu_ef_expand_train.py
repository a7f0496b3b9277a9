"""GPU: EF_expansion(trainable=True) and MSAP_SKN_decoder(trainable=True).  The node against the real
reference's float32 autograd and the float64 restatement on the stored fixtures (tests/golden/make_golden_ef_expand_grad.py), within
8x the stored float32 spread (section 9.15's bound); the graph path against the inference path within the 4x rule of
tests/test_gpu_ef_expand.py; grad mode off; then the decoder in the two cases that cover both expansions and the folding:
who gets a gradient, run-to-run bits, ten Adam steps on a Chamfer loss, the refusals, and Model's "train" prefix, which still raises."""
import numpy as np
import pytest
import torch

import ef_expand_cases as cases
import ef_expand_host as host

pytestmark = pytest.mark.gpu
T = torch.tensor


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _module(dev, name, w, trainable=True):
    from houv_amd.model_utils_completion import EF_expansion
    c = cases.GRAD_CFG[name]
    net = EF_expansion(c["C"], c["O"], step_ratio=c["r"], k=c["k"], trainable=trainable)
    net.load_state_dict({n: T(v).view(net.state_dict()[n].shape) for n, v in w.items()}, strict=True)
    return net.to(dev)


@pytest.mark.parametrize("name", sorted(cases.GRAD_FILES))
def test_reference_fixture(dev, golden, name):
    g = golden(cases.GRAD_FILES[name])
    x, idx, w, G, r = cases.grad_case(name, int(g["seed"]))
    assert np.array_equal(x, g["x"]) and np.array_equal(idx, g["idx"])
    net = _module(dev, name, w)
    rows = T(x).to(dev).requires_grad_(True)
    out = net.forward_rows(rows, idx=T(idx).to(dev))
    (out * T(G).to(dev)).sum().backward()
    o64, _, g64 = host.block(x, idx, *(w[n] for n in cases.PARAMS), r, np.float64, G)
    got = {n: p.grad.cpu().numpy().reshape(w[n].shape) for n, p in net.named_parameters()}
    worst = {}

    def hold(label, mine, f64, ref):
        spread = float(g[f"spread_{label}"])
        e64, eref = float(np.abs(mine - f64).max()) / spread, float(np.abs(mine - ref).max()) / spread
        worst[label] = (round(e64, 2), round(eref, 2))
        print(f"fixture {name} (seed {int(g['seed'])}, qualifies={bool(g['qualifies'])}) {label}: device vs float64 {e64:.2f}x the "
              f"spread, device vs the reference {eref:.2f}x")
        assert e64 <= 8 and eref <= 8, label

    hold("out", out.detach().cpu().numpy(), o64, g["ref_out"])
    hold("x", rows.grad.cpu().numpy(), g64["x"], g["ref_x"])
    for n in cases.PARAMS:
        at = g[f"at_{n}"].astype(np.int64)
        assert np.allclose(g64[n].reshape(-1)[at], g[f"f64_{n}"], rtol=1e-9, atol=1e-12)
        hold(n, got[n].reshape(-1)[at], g[f"f64_{n}"], g[f"ref_{n}"])


@pytest.mark.parametrize("name", sorted(cases.GRAD_FILES))
def test_graph_path_against_the_inference_path_and_grad_mode_off(dev, name):
    x, idx, w, G, r = cases.grad_case(name, 1)
    net = _module(dev, name, w).eval()
    before = {n: v.clone() for n, v in net.state_dict().items()}
    rows, ix = T(x).to(dev), T(idx).to(dev)
    graph = net.forward_rows(rows, idx=ix)
    assert graph.requires_grad and graph.grad_fn is not None
    with torch.no_grad():
        plain = net.forward_rows(rows, idx=ix)
    frozen = _module(dev, name, w, trainable=False)
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, frozen.forward_rows(rows, idx=ix))                  # the inference path itself, bit for bit
    assert not frozen.forward_rows(rows.clone().requires_grad_(True), idx=ix).requires_grad
    o64, _ = host.block(x, idx, *(w[n] for n in cases.PARAMS), r, np.float64)
    o32, _ = host.block(x, idx, *(w[n] for n in cases.PARAMS), r, np.float32)
    spread = float(np.abs(o32 - o64).max())
    eg, ep = float(np.abs(graph.detach().cpu().numpy() - o64).max()), float(np.abs(plain.cpu().numpy() - o64).max())
    print(f"{name}: graph path vs float64 {eg:.3e}, inference path vs float64 {ep:.3e}, float32 restatement vs float64 {spread:.3e}")
    assert eg <= 4 * spread and ep <= 4 * spread
    tr = {}
    net.forward_rows(rows, trace=tr, name="knn_exp1")
    tr2 = {}
    frozen.forward_rows(rows, trace=tr2, name="knn_exp1")
    assert sorted(tr) == sorted(tr2) == ["knn_exp1", "knn_exp1_x"] and all(torch.equal(tr[n], tr2[n]) for n in tr)
    assert sorted(net.state_dict()) == sorted(before) and all(torch.equal(v, net.state_dict()[n]) for n, v in before.items())
    assert sorted(net.state_dict()) == sorted(frozen.state_dict())


# the smallest sizes the encoder's hard-coded pts_num = [3072, 1536, 768, 384] allow: 512 + 1024 = 1536 points enter it
DECODERS = {
    "two_expansions": dict(num_coarse_raw=512, num_fps=2048, num_coarse=1024, num_fine=3072, local_folding=False),    # up_scale 2, step 3
    "folding": dict(num_coarse_raw=512, num_fps=1280, num_coarse=1024, num_fine=2048, local_folding=True),            # up_scale 1, step 2
}


def _decoder(dev, case, trainable=True):
    from houv_amd.models.vrcnet import MSAP_SKN_decoder
    torch.manual_seed(11)
    net = MSAP_SKN_decoder(layers=(1, 1, 1, 1), knn_list=(16,), pk=10, trainable=trainable, **DECODERS[case]).to(dev)
    net.eval()                                   # the encoder's two dropouts are the identity: runs repeat bit for bit
    gen = torch.Generator().manual_seed(12)
    feat = torch.randn(1, 1024, generator=gen).to(dev)
    pts = (torch.rand(1, 1024, 3, generator=gen) - 0.5).to(dev)
    return net, feat, pts


def _backward(net, feat, pts, with_coarse=False):
    """L = <G, fine> + <G', coarse_raw> (+ <G'', coarse>) -> (the gradient of global_feat, of every parameter, fine)."""
    for p in net.parameters():
        p.grad = None
    feat = feat.clone().requires_grad_(True)
    coarse_raw, coarse_high, coarse, fine = net(feat, pts)
    gen = torch.Generator().manual_seed(13)
    G1, G2, G3 = (torch.randn(t.shape, generator=gen).to(t.device) for t in (fine, coarse_raw, coarse))
    loss = (fine * G1).sum() + (coarse_raw * G2).sum()
    if with_coarse:
        loss = loss + (coarse * G3).sum()
    loss.backward()
    return feat.grad, {n: p.grad for n, p in net.named_parameters()}, fine.detach()


@pytest.mark.parametrize("case", sorted(DECODERS))
def test_decoder_gradients_reach_what_the_forward_evaluates(dev, case):
    net, feat, pts = _decoder(dev, case)
    assert (net.expansion1 is not None) == (case == "two_expansions")
    gfeat, grads, fine = _backward(net, feat, pts)
    assert tuple(fine.shape) == (1, DECODERS[case]["num_fine"], 3)
    assert torch.isfinite(gfeat).all() and float(gfeat.abs().max()) > 0
    # Without the folding, `fine` is computed from the selected features alone: conv_cup2's output (coarse_high, coarse) selects
    # rows and is returned, but no path leads from it to fine or coarse_raw, in the reference either.  Its gradient is checked
    # below with <G'', coarse> added to L.
    no_path = ("conv_cup2.weight", "conv_cup2.bias") if case == "two_expansions" else ()
    for n, gr in grads.items():
        unevaluated = n.startswith("conv_s") or ".fc." in n or ".fcs." in n
        if unevaluated or n in no_path:
            assert gr is None, n
        else:
            assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) > 0, n
    _, with_coarse, _ = _backward(net, feat, pts, with_coarse=True)
    for n, gr in with_coarse.items():
        if n.startswith("conv_s") or ".fc." in n or ".fcs." in n:
            assert gr is None, n
        else:
            assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) > 0, n
    gfeat2, grads2, fine2 = _backward(net, feat, pts)
    assert torch.equal(fine, fine2) and torch.equal(gfeat, gfeat2)
    assert all((grads[n] is None and grads2[n] is None) or torch.equal(grads[n], grads2[n]) for n in grads)


@pytest.mark.parametrize("case", sorted(DECODERS))
def test_decoder_adam_lowers_the_chamfer_loss(dev, case):
    from houv_amd.model_utils_completion import calc_cd
    net, feat, pts = _decoder(dev, case)
    target = (torch.rand(1, DECODERS[case]["num_fine"], 3, generator=torch.Generator().manual_seed(14)) - 0.5).to(dev)
    loss_of = lambda: calc_cd(net(feat, pts)[3], target)[1].mean()
    with torch.no_grad():
        before = float(loss_of())
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        loss = loss_of()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        after = float(loss_of())
    print(f"{case}: Chamfer loss {before:.5f} -> {after:.5f}; over the 10 steps:", " ".join(f"{v:.5f}" for v in losses))
    assert all(np.isfinite(losses)) and after < before


def test_decoder_refusals_and_inference_path(dev):
    net, feat, pts = _decoder(dev, "folding")
    with pytest.raises(ValueError, match="point_input"):
        net(feat, pts.clone().requires_grad_(True))
    frozen, _, _ = _decoder(dev, "folding", trainable=False)
    frozen.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad():
        a = net(feat, pts)
    b = frozen(feat.clone().requires_grad_(True), pts)
    assert all(not t.requires_grad for t in a + b) and all(torch.equal(u, v) for u, v in zip(a, b))


def test_the_train_prefix_still_raises(dev):
    from houv_amd.models.vrcnet import Model
    from vrcnet_cases import vrcnet_weights as W
    with pytest.raises(NotImplementedError):
        Model(W.args()).to(dev)(torch.zeros((1, 3, 2048), device=dev), prefix="train")
