"""GPU: VRCNet's Model(trainable=True) and its "train" prefix, at the decoder shapes of
tests/test_gpu_ef_expand_train.py (B = 1, which the prefix doubles; 1024 input points, 512 raw coarse points, one attention layer
per level, one list of 16) in the two cases that cover both expansions and the folding, a ground truth of 2048 points, seeded
weights (tests/golden/vrcnet_weights.py).  The latent head against the real reference's stored values and gradients
(tests/golden/make_golden_vrcnet_train.py) within 8x the stored float32 spread, test_model_gradients_vs_reference_golden's factor;
the loss against its formula; who gets a gradient; run-to-run bits of a whole step; ten Adam steps; every refusal; the inference
prefixes, bit for bit under either flag and grad mode; the state dict."""
import types

import numpy as np
import pytest
import torch

import vrcnet_host
import vrcnet_train_host as head_host
from vrcnet_cases import vrcnet_weights as W

pytestmark = pytest.mark.gpu
T = torch.tensor
ALPHA = 0.5

CASES = {
    "two_expansions": dict(num_coarse_raw=512, num_fps=2048, num_coarse=1024, num_points=3072, local_folding=False),   # up_scale 2, step 3
    "folding": dict(num_coarse_raw=512, num_fps=1280, num_coarse=1024, num_points=2048, local_folding=True),           # up_scale 1, step 2
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cfg(case):
    return vrcnet_host.cfg(layers=(1, 1, 1, 1), knn_list=(16,), pk=10, points_label=False, num_input=1024, **CASES[case])


def _model(dev, case, trainable=True, trace=None, **overrides):
    from houv_amd.models.vrcnet import Model
    c = _cfg(case)
    net = Model(W.args(c, **overrides), trace=trace, trainable=trainable)
    state = W.make_state(W.spec(c), W.SEED + 23)
    net.load_state_dict({n: T(v) for n, v in state.items()}, strict=True)
    return net.to(dev)


def _batch(dev, B=1):
    gen = torch.Generator().manual_seed(31)
    x = (torch.rand(B, 3, 1024, generator=gen) - 0.5).to(dev)
    gt = (torch.rand(B, 2048, 3, generator=gen) - 0.5).to(dev)
    eps = tuple(torch.randn(B, 128, generator=gen).to(dev) for _ in range(2))
    return x, gt, eps


def _step(net, x, gt, eps, seed=41):
    """One "train" step from the net's state: (fine, loss4_t, total, {name: grad})."""
    for p in net.parameters():
        p.grad = None
    torch.manual_seed(seed)                              # the encoder's two dropouts draw from torch's generator
    fine, loss4_t, total = net(x, gt, prefix="train", alpha=ALPHA, eps=eps)
    total.backward()
    return fine.detach(), loss4_t.detach(), total.detach(), {n: p.grad for n, p in net.named_parameters()}


def test_head_against_the_reference_fixture(dev, golden):
    g = golden("g33_vrcnet_train_head.npz")
    state, fx, fy, eq, ep, G = head_host.case(int(g["seed"]))
    assert np.array_equal(fx, g["feat_x"]) and np.array_equal(ep, g["eps_p"])
    net = _model(dev, "folding")
    own = net.state_dict()
    own.update({n: T(v).to(dev) for n, v in state.items()})
    net.load_state_dict(own, strict=True)
    lx, ly = T(fx).to(dev).requires_grad_(True), T(fy).to(dev).requires_grad_(True)
    vals = dict(zip(("q_mu", "q_std", "p_mu", "p_std", "z", "global_feat", "dl_rec", "dl_g"),
                    net._latent_head(lx, ly, (T(eq).to(dev), T(ep).to(dev)))))
    (20 * (vals["dl_rec"].mean() + vals["dl_g"].mean()) + (T(G).to(dev) * vals["global_feat"]).sum()).backward()
    grads = {n: p.grad for n, p in net.named_parameters() if n in state}
    grads.update(feat_x=lx.grad, feat_y=ly.grad)
    assert sorted(grads) == sorted(["feat_x", "feat_y"] + list(state)) and all(v is not None for v in grads.values())
    worst = 0.0
    for kind, mine in (("", vals), ("grad_", grads)):
        for n, t in mine.items():
            got = t.detach().cpu().numpy().reshape(-1).astype(np.float64)
            if f"{kind}{n}_idx" in g.files:
                got = got[g[f"{kind}{n}_idx"].astype(np.int64)]
            spread = float(g[f"spread_{kind}{n}"])
            e64 = float(np.abs(got - g[f"f64_{kind}{n}"]).max()) / spread
            eref = float(np.abs(got - g[f"ref_{kind}{n}"]).max()) / spread
            worst = max(worst, e64, eref)
            print(f"{kind}{n}: device vs float64 {e64:.2f}x the spread, device vs the reference {eref:.2f}x")
            assert e64 <= 8 and eref <= 8, kind + n
    print(f"latent head: worst ratio {worst:.2f}x of the 8x allowed")


@pytest.mark.parametrize("case", sorted(CASES))
def test_loss_value_gradients_and_run_to_run_bits(dev, case):
    from houv_amd.model_utils_completion import calc_cd
    trace = {}
    net = _model(dev, case, trace=trace).train()
    x, gt, eps = _batch(dev)
    fine, loss4_t, total, grads = _step(net, x, gt, eps)
    c = _cfg(case)
    assert tuple(fine.shape) == (2, c.num_points, 3) and tuple(loss4_t.shape) == (2,) and total.dim() == 0
    # the trace: the parts of the loss, the latent head's values and the sample of the ground truth
    for n in ("fps_gt", "q_mu", "q_std", "p_mu", "p_std", "z", "dl_rec", "dl_g", "loss1", "loss2", "loss3", "loss4"):
        assert n in trace, n
    assert tuple(trace["fps_gt"].shape) == (1, 1024) and tuple(trace["z"].shape) == (2, 128)
    assert torch.equal(trace["z"][:1], trace["q_mu"] + trace["q_std"] * eps[0])
    assert torch.equal(trace["z"][1:], trace["p_mu"] + trace["p_std"] * eps[1])
    assert torch.equal(trace["fine"], fine)
    gt2 = torch.cat((gt, gt), 0)
    with torch.no_grad():
        parts = [calc_cd(trace[n].detach(), gt2) for n in ("coarse_raw", "coarse_high", "coarse", "fine")]
        for i, (p, _) in enumerate(parts):
            assert torch.equal(p, trace[f"loss{i + 1}"].detach())
        assert torch.equal(parts[3][1], loss4_t)
        want = parts[0][0].mean() * 10 + parts[1][0].mean() * 0.5 + parts[2][0].mean() + parts[3][0].mean() * ALPHA
        want = want + (trace["dl_rec"].mean() + trace["dl_g"].mean()) * 20
    assert torch.equal(want, total)
    # who gets a gradient
    for n, gr in grads.items():
        if n.startswith("decoder.conv_s") or ".fc." in n or ".fcs." in n:      # scores select rows; one list: fc / fcs not evaluated
            assert gr is None, n
        else:
            assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) > 0, n
    assert all(grads[f"prior_infer.{l}.weight"] is not None for l in ("conv1", "conv2", "conv_res"))
    assert grads["decoder.conv_cup2.weight"] is not None
    # a second step from the same state, eps and dropout seed: the same bits everywhere
    fine2, loss4_t2, total2, grads2 = _step(net, x, gt, eps)
    assert torch.equal(fine, fine2) and torch.equal(loss4_t, loss4_t2) and torch.equal(total, total2)
    differ = [n for n in grads if grads[n] is not None and not torch.equal(grads[n], grads2[n])]
    assert not differ, differ
    # without a graph: the same tuple.  The graph-free decoder is the inference path, whose dropouts are the identity, so the
    # two are compared in eval().  Up to the decoder's first expansion both paths issue the same kernels on the same operands
    # (PCN_encoder, Linear_ResBlock and SA_SKN_Res_encoder carry the inference bits in eval(); every linear layer is the same
    # houv_gemm_f32 call), so everything recorded up to there is equal bit for bit; the folding case has no EF_expansion at
    # all (up_scale 1, Folding's two paths add the same three parts in the same order) and is equal to the last bit of total.
    # Past an EF_expansion node the paths differ within fp32 spread (tests/test_gpu_ef_expand_train.py measures it) and a
    # neighbour list or the top-k may then choose differently, which no fixed figure bounds: those parts are printed.
    with torch.no_grad(), pytest.warns(UserWarning, match="dropouts are the identity"):       # train() mode: said aloud
        net(x, gt, prefix="train", alpha=ALPHA, eps=eps)
    net.eval()
    f_eval, l_eval, t_eval, _ = _step(net, x, gt, eps)
    with_graph = dict(trace)
    with torch.no_grad():
        f3, l3, t3 = net(x, gt, prefix="train", alpha=ALPHA, eps=eps)
    assert not t3.requires_grad and t3.grad_fn is None and not f3.requires_grad and not l3.requires_grad
    assert tuple(f3.shape) == tuple(fine.shape) and tuple(l3.shape) == (2,) and torch.isfinite(f3).all()
    same = ["feat", "fps_gt", "q_mu", "q_std", "p_mu", "p_std", "z", "global_feat", "dl_rec", "dl_g", "coarse_raw", "loss1"]
    if case == "folding":
        same += ["coarse_high", "coarse", "fine", "loss2", "loss3", "loss4", "fps_out", "topk"]
    for n in same:
        assert torch.equal(trace[n], with_graph[n]), n
    if case == "folding":
        assert torch.equal(f3, f_eval) and torch.equal(l3, l_eval) and torch.equal(t3, t_eval)
    print(f"{case} in eval(): total {float(t_eval):.5f} with a graph, {float(t3):.5f} without; largest difference of a coordinate "
          f"of fine {float((f3 - f_eval).abs().max()):.3e}, of loss4_t {float((l3 - l_eval).abs().max()):.3e}")
    # the Chamfer share of total that may differ (loss2..4 past the first expansion) is a few units against the KL terms' 1e4
    assert torch.allclose(t3, t_eval, rtol=1e-3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_adam_lowers_the_total_loss(dev, case):
    net = _model(dev, case).train()
    x, gt, eps = _batch(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for i in range(11):
        opt.zero_grad(set_to_none=True)
        torch.manual_seed(51)
        total = net(x, gt, prefix="train", alpha=ALPHA, eps=eps)[2]
        losses.append(float(total.detach()))
        if i < 10:
            total.backward()
            opt.step()
    print(f"{case}: total {losses[0]:.5f} -> {losses[-1]:.5f} after 10 Adam steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_refusals(dev):
    x, gt, eps = _batch(dev)
    kw = dict(prefix="train", alpha=ALPHA, eps=eps)
    with pytest.raises(NotImplementedError, match="mmd_loss2"):
        _model(dev, "folding", distribution_loss="MMD")(x, gt, **kw)
    with pytest.raises(NotImplementedError, match="MMD or KLD"):
        _model(dev, "folding", distribution_loss="JS")(x, gt, **kw)
    with pytest.raises(NotImplementedError, match="Only CD"):
        _model(dev, "folding", loss="emd")(x, gt, **kw)
    net = _model(dev, "folding")
    with pytest.raises(ValueError, match="gt and alpha"):
        net(x, gt, prefix="train", eps=eps)
    with pytest.raises(ValueError, match="gt and alpha"):
        net(x, None, prefix="train", alpha=ALPHA, eps=eps)
    with pytest.raises(ValueError, match="x.requires_grad"):
        net(x.clone().requires_grad_(True), gt, **kw)
    with pytest.raises(ValueError, match="eps must be"):
        net(x, gt, prefix="train", alpha=ALPHA, eps=(eps[0], eps[1][:, :64]))
    with pytest.raises(NotImplementedError, match="trainable=True"):
        _model(dev, "folding", trainable=False)(x, gt, **kw)             # the default model still raises
    from houv_amd.models.vrcnet import Model
    with pytest.raises(NotImplementedError):
        Model(W.args()).to(dev)(torch.zeros((1, 3, 2048), device=dev), prefix="train")


@pytest.mark.parametrize("case", sorted(CASES))
def test_inference_prefixes_and_state_dict(dev, case):
    tr, tf = {}, {}
    net, frozen = _model(dev, case, trace=tr).eval(), _model(dev, case, trainable=False, trace=tf).eval()
    assert list(net.state_dict()) == list(frozen.state_dict())
    frozen.load_state_dict(net.state_dict(), strict=True)                 # round trip, either way
    net.load_state_dict(frozen.state_dict(), strict=True)
    x, gt, _ = _batch(dev, B=2)
    z = torch.randn(2, 128, generator=torch.Generator().manual_seed(61)).to(dev)
    want = frozen(x, prefix="test", z=z)["result"]
    want_val = frozen(x, gt, prefix="val", z=z)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            got = net(x, prefix="test", z=z)["result"]
            val = net(x, gt, prefix="val", z=z)
            again = frozen(x, prefix="test", z=z)["result"]
        assert not got.requires_grad and torch.equal(got, want) and torch.equal(again, want)
        assert sorted(val) == sorted(want_val) and all(torch.equal(val[n], want_val[n]) for n in val)
    assert sorted(tr) == sorted(tf)


def test_linear_resblock_carries_the_inference_bits(dev):
    from houv_amd.models.vrcnet import Linear_ResBlock
    torch.manual_seed(71)
    for n_in, n_out in ((1024, 1024), (1024, 256), (128, 1024)):
        blk = Linear_ResBlock(n_in, n_out, trainable=True).to(dev).eval()
        for rows in (1, 2, 48):
            f = torch.randn(rows, n_in, device=dev)
            graph = blk(f.clone().requires_grad_(True))
            with torch.no_grad():
                plain = blk(f)
            assert graph.requires_grad and not plain.requires_grad and torch.equal(graph.detach(), plain), (n_in, n_out, rows)
