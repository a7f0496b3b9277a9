"""GPU: models.vrcnet on the encoder golden and the three model cases of tests/golden/g27_vrcnet*.npz
(seeded weights from tests/golden/vrcnet_weights.py), under the golden's latent sample z.

As for ECG, the reference does not agree with itself across precisions on its discrete decisions, so parity is stated GIVEN the
decisions and the decisions are checked on their own:
  continuous   the float64 restatement (tests/vrcnet_host.py) run with the MODEL's traced decisions must agree with every stage
               the model records (feat, coarse_raw, coarse_high, coarse, fine) within 4x the fixture's float32-vs-float64 spread
               of that stage;
  agreement    where a `_safe` mask of the fixture holds (the reference's entry is the float64 ranking's and its float64 margin
               exceeds what rounding of the distances and 4x the float32 spread of the rows they are computed from can move) the
               model's entry must equal the reference's, for as long as all earlier decisions agreed; a mask may exclude at
               most vrcnet_cases.MAX_UNSAFE_SHARE of the entries, which the generator asserts for the reference too; the number
               of entries compared is printed."""
import numpy as np
import pytest
import torch

import vrcnet_cases as cases
import vrcnet_host as host
from vrcnet_cases import vrcnet_weights as W

pytestmark = pytest.mark.gpu
T = torch.tensor
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, name, trace=None, **kw):
    from houv_amd.models.vrcnet import Model
    net = Model(W.args(cases.MODEL_CASES[name], **kw), trace=trace)
    net.load_state_dict({k: T(v) for k, v in cases.model_state(name).items()}, strict=True)
    return net.to(dev).eval()


def _run(dev, golden, name):
    """(golden file, the model's stages, its traced decisions, the float64 restatement under those decisions)."""
    if name not in _CACHE:
        g = golden(f"g27_vrcnet_{name}.npz")
        c = cases.MODEL_CASES[name]
        trace = {}
        net = _model(dev, name, trace)
        x, z = T(g["x"]).to(dev), T(g["z"]).to(dev)
        res = net(x, prefix="test", z=z)
        assert sorted(res) == ["result"] and res["result"] is trace["fine"]
        own = {q: trace[q].cpu().numpy() for q in host.STAGES}
        dec = {n: trace[n].cpu().numpy().astype(np.int64) for n in host.decision_names(c)}
        assert sorted(n for n in trace if n not in host.STAGES and n != "z" and not n.endswith("_x")) == sorted(dec)
        assert sorted(n for n in trace if n.endswith("_x")) == sorted(n + "_x" for n in dec if n.startswith("knn_exp"))
        f64, used = host.model(cases.model_state(name), g["x"], c, g["z"], np.float64, dec)
        assert sorted(used) == sorted(dec)
        _CACHE[name] = (g, own, dec, f64, net, x, z)
    return _CACHE[name]


def test_encoder_given_its_decisions_vs_float64(dev, golden):
    from houv_amd.models.vrcnet import SA_SKN_Res_encoder
    g = golden("g27_vrcnet.npz")
    st = cases.encoder_state()
    net = SA_SKN_Res_encoder(pts_num=list(cases.ENC_PTS), k=list(cases.ENC_K), pk=cases.ENC_PK)
    net.load_state_dict({k: T(v) for k, v in st.items()}, strict=True)
    net = net.to(dev).eval()
    trace = {}
    rows = T(g["enc_x"]).to(dev).transpose(1, 2).contiguous()
    got = net.forward_rows(rows, trace).transpose(1, 2).cpu().numpy()
    assert sorted(trace) == sorted(str(n) for n in g["enc_decisions"])
    d = host.eh._Decisions({n: v.cpu().numpy() for n, v in trace.items()})
    f64 = host.encoder(st, g["enc_x"], d, cases.ENC_K, cases.ENC_PK, cases.ENC_PTS, np.float64, prefix="")
    err = float(np.abs(got - f64).max())
    print("encoder vs float64 restatement under its decisions", err, "bound", 4 * float(g["spread_enc"]))
    assert got.shape == (2, 64, cases.ENC_PTS[0]) and err <= 4 * float(g["spread_enc"])
    assert np.array_equal(net(T(g["enc_x"]).to(dev)).cpu().numpy(), got)                  # the reference's layout


@pytest.mark.parametrize("name", list(cases.MODEL_CASES))
def test_model_given_its_decisions_vs_float64(dev, golden, name):
    g, own, dec, f64, _, _, _ = _run(dev, golden, name)
    c = cases.MODEL_CASES[name]
    assert own["fine"].shape == (2, c.num_points, 3) and own["coarse"].shape == (2, c.num_coarse, 3)
    assert own["coarse_raw"].shape == (2, c.num_coarse_raw, 3)
    for q in host.STAGES:
        err = float(np.abs(own[q].astype(np.float64) - f64[q]).max())
        print(name, q, "model vs float64 restatement under the model's decisions", err, "bound", 4 * float(g[f"spread_{q}"]))
    for q in host.STAGES:
        assert float(np.abs(own[q].astype(np.float64) - f64[q]).max()) <= 4 * float(g[f"spread_{q}"]), (name, q)


@pytest.mark.parametrize("name", list(cases.MODEL_CASES))
def test_decisions_agree_with_the_reference_where_its_margin_is_safe(dev, golden, name):
    g, _, dec, _, _, _, _ = _run(dev, golden, name)
    ref = cases.reference_decisions(g, name)
    compared, agreed_so_far = {}, True
    for n in host.decision_names(cases.MODEL_CASES[name]):
        if not agreed_so_far:
            break
        if f"{n}_safe" in g.files:
            safe = cases.safe_mask(g, n)
            assert safe.mean() >= 1 - cases.MAX_UNSAFE_SHARE, (name, n, safe.mean())
            compared[n] = (int(safe.sum()), safe.size)
            bad = int((dec[n] != ref[n])[safe].sum())
            assert bad == 0, f"{name} {n}: {bad} of {safe.sum()} entries with a safe float64 margin differ from the reference"
        agreed_so_far = np.array_equal(dec[n], ref[n])
        if agreed_so_far and n not in compared:
            compared[n] = (ref[n].size, ref[n].size)
    print(name, "entries compared with the reference (compared, of):", compared)
    assert "knn1_0" in compared and compared["knn1_0"][0] >= (1 - cases.MAX_UNSAFE_SHARE) * compared["knn1_0"][1]


def test_val_prefix_and_emd(dev, golden):
    from houv_amd import metrics
    from houv_amd.model_utils_completion import calc_cd
    name = "b"
    g, own, _, _, _, x, z = _run(dev, golden, name)
    gt = torch.cat((x.transpose(1, 2), x.transpose(1, 2), x.transpose(1, 2)), dim=1).contiguous()
    val = _model(dev, name)(x, gt, prefix="val", z=z)
    assert sorted(val) == ["cd_p", "cd_t", "f1", "out1", "out2"]
    assert np.array_equal(val["out2"].cpu().numpy(), own["fine"]) and np.array_equal(val["out1"].cpu().numpy(), own["coarse_raw"])
    cd_p, cd_t, f1 = calc_cd(val["out2"], gt, calc_f1=True)
    d1, d2, _, _ = metrics.cd()(gt, val["out2"])
    for got, want in ((val["cd_p"], cd_p), (val["cd_t"], cd_t), (val["f1"], f1), (val["cd_t"], d1.mean(1) + d2.mean(1))):
        assert tuple(got.shape) == (2,) and bool(torch.isfinite(got).all()) and torch.equal(got, want)
    emd = _model(dev, name, eval_emd=True)(x, gt, prefix="val", z=z)["emd"]
    assert tuple(emd.shape) == (2,) and bool(torch.isfinite(emd).all())


def test_latent_sample_is_drawn_when_z_is_none_and_train_raises(dev, golden):
    name = "a"
    g, own, _, _, net, x, z = _run(dev, golden, name)
    plain = _model(dev, name)
    assert np.array_equal(plain(x, prefix="test", z=z)["result"].cpu().numpy(), own["fine"])     # with and without a trace
    outs = []
    for seed in (1, 2, 1):
        torch.manual_seed(seed)
        outs.append(plain(x, prefix="test")["result"])
    assert tuple(outs[0].shape) == (2, 2048, 3) and bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
    with pytest.raises(NotImplementedError):
        plain(x, x.transpose(1, 2).contiguous(), prefix="train", alpha=0.5)
