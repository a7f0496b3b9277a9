#!/usr/bin/env python3
"""Golden vectors for the VRCNet completion network from the REAL reference, CPU only.

    python tests/golden/make_golden_vrcnet.py

Imports completion/models/vrcnet.py with the stubs, the `torch.arange` patch and the mm3d_pn2 stand-ins of make_golden_ecg.py,
loads the seeded weights of tests/golden/vrcnet_weights.py with strict=True, and runs everything under model.eval() in float32
as it stands.  Written: g27_vrcnet.npz (layer and encoder goldens, state_dict names and shapes) and g27_vrcnet_{a,b,c}.npz, one
per model case -- one file would exceed the size the repository keeps a fixture to.

Layer goldens   the reference SA_module alone (one cloud) at N = 40 for C in {64, 128, 256, 512} and k in {10, 16}, and SK_SA_module with the
                lists [10, 20] at C = 64: these pin the index orders of houv_sa_attn (x2's view, conv_w's view, the repeat over
                share_planes) to the reference.
Encoder golden  SA_SKN_Res_encoder(pts_num=[128, 64, 32, 16], k=[16], pk=10) on 128 points (16 points is the fewest among which
                the reference's knn can list 16 neighbours).
Model cases     vrcnet_cases.MODEL_CASES, B = 2, the "test" prefix.  Stored per case: the input, the latent sample z (recorded by
                wrapping rsample), the reference's DECISIONS (recorded by wrapping its knn, knn_point, furthest_point_sample,
                three_nn and topk; vrcnet_host.decision_names names them), its feat / coarse_raw / coarse_high / coarse / fine
                (outputs subsampled), the float64 forward of tests/vrcnet_host.py WITH THOSE DECISIONS INJECTED, the
                float32-vs-float64 spread of the restatement under the same decisions, and per k-NN decision the mask of entries
                that are the float64 ranking's and whose float64 margin on both sides exceeds what fp32 rounding of the
                distances and 4x the float32 spread of the rows they are computed from can move (`<name>_safe`; `safe_mask`).

The script asserts that the float32 restatement with the reference's decisions reproduces the reference within 4x the spreads,
that no mask excludes more than vrcnet_cases.MAX_UNSAFE_SHARE of its entries, and that every file stays under 1 MiB."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_ecg as mge  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrcnet_cases as cases  # noqa: E402
import vrcnet_host as host  # noqa: E402
from vrcnet_cases import vrcnet_weights as W  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
B = 2
KEEP_EVERY = 5
T = torch.tensor


class Recorder:
    """Wraps the reference's decision functions; records in call order."""

    def __init__(self, mu, vrc):
        self.rec, self.nk = {}, 1
        self.count = dict(knn=0, knn_point=0, fps=0, three_nn=0)
        knn, knn_point, fps, tnn = mu.knn, mu.knn_point, mu.furthest_point_sample, mu.three_nn
        topk, rsample = torch.Tensor.topk, torch.distributions.Normal.rsample

        def w_knn(x, k):
            idx = knn(x, k)
            if x.shape[1] == 3:
                level, i = divmod(self.count["knn"], self.nk)
                self.count["knn"] += 1
                self.rec[f"knn{level + 1}_{i}"] = idx.numpy().copy()
            else:
                self.rec[{256: "knn_exp1", 64: "knn_exp2"}[x.shape[1]]] = idx.numpy().copy()
            return idx

        def numbered(kind, name, fn, pick):
            def w(*a):
                r = fn(*a)
                self.count[kind] += 1
                self.rec[f"{name}{self.count[kind]}"] = pick(r).numpy().copy()
                return r
            return w

        def w_fps_out(xyz, n):
            idx = fps(xyz, n)
            self.rec["fps_out"] = idx.numpy().copy()
            return idx

        def w_topk(t, *a, **k):
            r = topk(t, *a, **k)
            if t.dim() == 3 and t.shape[1] == 1:                         # the decoder's scores [B, 1, M]
                self.rec["topk"] = r[1].reshape(t.shape[0], -1).numpy().copy()
            return r

        def w_rsample(d, *a, **k):
            z = rsample(d, *a, **k)
            self.rec["z"] = z.numpy().copy()                             # before the generator's in-place ReLU
            return z
        mu.knn = vrc.knn = w_knn
        mu.knn_point = numbered("knn_point", "knn_pt", knn_point, lambda r: r[1])
        mu.furthest_point_sample = numbered("fps", "fps", fps, lambda r: r)
        mu.three_nn = numbered("three_nn", "three_nn", tnn, lambda r: r[1])
        vrc.furthest_point_sample = w_fps_out
        torch.Tensor.topk = w_topk
        torch.distributions.Normal.rsample = w_rsample

    def reset(self, nk):
        self.rec, self.nk = {}, nk
        self.count = dict(knn=0, knn_point=0, fps=0, three_nn=0)


def load(module, state):
    module.load_state_dict({k: T(v) for k, v in state.items()}, strict=True)
    return module.eval()


def compare(out, key, ref, f32, f64, keep=None, store_f64=True):
    """Assert the project's rule and store reference, float64 restatement (the tests recompute it where it is left out to keep
    the file small) and spread under `key`."""
    assert f32.dtype == np.float32 and f64.dtype == np.float64 and ref.dtype == np.float32 and ref.shape == f64.shape, key
    spread = float(np.abs(f32.astype(np.float64) - f64).max())
    err = float(np.abs(ref.astype(np.float64) - f64).max())
    print(f"{key}: |.| mean {np.abs(f64).mean():.3g} max {np.abs(f64).max():.3g}; float32 restatement vs float64 {spread:.3g}; "
          f"reference vs float64 {err:.3g}")
    assert err <= 4 * spread, key
    sel = (lambda a: a) if keep is None else (lambda a: a[:, keep])
    out[key], out["spread_" + key] = sel(ref), np.float64(spread)
    if store_f64:
        out[key + "_f64"] = sel(f64)
    if keep is not None:
        out[key + "_idx"] = keep.astype(np.int32)


def save(name, out):
    path = f"{OUT}/{name}"
    np.savez_compressed(path, **out)
    print("wrote", name, "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 2 ** 20, name


def layers(vrc, out, rng):
    rows = lambda t: np.ascontiguousarray(np.swapaxes(t[:, :, 0], 1, 2))
    for C in cases.SA_C:
        for k in cases.LAYER_K:
            st = cases.sa_state(C, k)
            net = load(vrc.SA_module(C, C // 16, C // 4, C, 8, k), st)
            x = rng.standard_normal((1, C, 1, cases.LAYER_N)).astype(np.float32)
            idx = rng.integers(0, cases.LAYER_N, (1, cases.LAYER_N, k))
            with torch.no_grad():
                ref = net([T(x), T(idx)])[0].numpy()
            f32, f64 = (host.sa_module(st, "", x, idx, d) for d in (np.float32, np.float64))
            key = f"sa{C}_{k}"
            out[key + "_x"], out[key + "_idx"] = rows(x), idx.astype(np.int16)
            compare(out, key, rows(ref), rows(f32), rows(f64), store_f64=False)
            ratio = float(np.abs(f64 - x).mean() / np.abs(x).mean())
            print(f"{key}: mean |attention branch| / mean |identity| = {ratio:.3g}")
            assert 0.1 <= ratio <= 10, key
    C, st = 64, cases.sk_state()
    net = load(vrc.SK_SA_module(C, C // 16, C // 4, C, 8, list(cases.SK_KS)), st)
    x = rng.standard_normal((B, C, 1, cases.LAYER_N)).astype(np.float32)
    idxs = [rng.integers(0, cases.LAYER_N, (B, cases.LAYER_N, k)) for k in cases.SK_KS]
    with torch.no_grad():
        ref = net([T(x), [T(i) for i in idxs]])[0].numpy()
    f32, f64 = (host.sk_sa_module(st, "", x, idxs, d) for d in (np.float32, np.float64))
    out["sk_x"] = rows(x)
    for i, idx in enumerate(idxs):
        out[f"sk_idx{i}"] = idx.astype(np.int16)
    compare(out, "sk", rows(ref), rows(f32), rows(f64), store_f64=False)


def safe_mask(rows, idx, eps):
    """rows[B,N,C] float64, idx[B,N,k]: True where the entry is the float64 ranking's and its squared distance d is separated
    from both neighbours in that ranking by more than twice margin(d) = tau d + 4 eps sqrt(C d) + 4 C eps^2: tau d covers the
    fp32 rounding of a direct distance (vrcnet_cases.tau), the rest what moving every channel of both rows by eps can do."""
    C, k = rows.shape[2], idx.shape[2]
    d = host.eh.sqdist_rows(rows, rows)
    order = np.argsort(d, axis=-1, kind="stable")
    assert d.shape[2] > k
    ds = np.take_along_axis(d, order[..., :k + 1], axis=-1)
    margin = cases.tau(C) * ds[..., 1:] + 4 * eps * np.sqrt(C * ds[..., 1:]) + 4 * C * eps * eps
    up = ds[..., 1:] - ds[..., :k] > 2 * margin
    down = np.ones_like(up)
    down[..., 1:] = up[..., :-1]
    return (order[..., :k] == idx) & up & down


def unsafe_share(name, rows, rows32, idx, out):
    """eps: 4x the float32 restatement's own error on the rows the distances are computed from, the project's allowance for
    any float32 implementation."""
    eps = 4 * float(np.abs(rows32.astype(np.float64) - rows).max())
    m = safe_mask(rows, idx, eps)
    out[f"{name}_safe"] = np.packbits(m)
    share = 1 - m.mean()
    print(f"{name}: C = {rows.shape[2]}, eps = {eps:.3g}, {m.size - m.sum()} of {m.size} entries ({100 * share:.2f} %) not the float64 "
          "choice or within the margin of a neighbour")
    assert share <= cases.MAX_UNSAFE_SHARE, name
    return share


def encoder(vrc, recorder, out, rng):
    st = cases.encoder_state()
    net = load(vrc.SA_SKN_Res_encoder(pts_num=list(cases.ENC_PTS), k=list(cases.ENC_K), pk=cases.ENC_PK), st)
    x = rng.uniform(-0.5, 0.5, (B, 3, cases.ENC_PTS[0])).astype(np.float32)
    recorder.reset(len(cases.ENC_K))
    with torch.no_grad():
        ref = net(T(x)).numpy()
    dec = dict(recorder.rec)
    run = lambda d: host.encoder(st, x, host.eh._Decisions(dec), cases.ENC_K, cases.ENC_PK, cases.ENC_PTS, d, prefix="")
    out["enc_x"] = x
    for n, v in dec.items():
        out[f"enc_{n}"] = v.astype(np.int16)
    out["enc_decisions"] = np.array(sorted(dec))
    compare(out, "enc", ref, run(np.float32), run(np.float64), store_f64=False)


def model_case(vrc, recorder, name, keys, rng):
    c = cases.MODEL_CASES[name]
    st = cases.model_state(name)
    net = load(vrc.Model(W.args(c)), st)
    keys[f"{name}_state_keys"] = np.array(list(net.state_dict().keys()))
    keys[f"{name}_state_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in net.state_dict().values()])
    x = rng.uniform(-0.5, 0.5, (B, 3, c.num_input)).astype(np.float32)
    got = {}
    h1 = net.encoder.register_forward_hook(lambda m, i, o: got.__setitem__("feat", o.detach().numpy().copy()))
    h2 = net.decoder.register_forward_hook(lambda m, i, o: got.update(
        {n: t.detach().transpose(1, 2).contiguous().numpy().copy() for n, t in zip(host.STAGES[1:], o)}))
    recorder.reset(len(c.knn_list))
    torch.manual_seed(27)
    with torch.no_grad():
        res = net(T(x), prefix="test")
    h1.remove(); h2.remove()
    assert np.array_equal(res["result"].numpy(), got["fine"])
    z = recorder.rec.pop("z")
    dec = dict(recorder.rec)
    want = host.decision_names(c)
    assert sorted(dec) == sorted(want), (sorted(dec), sorted(want))
    feats32 = {}
    f32, used = host.model(st, x, c, z, np.float32, dec, feats32)
    feats = {}
    f64, _ = host.model(st, x, c, z, np.float64, dec, feats)
    assert all(np.array_equal(used[n], dec[n]) for n in want)
    out = dict(x=x, z=z)
    for n in want:
        out[n] = dec[n].astype(np.int16 if dec[n].max() < 32768 else np.int32)
    shares = [unsafe_share(n, rows, feats32[n], dec[n], out) for n, rows in feats.items()]
    for q in host.STAGES:
        keep = np.arange(0, got[q].shape[1], KEEP_EVERY) if q != "feat" else np.arange(got[q].shape[1])
        compare(out, q, got[q], f32[q], f64[q], keep)
    assert got["fine"].shape == (B, c.num_points, 3) and 0.3 <= np.abs(f64["fine"]).max() <= 30, name
    save(f"g27_vrcnet_{name}.npz", out)
    return max(shares)


def main():
    torch.set_num_threads(8)
    mu, _ = mge.import_ecg()
    import models.vrcnet as vrc
    assert vrc.__file__.startswith(f"{mge.mg.REF}/completion")
    recorder = Recorder(mu, vrc)
    rng = np.random.default_rng(27)
    out = {}
    layers(vrc, out, rng)
    encoder(vrc, recorder, out, rng)
    worst = max(model_case(vrc, recorder, name, out, rng) for name in cases.MODEL_CASES)
    print(f"largest share of entries a mask excludes: {100 * worst:.2f} % (bound {100 * cases.MAX_UNSAFE_SHARE:.0f} %)")
    save("g27_vrcnet.npz", out)


if __name__ == "__main__":
    main()
