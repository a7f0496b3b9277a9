#!/usr/bin/env python3
"""Golden GRADIENTS of ECG's Dense_conv from the REAL reference, CPU only.

    python tests/golden/make_golden_ecg_grad.py

Part (a) of the fixture plan: completion/models/ecg.py's `Dense_conv` alone (imported with the stand-ins of make_golden_ecg.py),
growth rate 24, dense_n 3, k = 16, with seeded weights, float32 autograd on L = <G, out> for a seeded G, with and without the
caller's outer F.relu.  Cases: C in {24, 48} x N in {17, 33} x relu in {0, 1}, B = 2.

A gradient is discontinuous where a ReLU input is 0 or two pool candidates are equal, so the input is CHOSEN: the seeds 0, 1, ...
(cap 512) are walked and the first is taken for which, in the float64 forward of the NumPy restatement
(tests/ecg_grad_host.py) under the reference's own k-NN lists, every ReLU input (the outer one included) has |pre| >= delta and
every pool has its runner-up at least delta below the maximum, delta = 4x the float32-vs-float64 spread of the activations.  (The
one exemption is an exact tie at 0, which only ReLU outputs produce: it carries no gradient whoever wins, and the ReLU margins
already cover it.  s2 has no activation and is never exempt.)  Nothing is ever masked out; if no seed passes, the script raises.

Stored in g29_ecg_grad.npz per case: x[B,C,N], idx[B,N,16] (the reference's own lists), G, the six weights (per shape), the reference's seven
float32 gradients (gx as [B,C,N]), the float64 restatement's, and per gradient the float32-vs-float64 spread of the restatement
(the maximum over the tensor).  The script asserts that the float32 restatement lies within 4x that spread of the reference.

Part (c), no reference run: for the input p512 of g26_ecg.npz (seeded weights of ecg_weights.py) the whole network restated in
torch on the CPU (ecg_grad_host.torch_model, the reference's materialising form) is differentiated in float32 and in float64
under the REFERENCE's decisions stored in g26, loss L = <G1, out1> + <G2, out2> with G1, G2 = linear_loss_weights(); stored per
parameter: the relative L2 error of the float32 gradient against the float64 one (p512_rel_<name>).

Part (b), g29_ecg_grad_b.npz (a file of its own: one file may not exceed 1 MiB): the REAL reference's `EF_encoder` with
hierarchy (32, 24, 16) and k = 16 on N = 48 points, B = 2 (B = 1 if no seed passes at 2; if none passes there either the script
raises), the seeded weights decoder.encoder.* of ecg_weights.py, float32 autograd on L = <G, out>.  The seed walk asks, in
float64 (ecg_host.ef_encoder for the decisions, ecg_grad_host.torch_model(encoder_only="") for the activations), for every ReLU
input, every pool margin and every decision margin, with two exemptions that the network's structure forces (under the literal
rule the walk over 0..511 raised at B = 2 and at B = 1, and every seed failed on these alone): a ReLU input that is exactly 0
and a pool whose two largest candidates are exactly equal.  In float64 neither happens by chance: an exact 0 is what an
earlier ReLU clamped (the outer F.relu of a Dense_conv sees its y0 / s1 maxima and the pass-through x0 again), and an exact tie
is one upstream element met twice (a Dense_conv's centre columns, several neighbours clamped at 0, two sampled points whose
neighbourhood maxima came from the same point one level up); the gradient reaches the same upstream element, or none, whoever
wins.  Everything else must clear its margin -- for decisions the gaps between consecutive entries of each k-NN and
three-NN list up to the first one left out, and between the maximum and the runner-up of every furthest-point step -- to be at
least 4x the float32-vs-float64 spread of the same quantity, and for the reference's own recorded decisions to equal the
float64 ones.  Stored: x, G, the thirteen decisions, and per parameter at most 2048 seeded entries (flat indices, the reference's
float32 gradients there, the float64 restatement's, and the float32-vs-float64 spread of the restatement over the whole
tensor).  The script asserts that the float32 restatement lies within 4x the spread of the reference on every entry of every
tensor."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ecg_weights  # noqa: E402
import make_golden_ecg as mge  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ecg_grad_host as gh  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
B, K, CAP = 2, 16, 512
G = gh.G
WNAMES = ("W0", "b0", "W1", "b1", "W2", "b2")


def weights(C, seed):
    rng = np.random.default_rng(1000 + seed)
    u = lambda shape, fan: rng.uniform(-1, 1, shape).astype(np.float32) / np.float32(np.sqrt(fan))
    return dict(W0=u((G, 2 * C), 2 * C / 3), b0=u((G,), 8), W1=u((G, G + C), (G + C) / 3), b1=u((G,), 8),
                W2=u((G, 2 * G + C), (2 * G + C) / 3), b2=u((G,), 8))


def margins(w, x_rows, idx, relu_out):
    """(the smallest margin, delta) of the float64 forward: ReLU inputs, positive pools, the outer ReLU."""
    f64 = gh.dense_conv_forward_rows(x_rows, idx, **w)
    f32 = gh.dense_conv_forward_rows(x_rows, idx, **w, dtype=np.float32)
    delta = 4 * max(float(np.abs(f32[n] - f64[n]).max()) for n in ("z0", "z1", "full"))
    C = x_rows.shape[2]
    top = np.sort(f64["full"][..., gh.pooled_columns(C)], axis=2)
    gap = np.where((top[:, :, -1] == 0) & (top[:, :, -2] == 0), np.inf, top[:, :, -1] - top[:, :, -2])   # an exact tie at the ReLU's 0
    m = min(float(np.abs(f64["z0"]).min()), float(np.abs(f64["z1"]).min()), float(gap.min()))
    if relu_out:
        out = f64["full"].max(2)
        live = np.ones(out.shape[-1], bool)
        live[:G] = live[G + C:2 * G + C] = False                                  # y0 and s1 are >= 0 already: covered by z0, z1
        m = min(m, float(np.abs(out[..., live]).min()))
    return m, delta


def linear_loss_weights(shape1, shape2):
    """The seeded G1, G2 of part (c), float32, as the tests regenerate them."""
    return (np.random.default_rng(11).standard_normal(shape1).astype(np.float32),
            np.random.default_rng(12).standard_normal(shape2).astype(np.float32))


def whole_model(out):
    import ecg_cases as cases
    import ecg_host as host
    name = "p512"
    g26 = np.load(os.path.join(OUT, "g26_ecg.npz"))
    num_points, num_coarse, _ = cases.GOLDEN_CASES[name]
    state, x = cases.state(name), g26[f"{name}_x"]
    dec = {n: g26[f"{name}_{n}"] for n in host.DECISIONS if f"{name}_{n}" in g26.files}
    G1, G2 = linear_loss_weights((x.shape[0], num_coarse, 3), (x.shape[0], num_points, 3))
    o64, g64 = gh.torch_model_grads(state, x, num_points, num_coarse, dec, G1, G2, torch.float64)
    o32, g32 = gh.torch_model_grads(state, x, num_points, num_coarse, dec, G1, G2, torch.float32)
    f64 = host.model(state, x, num_points, num_coarse, np.float64, dec)[0]
    assert all(np.abs(o64[n] - f64[n]).max() <= 1e-11 for n in f64)               # the torch restatement is ecg_host's network
    for n in g64:
        rel = float(np.linalg.norm(g32[n] - g64[n]) / np.linalg.norm(g64[n]))
        assert np.isfinite(rel) and rel > 0, n
        out[f"{name}_rel_{n}"] = np.float64(rel)
    rels = [float(out[f"{name}_rel_{n}"]) for n in g64]
    print(f"{name}: {len(rels)} parameters, relative L2 of float32 against float64 {min(rels):.2e} .. {max(rels):.2e}")


HIER_B, N_B, KEEP = (32, 24, 16), 48, 2048
DEC_B = ("fps1", "knn_pt1", "fps2", "knn_pt2", "fps3", "knn_pt3", "knn_feat1", "knn_feat2", "knn_feat3", "knn_feat4", "three_nn1",
         "three_nn2", "three_nn3")


def _list_margin(a64, b64, k):
    """(the smallest gap between consecutive entries of the sorted squared distances up to the first one left out of a k-list,
    4x the float32-vs-float64 spread of the distances) for queries a[B,N,C] against b[B,M,C]."""
    import ecg_host as host
    d64 = host.sqdist_rows(a64, b64)
    d32 = host.sqdist_rows(a64.astype(np.float32), b64.astype(np.float32))
    s = np.sort(d64, axis=-1)[..., :k + 1]
    return float(np.diff(s, axis=-1).min()), 4 * float(np.abs(d32 - d64).max())


def _fps_margin(p64, idx):
    """The same for furthest_point_sample's arg-max steps along the recorded sample idx[B,S] of p[B,N,3]."""
    m, spread = np.inf, 0.0
    for b in range(p64.shape[0]):
        md64, md32, p32 = np.full(p64.shape[1], 1e10), np.full(p64.shape[1], 1e10, np.float32), p64[b].astype(np.float32)
        for j in range(1, idx.shape[1]):
            d64, d32 = p64[b] - p64[b, idx[b, j - 1]], p32 - p32[idx[b, j - 1]]
            md64 = np.minimum(md64, (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2])
            md32 = np.minimum(md32, (d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2])
            top = np.sort(md64)
            m, spread = min(m, float(top[-1] - top[-2])), max(spread, float(np.abs(md32 - md64).max()))
    return m, 4 * spread


def _kink_margins(k64, k32):
    """[(margin, delta)] over every recorded ReLU input and pool of ecg_grad_host.torch_model."""
    res = []
    for a64, a32 in zip(k64["relu"], k32["relu"]):
        live = np.abs(a64[a64 != 0])                                              # an exact 0: what an earlier ReLU clamped
        res.append((float(live.min()) if live.size else np.inf, 4 * float(np.abs(a32 - a64).max())))
    for a64, a32 in zip(k64["pool"], k32["pool"]):
        top = np.sort(a64, axis=-1)
        gap = top[..., -1] - top[..., -2] if a64.shape[-1] > 1 else np.array(np.inf)
        gap = np.where(gap == 0, np.inf, gap)                                     # an exact tie: copies of one element
        res.append((float(gap.min()), 4 * float(np.abs(a32 - a64).max())))
    return res


def encoder_b(mu, ecg, rec):
    import ecg_host as host
    state = {n[len("decoder.encoder."):]: v for n, v in ecg_weights.make_state(512, 1).items() if n.startswith("decoder.encoder.")}
    net = ecg.EF_encoder(growth_rate=G, dense_n=3, k=K, hierarchy=list(HIER_B), input_size=3, output_size=256).float()
    net.load_state_dict({n: torch.tensor(v) for n, v in state.items()}, strict=True)
    saved, host.HIERARCHY = host.HIERARCHY, HIER_B
    try:
        for Bb in (2, 1):
            for seed in range(CAP):
                x = np.random.default_rng(seed).uniform(-0.5, 0.5, (Bb, 3, N_B)).astype(np.float32)
                feats, dec = {}, host._Decisions(None)
                host.ef_encoder(state, x, dec, np.float64, prefix="", features=feats)
                D = dec.used
                pcs = [np.ascontiguousarray(np.swapaxes(x, 1, 2)).astype(np.float64)]
                for i in (1, 2, 3):
                    pcs.append(np.take_along_axis(pcs[-1], D[f"fps{i}"][:, :, None], axis=1))
                pairs = [_list_margin(feats[f"knn_feat{i}"], feats[f"knn_feat{i}"], K) for i in (1, 2, 3, 4)]
                pairs += [_list_margin(pcs[i], pcs[i - 1], K) for i in (1, 2, 3)]
                pairs += [_list_margin(pcs[3 - i], pcs[4 - i], 3) for i in (1, 2, 3)]
                pairs += [_fps_margin(pcs[i - 1], D[f"fps{i}"]) for i in (1, 2, 3)]
                if any(m < d for m, d in pairs):
                    continue
                Gm = np.random.default_rng(8000 + seed).standard_normal((Bb, 256, N_B)).astype(np.float32)
                k64, k32 = {}, {}
                o64, g64 = gh.torch_encoder_grads(state, x, D, Gm, torch.float64, k64)
                o32, g32 = gh.torch_encoder_grads(state, x, D, Gm, torch.float32, k32)
                kinks = _kink_margins(k64, k32)
                if any(m < d for m, d in kinks):
                    continue
                rec.reset()
                for p_ in net.parameters():
                    p_.grad = None
                y = net(torch.tensor(x))
                if sorted(rec.rec) != sorted(DEC_B) or any(not np.array_equal(rec.rec[n], D[n]) for n in DEC_B):
                    continue                                                      # the reference's float32 ranking decided otherwise
                (y * torch.tensor(Gm)).sum().backward()
                assert np.abs(y.detach().numpy() - o64).max() <= 1e-3
                ref = {n: p_.grad.numpy() for n, p_ in net.named_parameters()}
                out = dict(x=x, G=Gm, seed=np.int64(seed),
                           margin=np.array([min(m / d for m, d in pairs + kinks)]))
                for n in DEC_B:
                    out[n] = D[n].astype(np.int32)
                for j, n in enumerate(sorted(state)):
                    a64, a32, r = g64[n].reshape(-1), g32[n].reshape(-1), ref[n].reshape(-1)
                    spread = float(np.abs(a32 - a64).max())
                    assert np.abs(a32 - r).max() <= 4 * spread, (n, float(np.abs(a32 - r).max()), spread)
                    keep = np.sort(np.random.default_rng(9000 + j).permutation(a64.size)[:KEEP]).astype(np.int32)
                    out[f"idx_{n}"], out[f"ref_{n}"], out[f"f64_{n}"], out[f"spread_{n}"] = keep, r[keep].copy(), a64[keep], np.float64(spread)
                print(f"(b) B={Bb}: seed {seed}, smallest margin / delta {float(out['margin'][0]):.2f}, {len(state)} parameters")
                return out
        raise RuntimeError(f"(b): no seed below {CAP} keeps the EF_encoder clear of its kinks and decisions at B = 2 or B = 1")
    finally:
        host.HIERARCHY = saved


def main():
    torch.set_num_threads(8)
    mu, ecg = mge.import_ecg()
    rec = mge.Recorder(mu, ecg)
    path_b = os.path.join(OUT, "g29_ecg_grad_b.npz")
    np.savez_compressed(path_b, **encoder_b(mu, ecg, rec))
    print(f"wrote {path_b}: {os.path.getsize(path_b)} bytes")
    rec.on = False
    out = {}
    whole_model(out)
    for C in (24, 48):
        for N in (17, 33):
            for relu_out in (0, 1):
                name = f"c{C}n{N}r{relu_out}"
                w = weights(C, C + N)
                net = ecg.Dense_conv(C, growth_rate=G, dense_n=3, k=K).float()
                sd = {"first_conv.weight": w["W0"][:, :, None, None], "first_conv.bias": w["b0"],
                      "model.stack_conv_1.model.conv.weight": w["W1"][:, :, None, None], "model.stack_conv_1.model.conv.bias": w["b1"],
                      "model.stack_conv_2.model.conv.weight": w["W2"][:, :, None, None], "model.stack_conv_2.model.conv.bias": w["b2"]}
                net.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
                for seed in range(CAP):
                    x = np.random.default_rng(seed).standard_normal((B, C, N)).astype(np.float32)
                    idx = mu.knn(torch.tensor(x), K).numpy()
                    m, delta = margins(w, np.ascontiguousarray(np.swapaxes(x, 1, 2)), idx, relu_out)
                    if m >= delta:
                        break
                else:
                    raise RuntimeError(f"no seed below {CAP} keeps {name} clear of its kinks")
                Gm = np.random.default_rng(7000 + seed).standard_normal((B, C + 3 * G, N)).astype(np.float32)
                xt = torch.tensor(x, requires_grad=True)
                y = net(xt)
                assert tuple(y.shape) == (B, C + 3 * G, N)
                if relu_out:
                    y = F.relu(y)
                net.zero_grad()
                (y * torch.tensor(Gm)).sum().backward()
                ref = dict(gx=xt.grad.numpy(), gW0=net.first_conv.weight.grad.numpy()[:, :, 0, 0], gb0=net.first_conv.bias.grad.numpy(),
                           gW1=net.model.stack_conv_1.model.conv.weight.grad.numpy()[:, :, 0, 0],
                           gb1=net.model.stack_conv_1.model.conv.bias.grad.numpy(),
                           gW2=net.model.stack_conv_2.model.conv.weight.grad.numpy()[:, :, 0, 0],
                           gb2=net.model.stack_conv_2.model.conv.bias.grad.numpy())
                rows, g_rows = np.ascontiguousarray(np.swapaxes(x, 1, 2)), np.ascontiguousarray(np.swapaxes(Gm, 1, 2))
                r64 = gh.dense_conv_backward(rows, idx, **w, gout=g_rows, relu_out=bool(relu_out))
                r32 = gh.dense_conv_backward(rows, idx, **w, gout=g_rows, relu_out=bool(relu_out), dtype=np.float32)
                assert np.array_equal(r32["arg"], r64["arg"]), name
                out[f"{name}_x"], out[f"{name}_idx"], out[f"{name}_G"], out[f"{name}_seed"] = x, idx.astype(np.int32), Gm, np.int64(seed)
                out[f"{name}_margin"] = np.array([m, delta])
                for n in WNAMES:                                                  # shared by the two relu cases of a shape
                    out[f"c{C}n{N}_{n}"] = w[n]
                for n in gh.GRADS:
                    a64 = np.swapaxes(r64[n], 1, 2) if n == "gx" else r64[n]
                    a32 = np.swapaxes(r32[n], 1, 2) if n == "gx" else r32[n]
                    spread = float(np.abs(a32 - a64).max())
                    off = float(np.abs(a32 - ref[n]).max())
                    assert off <= 4 * spread, (name, n, off, spread)
                    out[f"{name}_ref_{n}"], out[f"{name}_f64_{n}"], out[f"{name}_spread_{n}"] = ref[n].copy(), a64, np.float64(spread)
                print(f"{name}: seed {seed}, margin {m:.2e} >= delta {delta:.2e}")
    path = os.path.join(OUT, "g29_ecg_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
