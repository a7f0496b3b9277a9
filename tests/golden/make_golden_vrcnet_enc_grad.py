#!/usr/bin/env python3
"""Golden GRADIENTS of VRCNet's encoder hierarchy from the REAL reference, CPU only.

    python tests/golden/make_golden_vrcnet_enc_grad.py

completion/models/vrcnet.py's `SA_SKN_Res_encoder` (imported with the stand-ins of make_golden_ecg.py) in the case of the encoder
golden of tests/vrcnet_cases.py -- pts_num = ENC_PTS, k = ENC_K, pk = ENC_PK, the seeded weights of encoder_state() -- in eval()
(dropout is the identity), float32 autograd on L = <G, out>, B = 2.  The input carries no gradient here: the stand-in three_nn is
differentiable where the reference's CUDA op is not, so the reference's own input gradient cannot be had on the CPU; the parameters'
gradients are what is stored.

A gradient is discontinuous at every ReLU kink, at every tie of a maximum and at every change of a discrete decision, so the input
is CHOSEN: the seeds 0, 1, ... (cap 64) are walked and the first is taken for which, in the float64 restatement
(tests/vrcnet_enc_grad_host.py),
  * every ReLU input that is not exactly 0 lies further from 0 than 4x the float32-vs-float64 spread of the restatement's ReLU
    inputs (section 9.14's rule);
  * every pooled maximum, and every maximum over the points behind conv5, leads its runner-up by more than the same margin; an
    exact tie at 0 is exempt (section 9.13: the candidates are what a ReLU clamped, and its mask sends no gradient either way);
  * every discrete decision is safe: each k-NN list passes make_golden_vrcnet.safe_mask (section 9.11) on ALL its entries, each
    knn_pt and three_nn list keeps its distances further apart than 4x their float32-vs-float64 spread, and each arg-max step of
    the furthest-point samples leads by as much (the margins of make_golden_ecg_grad.py);
and for which the reference, run as it stands, takes exactly those decisions.  Nothing is masked out.  If no seed qualifies at B = 2
the walk is repeated at B = 1; if none does there either, the narrower fixture is stored: the reference's edge_preserve_sampling
followed by three_nn_upsampling + three_interpolate back onto the points, 128 -> 64 -> 128 points, with the feature gradient.

Stored (g31_vrcnet_enc_grad.npz): `kind` (encoder_b2, encoder_b1 or pool_upsample), the seed, the decisions, and per tensor at most
KEEP seeded entries: their flat indices, the reference's float32 gradient there, the float64 restatement's, and the
float32-vs-float64 spread of the restatement over the whole tensor.  The inputs are functions of the seed
(tests/vrcnet_enc_grad_cases.py) and are not stored.  The script asserts that the float32 restatement lies within 4x that spread of
the reference on every stored entry."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_ecg as mge  # noqa: E402
import make_golden_ecg_grad as megg  # noqa: E402
import make_golden_vrcnet as mgv  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import edge_pool_host as ep  # noqa: E402
import vrcnet_cases as cases  # noqa: E402
import vrcnet_enc_grad_cases as ec  # noqa: E402
import vrcnet_enc_grad_host as egh  # noqa: E402
import vrcnet_grad_host as gh  # noqa: E402
import vrcnet_host as host  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CAP = 64
T = torch.tensor


def decisions_safe(x, dec):
    """Every decision of the encoder on input x[B,3,N], by the rules of the module docstring.  -> (bool, the first that fails)."""
    pts = [np.ascontiguousarray(np.swapaxes(x, 1, 2)).astype(np.float64)]
    for l in (1, 2, 3):
        pts.append(np.take_along_axis(pts[-1], dec[f"fps{l}"][:, :, None], axis=1))
    for l in (1, 2, 3, 4):
        for i in range(len(cases.ENC_K)):
            p, idx = pts[l - 1], dec[f"knn{l}_{i}"]
            if p.shape[1] > idx.shape[2]:
                ok = mgv.safe_mask(p, idx, 0.0).all()                              # the coordinates are the input's own floats
            else:                                                                  # the list holds the whole level: its order alone
                m, d = megg._list_margin(p, p, p.shape[1] - 1)
                ok = m >= d and np.array_equal(host.nearest(p, p, idx.shape[2]), idx)
            if not ok:
                return False, f"knn{l}_{i}"
    for l in (1, 2, 3):
        for name, (m, d) in ((f"knn_pt{l}", megg._list_margin(pts[l], pts[l - 1], min(cases.ENC_PK, pts[l - 1].shape[1]))),
                             (f"three_nn{l}", megg._list_margin(pts[3 - l], pts[4 - l], 3)),
                             (f"fps{l}", megg._fps_margin(pts[l - 1], dec[f"fps{l}"]))):
            if m < d:
                return False, name
    return True, ""


def kinks_clear(state, x, dec):
    """-> (ok, margin, spread, why) for the ReLU inputs and the maxima of the float64 restatement."""
    k64, k32, t64, t32 = [], [], [], []
    run = lambda dt, k, t: egh.encoder(state, x, dec, cases.ENC_K, cases.ENC_PK, cases.ENC_PTS, dt, "", k, t)
    run(np.float64, k64, t64)
    m = gh.margin(k64)
    run(np.float32, k32, t32)
    spread = max(float(np.abs(a32.astype(np.float64) - a64).max()) for (_, a64), (_, a32) in zip(k64, k32))
    if m <= 4 * spread:
        return False, m, spread, "a ReLU input"
    for name, gap in t64:
        if name.endswith("conv5"):
            live = gap                                                             # conv5 carries a bias: no clamped candidates
        else:
            # an exact tie at 0: every tied candidate is a clamped ReLU output (tie_is_at_zero asserts it)
            live = np.where(gap == 0, np.inf, gap)
        if float(live.min()) <= 4 * spread:
            return False, m, spread, name
    return True, m, spread, ""


def tie_is_at_zero(state, x, dec):
    """The exemption's premise, asserted: wherever a pooled gap is exactly 0 the tied maximum is exactly 0."""
    tops, kinks = [], []
    egh.encoder(state, x, dec, cases.ENC_K, cases.ENC_PK, cases.ENC_PTS, np.float64, "", kinks, tops)
    x_of = {n: a for n, a in kinks}
    for name, gap in tops:
        if name.endswith("conv5"):
            continue
        level = int(name[-1])
        rows = np.ascontiguousarray(np.swapaxes(np.maximum(x_of[f"x{level}"][:, :, 0], 0), 1, 2))
        pooled = ep.forward(rows, dec[f"fps{level}"], dec[f"knn_pt{level}"])[0][:, :, rows.shape[2]:]
        if (pooled[gap == 0] != 0).any():
            return False
    return True


def store(out, ref, g64, g32, keep):
    worst = 0.0
    for n in sorted(ref):
        r, a64, a32 = ref[n].reshape(-1), g64[n].reshape(-1), g32[n].reshape(-1)
        assert r.dtype == np.float32 and a32.dtype == np.float32 and a64.dtype == np.float64 and r.shape == a64.shape, n
        spread = float(np.abs(a32.astype(np.float64) - a64).max())
        at = ec.sample(n, r.size, keep)
        err = float(np.abs(r[at].astype(np.float64) - a64[at]).max())
        assert np.abs(a32[at].astype(np.float64) - r[at]).max() <= 4 * spread, n
        assert err <= 4 * spread, (n, err, spread)
        worst = max(worst, err / spread if spread > 0 else 0.0)
        out[f"at_{n}"], out[f"ref_{n}"], out[f"f64_{n}"], out[f"spread_{n}"] = at.astype(np.int32), r[at], a64[at], np.float64(spread)
    print(f"{len(ref)} tensors, reference within {worst:.2f}x the float32 spread of the float64 restatement")


def whole_encoder(vrc, recorder):
    state = cases.encoder_state()
    net = mgv.load(vrc.SA_SKN_Res_encoder(pts_num=list(cases.ENC_PTS), k=list(cases.ENC_K), pk=cases.ENC_PK), state)
    names = egh.decision_names(cases.ENC_K)
    for B in (2, 1):
        for seed in range(CAP):
            x, G = ec.inputs_encoder(B, seed)
            d = host.eh._Decisions(None)
            host.encoder(state, x, d, cases.ENC_K, cases.ENC_PK, cases.ENC_PTS, np.float64, prefix="")
            dec = {n: d.used[n] for n in names}
            ok, why = decisions_safe(x, dec)
            if ok:
                ok, m, spread, why = kinks_clear(state, x, dec)
                why = f"{why} (smallest non-zero ReLU input {m:.3g}, spread {spread:.3g})"
            print(f"encoder B={B} seed {seed}: {'qualifies' if ok else 'fails at ' + why}", flush=True)
            if not ok:
                continue
            assert tie_is_at_zero(state, x, dec)
            recorder.reset(len(cases.ENC_K))
            net.zero_grad()
            y = net(T(x))
            if sorted(recorder.rec) != sorted(names) or any(not np.array_equal(recorder.rec[n], dec[n]) for n in names):
                print("  the reference's float32 ranking decided otherwise")
                continue
            (y * T(G)).sum().backward()
            ref = {n: p.grad.numpy() for n, p in net.named_parameters()}
            run = lambda dt: egh.encoder(state, x, dec, cases.ENC_K, cases.ENC_PK, cases.ENC_PTS, dt, "")[1](G)[1]
            out = dict(kind=np.array(f"encoder_b{B}"), seed=np.int32(seed), kink_spread=np.float64(spread))
            for n in names:
                out[f"dec_{n}"] = dec[n].astype(np.int16)
            store(out, ref, run(np.float64), run(np.float32), ec.KEEP_ENCODER)
            return out
    return None


def pool_upsample(mu):
    """The narrower fixture: edge_preserve_sampling then three_nn_upsampling + three_interpolate, 128 -> 64 -> 128 points."""
    N, S, C, pk = ec.NARROW["N"], ec.NARROW["S"], ec.NARROW["C"], ec.NARROW["pk"]
    for seed in range(CAP):
        feat, pts, G = ec.inputs_narrow(seed)
        p64 = pts.astype(np.float64)
        ft, pt = T(feat).requires_grad_(True), T(pts)
        net, p_idx, pn_idx, centres = mu.edge_preserve_sampling(ft, pt, S, pk)
        idx, weight = mu.three_nn_upsampling(pt, centres)
        dec = dict(fps1=p_idx.numpy().astype(np.int64), knn_pt1=pn_idx.numpy().astype(np.int64), three_nn1=idx.numpy().astype(np.int64))
        c64 = np.take_along_axis(p64, dec["fps1"][:, :, None], axis=1)
        pairs = [megg._list_margin(c64, p64, pk), megg._list_margin(p64, c64, 3), megg._fps_margin(p64, dec["fps1"])]
        rows = np.ascontiguousarray(np.swapaxes(feat, 1, 2)).astype(np.float64)
        nb = np.stack([rows[b, dec["knn_pt1"][b]] for b in range(rows.shape[0])])
        gap = float(egh._gap(nb, 2).min())
        # the features are the input's own floats (spread 0): any positive lead is safe
        ok = all(m >= d for m, d in pairs) and gap > 0
        ok = ok and np.array_equal(host.nearest(c64, p64, pk), dec["knn_pt1"]) and np.array_equal(host.nearest(p64, c64, 3), dec["three_nn1"])
        print(f"pool + upsample seed {seed}: {'qualifies' if ok else 'fails'}", flush=True)
        if not ok:
            continue
        y = mge.three_interpolate(net, idx, weight.detach())             # the stand-in the reference's unpooling calls
        (y * T(G)).sum().backward()

        def run(dt):
            x = np.asarray(feat, dtype=dt)[:, :, None, :]
            f, pbw = egh._pool(x, dec["fps1"], dec["knn_pt1"], None, "")
            _, ubw = egh._upsample(f, pts.astype(dt), np.take_along_axis(pts.astype(dt), dec["fps1"][:, :, None], axis=1), dec["three_nn1"])
            return dict(feat=pbw(ubw(np.asarray(G, dtype=dt)[:, :, None, :]))[:, :, 0])
        out = dict(kind=np.array("pool_upsample"), seed=np.int32(seed))
        for n, v in dec.items():
            out[f"dec_{n}"] = v.astype(np.int16)
        store(out, dict(feat=ft.grad.numpy()), run(np.float64), run(np.float32), ec.KEEP)
        return out
    raise SystemExit(f"no seed below {CAP} qualifies, not even for the pooling alone")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mu, _ = mge.import_ecg()
    import models.vrcnet as vrc
    assert vrc.__file__.startswith(f"{mge.mg.REF}/completion")
    out = whole_encoder(vrc, mgv.Recorder(mu, vrc)) or pool_upsample(mu)
    path = os.path.join(OUT, ec.FILE)
    np.savez_compressed(path, **out)
    print("wrote", ec.FILE, "kind", str(out["kind"]), "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
