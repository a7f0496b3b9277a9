#!/usr/bin/env python3
"""Golden vectors for the IDAM head from the REAL reference, CPU only.

    python tests/golden/make_golden_idam.py

Imports registration/models/idam.py with the stubs of make_golden.py plus an empty `h5py` module (idam.py imports it at the
top and never uses it; `.cuda()` is the identity).  The model takes the seeded weights of tests/golden/idam_weights.py
(BatchNorm statistics randomised, eval mode) and runs the test-prefix forward in float32 as it stands; forward hooks collect what
the forward does not keep.  B = 2 (`t.squeeze()` at idam.py:341 breaks B = 1) at N = 96, 192 and 768, i.e. M = 16, 32 and 128
kept points.  Stored in g24_idam.npz per case: the clouds, the reference's k-NN lists, the embeddings of the kept points, both
significance vectors, the kept index lists, per iteration the kept source on entry / rowmax / clamped scores / corr_idx /
normalised weights / R / t, the final T, T_f64 and the case's own spread of R, t and T; once: the state_dict key list and the
spreads over all cases.  (Under random weights the correspondences of the two small cases give a nearly singular covariance: the
float32 and the float64 Kabsch solve of the SAME correspondences and weights then differ by O(1), which the per-case spread
records; the N = 768 case pins the pose to ~2e-4.)

The float64 yardstick is the NumPy restatement tests/idam_host.py (the reference forces float32 at :262-263).  Every iteration
is restated from the REFERENCE's own inputs of that iteration (`idam_host.stepwise`), in float32 and in float64: spread_<q> is
the largest difference between the two over all cases, which is what the tests' tolerances scale with, and T_f64 is the pose
composed of the float64 iterations.

The script asserts the conditions under which those tests are not vacuous, and prints the measured values:
  (a) the gap at the M-th significance place is >= 100x the float32-vs-float64 significance difference, in every cloud;
  (b) at most 2 % of all (iteration, row) entries are flagged (best two distinct float64 scores closer than the score bound
      4 x spread_scores, not both exactly +-20);
  (c) at least one row is tied at the clamp, and at least half of the rows have an unclamped maximum;
and that the reference's kept lists, its corr_idx on unflagged rows and its median masks equal the restatement's in both
precisions."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import idam_weights  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import idam_host as host  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = {"n96": 96, "n192": 192, "n768": 768}
CLOUD_SEED = int(os.environ.get("IDAM_CLOUD_SEED", "32"))
QUANT = ("emb", "sig", "rowmax", "scores", "weights", "R", "t", "T")


def reference_run(net, idam, src, tgt):
    """One test-prefix forward of the reference with hooks on the submodules."""
    rec = {"emb": [], "sig": [], "conv1": [], "conv2": [], "head": []}
    f = lambda t: t.detach().cpu().numpy()
    hooks = [net.emb_nn.register_forward_hook(lambda m, i, o: rec["emb"].append(f(o))),
             net.significance_fc.register_forward_hook(lambda m, i, o: rec["sig"].append(f(o.squeeze(1))))]
    for i in range(net.num_iter):
        hooks.append(net.sim_mat_conv1[i].register_forward_hook(lambda m, i_, o: rec["conv1"].append(f(o.max(-1)[0]))))
        hooks.append(net.sim_mat_conv2[i].register_forward_hook(lambda m, i_, o: rec["conv2"].append(o.squeeze(1).clamp(min=-20, max=20))))
    hooks.append(net.head.register_forward_hook(
        lambda m, i, o: rec["head"].append((np.swapaxes(f(i[0]), 1, 2).copy(), f(i[2].squeeze(1)), f(o[0]), f(o[1])))))
    with torch.no_grad():
        T = net(src, tgt, prefix="test")
        knn_s = idam.knn(src.transpose(1, 2).contiguous(), k=12)
        knn_t = idam.knn(tgt.transpose(1, 2).contiguous(), k=12)
    for h in hooks:
        h.remove()
    M = src.shape[1] // 6
    out = dict(T=f(T), knn_src=f(knn_s).astype(np.int32), knn_tgt=f(knn_t).astype(np.int32))
    emb_t, emb_s = (np.swapaxes(e, 1, 2) for e in rec["emb"])             # the forward embeds tgt first; rows [B,N,E]
    sig_s, sig_t = rec["sig"]
    out.update(sig_src=sig_s, sig_tgt=sig_t)
    out["src_idx"] = f(torch.tensor(sig_s).topk(k=M, dim=-1)[1]).astype(np.int32)
    out["tgt_idx"] = f(torch.tensor(sig_t).topk(k=M, dim=-1)[1]).astype(np.int32)
    bi = np.arange(len(sig_s))[:, None]
    out["es"], out["et"] = emb_s[bi, out["src_idx"]].copy(), emb_t[bi, out["tgt_idx"]].copy()
    for i in range(net.num_iter):
        out[f"rowmax{i}"] = np.swapaxes(rec["conv1"][i], 1, 2).copy()     # [B,M,32]
        out[f"scores{i}"] = f(rec["conv2"][i])
        out[f"corr_idx{i}"] = f(rec["conv2"][i].max(-1)[1]).astype(np.int32)
        out[f"src_at{i}"], out[f"weights{i}"], out[f"R{i}"], out[f"t{i}"] = rec["head"][i]
    return out


def restated(state, src, tgt, ref, dtype):
    """The restatement on the reference's inputs: embedding and significance from the clouds and the reference's k-NN lists, each
    iteration from the reference's kept points, embeddings and source on entry."""
    B, N, _ = src.shape
    e_s, e_t = host.embed(state, src, ref["knn_src"], dtype), host.embed(state, tgt, ref["knn_tgt"], dtype)
    g_s, g_t = host.significance(state, e_s, dtype), host.significance(state, e_t, dtype)
    i_s, i_t = host.keep(g_s, N // 6), host.keep(g_t, N // 6)
    bi = np.arange(B)[:, None]
    its, T = host.stepwise(state, [ref[f"src_at{i}"] for i in range(idam_weights.NUM_ITERS)], tgt[bi, ref["tgt_idx"]],
                           ref["es"], ref["et"], dtype)
    q = dict(emb=np.concatenate([e_s[bi, ref["src_idx"]], e_t[bi, ref["tgt_idx"]]]), sig=np.concatenate([g_s, g_t]), T=T)
    for n in ("rowmax", "scores", "weights", "R", "t"):
        q[n] = np.stack([it[n] for it in its])
    return dict(sig_src=g_s, sig_tgt=g_t, src_idx=i_s, tgt_idx=i_t, iters=its, T=T), q


def main():
    torch.set_num_threads(8)
    mg.import_reference()
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    import models.idam as idam
    net = idam.Model(idam_weights.Args)
    state = idam_weights.make_state()
    missing, unexpected = net.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing), (missing, unexpected)
    net.eval()
    out = {"state_keys": np.array(sorted(k for k in net.state_dict() if not k.endswith("num_batches_tracked")))}
    rng = np.random.default_rng(CLOUD_SEED)
    spread = {n: 0.0 for n in QUANT}
    runs = {}
    for name, N in CASES.items():
        pairs = [mg.synth_pair(rng, N, 45) for _ in range(2)]
        src, tgt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        ref = reference_run(net, idam, torch.tensor(src), torch.tensor(tgt))
        r32, q32 = restated(state, src, tgt, ref, np.float32)
        r64, q64 = restated(state, src, tgt, ref, np.float64)
        assert q32["T"].dtype == np.float32 and q64["scores"].dtype == np.float64
        for n in QUANT:
            spread[n] = max(spread[n], float(np.abs(q32[n].astype(np.float64) - q64[n]).max()))
        out.update({f"{name}_src": src, f"{name}_tgt": tgt, f"{name}_T_gt": np.stack([p[2] for p in pairs])})
        out.update({f"{name}_{k}": v for k, v in ref.items()})
        out[f"{name}_T_f64"] = r64["T"]
        for n in ("R", "t", "T"):          # the pose is only as well pinned as the covariance of THIS case's correspondences is conditioned
            out[f"{name}_spread_{n}"] = np.float64(np.abs(q32[n].astype(np.float64) - q64[n]).max())
        runs[name] = (ref, r32, r64)
        print(f"{name}: reference T vs float64 restatement composed of its own iterations {np.abs(ref['T'] - r64['T']).max():.3g}; "
              f"float32-vs-float64 here: R {np.abs(q32['R'] - q64['R']).max():.3g}, T {np.abs(q32['T'] - q64['T']).max():.3g}")
    print("float32-vs-float64 spread of the restatement, each iteration from the reference's inputs:",
          {k: f"{v:.3g}" for k, v in spread.items()})
    bound = 4 * spread["scores"]
    n_rows = n_flag = n_tied = n_unclamped = 0
    for name, (ref, r32, r64) in runs.items():
        M = CASES[name] // 6
        for c in ("src", "tgt"):                                           # (a)
            s64, s32 = r64[f"sig_{c}"], r32[f"sig_{c}"]
            srt = -np.sort(-s64, axis=-1)
            gap = float((srt[:, M - 1] - srt[:, M]).min())
            err = float(np.abs(s32.astype(np.float64) - s64).max())
            print(f"{name} {c}: significance spans {s64.min():.3g}..{s64.max():.3g}, gap at place M {gap:.3g}, f32-f64 {err:.3g}, "
                  f"ratio {gap / err:.0f}")
            assert gap >= 100 * err, f"{name} {c}: condition (a) fails"
            print(f"{name} {c}: kept list, order included: reference == float32 restatement {np.array_equal(ref[f'{c}_idx'], r32[f'{c}_idx'])}, "
                  f"== float64 {np.array_equal(ref[f'{c}_idx'], r64[f'{c}_idx'])}")
            assert all(np.array_equal(np.sort(ref[f"{c}_idx"], -1), np.sort(r[f"{c}_idx"], -1)) for r in (r32, r64))
        for i, (it, it32) in enumerate(zip(r64["iters"], r32["iters"])):
            fl = host.flagged_rows(it["scores"], bound)
            top = it["scores"].max(-1)
            tied = (np.abs(top) == 20) & ((it["scores"] == top[..., None]).sum(-1) >= 2)
            masks = np.array_equal(ref[f"weights{i}"] > 0, it["weights"] > 0) and np.array_equal(it32["weights"] > 0, it["weights"] > 0)
            print(f"{name} iteration {i}: flagged {int(fl.sum())}/{fl.size}, tied at the clamp {int(tied.sum())}, unclamped maximum "
                  f"{int((np.abs(top) < 20).sum())}, corr_idx reference == float64 on all rows "
                  f"{np.array_equal(ref[f'corr_idx{i}'], it['corr_idx'])}, median masks equal {masks}")
            assert np.array_equal(ref[f"corr_idx{i}"][~fl], it["corr_idx"][~fl])
            assert np.array_equal(it32["corr_idx"][~fl], it["corr_idx"][~fl]) and masks
            n_rows += fl.size; n_flag += int(fl.sum()); n_tied += int(tied.sum()); n_unclamped += int((np.abs(top) < 20).sum())
    print(f"(b) flagged {n_flag}/{n_rows} = {n_flag / n_rows:.4f}; (c) tied at the clamp {n_tied}, unclamped maximum "
          f"{n_unclamped}/{n_rows} = {n_unclamped / n_rows:.3f}")
    assert n_flag <= 0.02 * n_rows, "condition (b) fails"
    assert n_tied >= 1 and n_unclamped >= 0.5 * n_rows, "condition (c) fails"
    for n in QUANT:
        out[f"spread_{n}"] = np.float64(spread[n])
    np.savez_compressed(f"{OUT}/g24_idam.npz", **out)
    print("wrote g24_idam.npz, bytes", os.path.getsize(f"{OUT}/g24_idam.npz"))


if __name__ == "__main__":
    main()
