#!/usr/bin/env python3
"""Golden vectors for the ECG completion network from the REAL reference, CPU only.

    python tests/golden/make_golden_ecg.py

Imports completion/models/ecg.py with the stubs of make_golden.py (`.cuda()` is the identity), the `torch.arange` device patch
of make_golden_dcp.py and torch stand-ins, written below, for the six mm3d_pn2 ops it calls (furthest_point_sample,
gather_points, grouping_operation, three_nn, three_interpolate, ball_query).  Loads the seeded weights of
tests/golden/ecg_weights.py into its Model with strict=True and runs the test-prefix forward in float32 as it stands.

Cases (num_points, num_coarse, num_input), B = 2: (512, 512, 512) -- scale 1, no expansion, the final FPS goes 1024 -> 512 -- and
(1280, 512, 512) -- scale 2: EF_expansion and the final FPS 2048 -> 1280.  Both satisfy the reference's own minimum (>= 500
points for its uniform loss, >= 1024 encoder points).

The reference does not agree with itself across precisions on its discrete decisions (near-ties of the expanded-form k-NN, then
of everything downstream), so no end-to-end tolerance exists.  Stored per case instead: the input; the reference's DECISIONS,
recorded by wrapping its knn, knn_point, furthest_point_sample and three_nn (ecg_host.DECISIONS names them); its feat / out1 /
out2 (float32, outputs subsampled); the float64 forward of the NumPy restatement tests/ecg_host.py WITH THOSE DECISIONS INJECTED;
the float32-vs-float64 spread of the restatement under the same decisions; per feature-space k-NN decision the mask of entries
whose float64 margin exceeds tau = 4 (C + 3) 2^-24 on both sides (`<name>_safe`: any ranking whose distances are accurate to
tau / 2 has the same entry there); once: the state_dict names and shapes of both cases.

The script asserts that the float32 restatement with the reference's decisions reproduces the reference within 4x the spreads."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import ecg_weights  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ecg_host as host  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = {"p512": (512, 512, 512), "p1280": (1280, 512, 512)}
B = 2
KEEP_EVERY = 5


# ---- torch stand-ins for the mm3d_pn2 ops (the CUDA kernels' semantics, float32) ---------------------------------------------
def furthest_point_sample(xyz, npoint):
    Bn, N, _ = xyz.shape
    md = torch.full((Bn, N), 1e10, dtype=xyz.dtype)
    idx = torch.zeros((Bn, npoint), dtype=torch.int64)
    last = torch.zeros(Bn, dtype=torch.int64)
    for j in range(1, npoint):
        q = xyz[torch.arange(Bn), last].unsqueeze(1)
        d = xyz - q
        d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        md = torch.minimum(md, d)
        last = torch.argmax(md, dim=1)                       # first maximum
        idx[:, j] = last
    return idx.int()


def gather_points(features, idx):
    return torch.gather(features, 2, idx.long().unsqueeze(1).expand(-1, features.shape[1], -1))


def grouping_operation(features, idx):
    Bn, C, _ = features.shape
    return gather_points(features, idx.reshape(Bn, -1)).view(Bn, C, *idx.shape[1:])


def _sqdist(a, b):
    d = b.unsqueeze(1) - a.unsqueeze(2)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def three_nn(target, source):
    d2 = _sqdist(target, source)
    idx = torch.argsort(d2, dim=2, stable=True)[..., :3]
    return torch.sqrt(torch.gather(d2, 2, idx)), idx.int()


def three_interpolate(features, idx, weight):
    f = grouping_operation(features, idx)
    w = weight.unsqueeze(1)
    return (w[..., 0] * f[..., 0] + w[..., 1] * f[..., 1]) + w[..., 2] * f[..., 2]


def ball_query(min_radius, max_radius, nsample, xyz, center):
    d2 = _sqdist(center, xyz)
    hit = (d2 == 0) | ((d2 >= min_radius * min_radius) & (d2 < max_radius * max_radius))
    rank = torch.cumsum(hit.long(), dim=2) - 1
    N = xyz.shape[1]
    idx = torch.zeros(center.shape[:2] + (nsample,), dtype=torch.int64)
    ar = torch.arange(N).expand_as(rank)
    for s in range(nsample):
        sel = hit & (rank == s)
        has = sel.any(dim=2)
        pos = torch.where(sel, ar, torch.full_like(ar, N)).min(dim=2).values
        first = idx[..., 0] if s else torch.zeros_like(pos)
        idx[..., s] = torch.where(has, pos, first)
    return idx.int()


def import_ecg():
    mg.import_reference()
    for n in [m for m in sys.modules if m == "models" or m.startswith("models.") or m in ("model_utils", "train_utils")]:
        del sys.modules[n]
    mm3d = types.ModuleType("mm3d_pn2")
    for f in (furthest_point_sample, gather_points, grouping_operation, three_nn, three_interpolate, ball_query):
        setattr(mm3d, f.__name__, f)
    sys.modules["mm3d_pn2"] = mm3d
    _arange = torch.arange
    torch.arange = lambda *a, **k: _arange(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
    sys.path.insert(0, f"{mg.REF}/completion")
    import model_utils
    import models.ecg as ecg
    assert model_utils.__file__.startswith(f"{mg.REF}/completion") and ecg.__file__.startswith(f"{mg.REF}/completion")
    return model_utils, ecg


class Recorder:
    """Wraps the reference's decision functions; records in call order while `on`."""

    def __init__(self, mu, ecg):
        self.rec, self.on = {}, True
        self.count = dict(knn=0, knn_point=0, fps=0, three_nn=0)
        knn, knn_point, fps, tnn, uni = mu.knn, mu.knn_point, mu.furthest_point_sample, mu.three_nn, ecg.get_uniform_loss

        def w_knn(x, k):
            idx = knn(x, k)
            if self.on:
                self.count["knn"] += 1
                self.rec["knn_exp" if x.shape[1] == 256 else f"knn_feat{self.count['knn']}"] = idx.numpy().copy()
            return idx

        def w_knn_point(pk, a, b):
            d, idx = knn_point(pk, a, b)
            if self.on:
                self.count["knn_point"] += 1
                self.rec[f"knn_pt{self.count['knn_point']}"] = idx.numpy().copy()
            return d, idx

        def w_fps(xyz, n):
            idx = fps(xyz, n)
            if self.on:
                self.count["fps"] += 1
                self.rec[f"fps{self.count['fps']}"] = idx.numpy().copy()
            return idx

        def w_fps_out(xyz, n):
            idx = fps(xyz, n)
            self.rec["fps_out"] = idx.numpy().copy()
            return idx

        def w_tnn(t, s):
            d, idx = tnn(t, s)
            if self.on:
                self.count["three_nn"] += 1
                self.rec[f"three_nn{self.count['three_nn']}"] = idx.numpy().copy()
            return d, idx

        def w_uniform(*a, **k):                              # its FPS / knn_point calls are not decisions of the network
            self.on = False
            try:
                return uni(*a, **k)
            finally:
                self.on = True
        mu.knn, mu.knn_point, mu.furthest_point_sample, mu.three_nn = w_knn, w_knn_point, w_fps, w_tnn
        ecg.furthest_point_sample, ecg.get_uniform_loss = w_fps_out, w_uniform

    def reset(self):
        self.rec = {}
        self.count = dict(knn=0, knn_point=0, fps=0, three_nn=0)


def safe_mask(rows, idx):
    """rows[B,N,C] float64, idx[B,N,k]: True where the entry is the float64 ranking's and its squared distance is separated from
    both neighbours in that ranking by more than tau, relatively."""
    C = rows.shape[2]
    tau = 4 * (C + 3) * 2.0 ** -24
    d = host.sqdist_rows(rows, rows)
    order = np.argsort(d, axis=-1, kind="stable")
    k = idx.shape[2]
    ds = np.take_along_axis(d, order[..., :k + 1], axis=-1) if d.shape[2] > k else None
    assert ds is not None
    same = order[..., :k] == idx
    up = ds[..., 1:k + 1] - ds[..., :k] > tau * ds[..., 1:k + 1]
    down = np.ones_like(up)
    down[..., 1:] = up[..., :-1]
    return same & up & down


def main():
    torch.set_num_threads(8)
    mu, ecg = import_ecg()
    recorder = Recorder(mu, ecg)
    out = {}
    rng = np.random.default_rng(26)
    for name, (num_points, num_coarse, num_input) in CASES.items():
        scale = int(np.ceil(num_points / (num_coarse + num_input)))
        net = ecg.Model(ecg_weights.args(num_points), num_coarse=num_coarse, num_input=num_input)
        state = ecg_weights.make_state(num_coarse, scale)
        net.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
        net.eval()
        out[f"{name}_state_keys"] = np.array(list(net.state_dict().keys()))
        out[f"{name}_state_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in net.state_dict().values()])
        x = rng.uniform(-0.5, 0.5, (B, 3, num_input)).astype(np.float32)
        rec = {}
        h1 = net.encoder.register_forward_hook(lambda m, i, o: rec.__setitem__("feat", o.detach().numpy()))
        h2 = net.decoder.register_forward_hook(lambda m, i, o: rec.__setitem__("out1", o[0].detach().transpose(1, 2).contiguous().numpy()))
        recorder.reset()
        with torch.no_grad():
            res = net(torch.tensor(x), prefix="test")
        h1.remove(); h2.remove()
        decisions = dict(recorder.rec)
        want = [n for n in host.DECISIONS if n != "knn_exp" or scale >= 2]
        assert sorted(decisions) == sorted(want), sorted(decisions)
        ref = dict(feat=rec["feat"], out1=rec["out1"], out2=res["result"].numpy())
        assert ref["out1"].shape == (B, num_coarse, 3) and ref["out2"].shape == (B, num_points, 3)
        f32, used = host.model(state, x, num_points, num_coarse, np.float32, decisions)
        feats = {}
        f64, _ = host.model(state, x, num_points, num_coarse, np.float64, decisions, feats)
        assert all(np.array_equal(used[n], decisions[n]) for n in want)
        out[f"{name}_x"] = x
        for n in want:
            out[f"{name}_{n}"] = decisions[n].astype(np.int16 if decisions[n].max() < 32768 else np.int32)
        for n, rows in feats.items():
            m = safe_mask(rows, decisions[n])
            out[f"{name}_{n}_safe"] = np.packbits(m)
            print(f"{name} {n}: C = {rows.shape[2]}, {m.size - m.sum()} of {m.size} entries within tau of a neighbour or not the float64 choice")
        for q in ("feat", "out1", "out2"):
            assert f32[q].dtype == np.float32 and f64[q].dtype == np.float64
            spread = float(np.abs(f32[q].astype(np.float64) - f64[q]).max())
            err = float(np.abs(ref[q].astype(np.float64) - f64[q]).max())
            print(f"{name} {q}: |.| mean {np.abs(f64[q]).mean():.3g} max {np.abs(f64[q]).max():.3g}; float32 restatement vs float64 "
                  f"{spread:.3g}; reference vs float64 {err:.3g}; reference vs float32 restatement "
                  f"{np.abs(ref[q] - f32[q]).max():.3g}")
            assert err <= 4 * spread, (name, q)
            keep = np.arange(0, ref[q].shape[1], KEEP_EVERY) if q != "feat" else np.arange(ref[q].shape[1])
            out[f"{name}_{q}_idx"] = keep.astype(np.int32)
            out[f"{name}_{q}"] = ref[q][:, keep]
            out[f"{name}_{q}_f64"] = f64[q][:, keep]
            out[f"{name}_spread_{q}"] = np.float64(spread)
        assert np.abs(f64["out2"]).max() >= 0.3 and np.abs(f64["out2"]).max() <= 30, name
    np.savez_compressed(f"{OUT}/g26_ecg.npz", **out)
    print("wrote g26_ecg.npz, bytes", os.path.getsize(f"{OUT}/g26_ecg.npz"))


if __name__ == "__main__":
    main()
