#!/usr/bin/env python3
"""Golden vectors for the PCN completion network from the REAL reference, CPU only.

    python tests/golden/make_golden_pcn.py

Imports registration/models/pcn.py with the stubs of make_golden.py (`.cuda()` is the identity), loads the seeded weights of
tests/golden/pcn_weights.py into its Model with strict=True and runs the test-prefix forward in float32 as it stands, with a
forward hook on the encoder for `feat` and on the decoder for `out1`; one "val" forward checks that the prefix runs.  Cases
(num_points / num_coarse): 64/64 (scale 1), 96/24 (scale 4), 2048/1024 (scale 2); the input cloud has N = 100 points, B = 2.
Stored in g25_pcn.npz per case: the input x[B,3,N], the reference's feat / out1 / out2 (float32; the 2048-point case stores
every 7th point of out2 and of out1 (an odd step: both grid columns of scale 2 are kept) to keep the file small -- the index lists are stored), the float64 forward of
the NumPy restatement tests/pcn_host.py under the same weights (NOT of the reference model: the restatement is tied to the
reference by the float32 comparison below), and the float32-vs-float64 spread of each quantity; once: the
state_dict name and shape list, and the gen_grid / gen_1d_grid / gen_grid_up values for ratios 1, 2, 4, 8, 16.

The script asserts that the float32 restatement reproduces the reference within 4x the spreads, and that activations are O(1)
and the pooled feature is not bias-dominated (|feat| mean >= 0.3, |out2| up to >= 0.3)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import pcn_weights  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcn_host as host  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = {"p64c64": (64, 64), "p96c24": (96, 24), "p2048c1024": (2048, 1024)}
N_IN, B = 100, 2
KEEP_EVERY = {"p2048c1024": 7}          # odd: both grid columns of scale 2 are sampled
GRID_RATIOS = (1, 2, 4, 8, 16)


def main():
    torch.set_num_threads(8)
    _, _, _, _, muc = mg.import_reference()
    import models.pcn as pcn
    out = {}
    rng = np.random.default_rng(25)
    for r in GRID_RATIOS:
        out[f"grid_up_{r}"] = muc.gen_grid_up(r, 0.05).numpy()
        out[f"grid_up_default_{r}"] = muc.gen_grid_up(r).numpy()
        out[f"grid_{r}"] = muc.gen_grid(r).numpy()
        out[f"grid_1d_{r}"] = muc.gen_1d_grid(r).numpy()
    for name, (num_points, num_coarse) in CASES.items():
        args = pcn_weights.args(num_points)
        net = pcn.Model(args, num_coarse=num_coarse)
        state = pcn_weights.make_state(num_coarse)
        net.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
        net.eval()
        if name == "p64c64":
            out["state_keys"] = np.array(list(net.state_dict().keys()))
            out["state_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in net.state_dict().values()])
        x = rng.uniform(-0.5, 0.5, (B, 3, N_IN)).astype(np.float32)
        rec = {}
        h1 = net.encoder.register_forward_hook(lambda m, i, o: rec.__setitem__("feat", o.detach().numpy()))
        h2 = net.decoder.register_forward_hook(lambda m, i, o: rec.__setitem__("out1", o[0].detach().transpose(1, 2).contiguous().numpy()))
        with torch.no_grad():
            res = net(torch.tensor(x), prefix="test")
            gt = torch.tensor(rng.uniform(-0.5, 0.5, (B, num_points, 3)).astype(np.float32))
            val = net(torch.tensor(x), gt, prefix="val")
        h1.remove(); h2.remove()
        assert sorted(val) == ["cd_p", "cd_t", "f1", "out1", "out2"]
        ref = dict(feat=rec["feat"], out1=rec["out1"], out2=res["result"].numpy())
        assert ref["out1"].shape == (B, num_coarse, 3) and ref["out2"].shape == (B, num_points, 3)
        assert np.array_equal(val["out2"].numpy(), ref["out2"])
        f32 = host.model(state, x, num_points, num_coarse, np.float32)
        f64 = host.model(state, x, num_points, num_coarse, np.float64)
        step = KEEP_EVERY.get(name, 1)
        out[f"{name}_x"] = x
        for q in ("feat", "out1", "out2"):
            assert f32[q].dtype == np.float32 and f64[q].dtype == np.float64
            spread = float(np.abs(f32[q].astype(np.float64) - f64[q]).max())
            err = float(np.abs(ref[q].astype(np.float64) - f64[q]).max())
            print(f"{name} {q}: |.| mean {np.abs(f64[q]).mean():.3g} max {np.abs(f64[q]).max():.3g}; float32 restatement vs float64 "
                  f"{spread:.3g}; reference vs float64 {err:.3g}; reference vs float32 restatement "
                  f"{np.abs(ref[q] - f32[q]).max():.3g}")
            assert err <= 4 * spread, (name, q)
            keep = np.arange(0, ref[q].shape[1], step) if q != "feat" else np.arange(ref[q].shape[1])
            out[f"{name}_{q}_idx"] = keep.astype(np.int32)
            out[f"{name}_{q}"] = ref[q][:, keep]
            out[f"{name}_{q}_f64"] = f64[q][:, keep]
            out[f"{name}_spread_{q}"] = np.float64(spread)
        assert np.abs(f64["feat"]).mean() >= 0.3 and np.abs(f64["out2"]).max() >= 0.3, name
        assert (f64["feat"] < 0).any() and (f64["feat"] > 0).any()
    np.savez_compressed(f"{OUT}/g25_pcn.npz", **out)
    print("wrote g25_pcn.npz, bytes", os.path.getsize(f"{OUT}/g25_pcn.npz"))


if __name__ == "__main__":
    main()
