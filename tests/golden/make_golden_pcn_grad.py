#!/usr/bin/env python3
"""Golden GRADIENTS of the PCN completion network from the REAL reference, CPU only.

    python tests/golden/make_golden_pcn_grad.py

Imports registration/models/pcn.py with the stubs of make_golden.py, loads the seeded weights of tests/golden/pcn_weights.py
with strict=True and runs float32 autograd on L = <G1, out1> + <G2, out2> with seeded G1, G2 (out1 from a forward hook on the
decoder, out2 from the "test" prefix).  A linear loss keeps Chamfer's own arg-min decisions out of a network fixture.

A gradient is discontinuous where a ReLU input is 0 or two pool candidates are equal, so the input cloud is CHOSEN: for each
case the seeds 0, 1, ... (cap 512) are walked and the first is taken for which, in the float64 forward of the NumPy restatement,
every ReLU input has |pre| >= delta and every pool's runner-up lies at least delta below the maximum, delta = 4x the
float32-vs-float64 spread of that quantity (pcn_grad_host.clear_margins).  No element is ever masked out; if no seed passes, the
script raises.  To keep the walk short a seed whose float64 forward already has a ReLU input or a pool margin below 2e-7 is
skipped without its float32 forward; the script asserts that every delta it does compute is above 2e-7, so no skipped seed
could have qualified.

Cases (B, N, num_points / num_coarse): (1, 33, 32/8) and (2, 65, 64/16).  Stored in g28_pcn_grad.npz per case: x, G1, G2, the
seed, and per parameter tensor a seeded list of at most 2048 entries -- the flat indices, the reference's float32 gradients
there, the float64 restatement's (tests/pcn_grad_host.model_backward), and the float32-vs-float64 spread of the restatement over
the whole tensor (decoder.fc1.weight alone would be 4 MB).  The script asserts that the float32 restatement lies within 4x the
spread of the reference's gradient on every entry of every tensor."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import pcn_weights  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcn_grad_host as ghost  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = {"b1n33p32c8": (1, 33, 32, 8), "b2n65p64c16": (2, 65, 64, 16)}
CAP, KEEP, SCREEN = 512, 2048, 2e-7


def choose(state, B, N, num_points, num_coarse):
    for seed in range(CAP):
        x = np.random.default_rng(seed).uniform(-0.5, 0.5, (B, 3, N)).astype(np.float32)
        k64 = ghost.model_kinks(state, x, num_points, num_coarse, np.float64)
        tops = [np.sort(a, 1) for a in k64[1]]
        if min(float(np.abs(a).min()) for a in k64[0]) < SCREEN or min(float((t[:, -1] - t[:, -2]).min()) for t in tops) < SCREEN:
            continue
        k32 = ghost.model_kinks(state, x, num_points, num_coarse, np.float32)
        deltas = [4 * float(np.abs(a - b).max()) for a, b in zip(k64[0] + k64[1], k32[0] + k32[1])]
        assert min(deltas) > SCREEN, (seed, deltas)
        ok, margin = ghost.clear_margins(k64, k32)
        if ok:
            return seed, x, margin, deltas
    raise RuntimeError(f"no seed below {CAP} keeps B={B} N={N} {num_points}/{num_coarse} clear of its kinks")


def main():
    torch.set_num_threads(8)
    mg.import_reference()
    import models.pcn as pcn
    out = {}
    for name, (B, N, num_points, num_coarse) in CASES.items():
        state = pcn_weights.make_state(num_coarse)
        seed, x, margin, deltas = choose(state, B, N, num_points, num_coarse)
        print(f"{name}: seed {seed}, smallest margin {margin:.3g} deltas, deltas {min(deltas):.3g} .. {max(deltas):.3g}")
        rng = np.random.default_rng(28 + num_coarse)
        G1 = rng.uniform(-1, 1, (B, num_coarse, 3)).astype(np.float32)
        G2 = rng.uniform(-1, 1, (B, num_points, 3)).astype(np.float32)
        net = pcn.Model(pcn_weights.args(num_points), num_coarse=num_coarse)
        net.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
        rec = {}
        hook = net.decoder.register_forward_hook(lambda m, i, o: rec.__setitem__("out1", o[0].transpose(1, 2)))
        out2 = net(torch.tensor(x), prefix="test")["result"]
        hook.remove()
        assert rec["out1"].shape == (B, num_coarse, 3) and out2.shape == (B, num_points, 3) and out2.requires_grad
        ((torch.tensor(G1) * rec["out1"]).sum() + (torch.tensor(G2) * out2).sum()).backward()
        ref = {k: p.grad.numpy() for k, p in net.named_parameters()}
        r64 = ghost.model_backward(state, x, G1, G2, num_points, num_coarse, np.float64)
        r32 = ghost.model_backward(state, x, G1, G2, num_points, num_coarse, np.float32)
        assert np.abs(out2.detach().numpy() - r64["out2"]).max() < 1e-4
        assert list(ref) == list(state) and len(ref) == 20
        out[f"{name}_x"], out[f"{name}_G1"], out[f"{name}_G2"], out[f"{name}_seed"] = x, G1, G2, np.int32(seed)
        pick = np.random.default_rng(2028)
        for k in state:
            g64, g32 = r64["grads"][k], r32["grads"][k]
            assert ref[k].shape == g64.shape == g32.shape and g32.dtype == np.float32
            spread = float(np.abs(g32.astype(np.float64) - g64).max())
            err32 = float(np.abs(g32.astype(np.float64) - ref[k]).max())
            print(f"  {k:22s} |g| up to {np.abs(g64).max():8.3g}  float32 restatement vs float64 {spread:.3g}  vs the reference "
                  f"{err32:.3g}  reference vs float64 {np.abs(ref[k] - g64).max():.3g}")
            assert err32 <= 4 * spread, (name, k, err32, spread)
            idx = np.sort(pick.choice(g64.size, min(KEEP, g64.size), replace=False)).astype(np.int32)
            out[f"{name}_{k}_idx"] = idx
            out[f"{name}_{k}_ref"] = ref[k].reshape(-1)[idx]
            out[f"{name}_{k}_f64"] = g64.reshape(-1)[idx]
            out[f"{name}_{k}_spread"] = np.float64(spread)
    np.savez_compressed(f"{OUT}/g28_pcn_grad.npz", **out)
    print("wrote g28_pcn_grad.npz, bytes", os.path.getsize(f"{OUT}/g28_pcn_grad.npz"))


if __name__ == "__main__":
    main()
