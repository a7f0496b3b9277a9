#!/usr/bin/env python3
"""Golden GRADIENTS of VRCNet's attention blocks from the REAL reference, CPU only.

    python tests/golden/make_golden_vrcnet_grad.py

(a) completion/models/vrcnet.py's `SA_module` alone (imported with the stand-ins of make_golden_ecg.py) at C in {64, 128, 256,
    512} x k in {10, 16}, N = 40, B = 2, random lists, float32 autograd on L = <G, out>: g30_vrcnet_grad_a<C>.npz, one file per
    width (together they would pass the 1 MiB a committed file may have).
(b) `SKN_Res_unit(64, 64, [10, 20], layers=2)`, N = 40, B = 2: g30_vrcnet_grad_b.npz.

A gradient is discontinuous where a ReLU input is 0, so the input is CHOSEN: the seeds 0, 1, ... (cap 64) are walked and the
first is taken for which, in the float64 forward of the NumPy restatement (tests/vrcnet_grad_host.py), every ReLU input (x, t, pre,
o, the outer y of a branch, the unit's af input) that is not exactly 0 lies further from 0 than 4x the float32-vs-float64 spread
of the restatement's ReLU inputs (the largest over them).  An input that is exactly 0 is exempt: it is what an earlier ReLU
clamped, torch and the kernel agree that the gradient there is 0.  Nothing is ever masked out; if no seed passes, the script
raises.  Weights, inputs, lists and G are functions of the seed (tests/vrcnet_grad_cases.py) and are not stored.

Stored per case: the seed, the lists (a check on the regeneration), the kink spread, and per tensor (every parameter and x) at
most 1024 seeded entries: their flat indices, the reference's float32 gradient there, the float64 restatement's, and the
float32-vs-float64 spread of the restatement over the WHOLE tensor.  The script asserts that the float32 restatement lies within
4x that spread of the reference on every stored entry."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_ecg as mge  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrcnet_grad_cases as gc  # noqa: E402
import vrcnet_grad_host as gh  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CAP = 64
T = torch.tensor


def qualifies(run):
    """run(dtype, kinks) evaluates the forward; -> (smallest non-zero |ReLU input| in float64, the float32-vs-float64 spread)."""
    k64, k32 = [], []
    run(np.float64, k64)
    run(np.float32, k32)
    spread = max(float(np.abs(a32.astype(np.float64) - a64).max()) for (_, a64), (_, a32) in zip(k64, k32))
    return gh.margin(k64), spread


def store(out, key, ref, run):
    """ref: {name: the reference's float32 gradient}; run(dtype) -> {name: the restatement's}."""
    g64, g32 = run(np.float64), run(np.float32)
    assert set(ref) == set(g64)
    worst = 0.0
    for n in sorted(ref):
        r, a64, a32 = ref[n].reshape(-1), g64[n].reshape(-1), g32[n].reshape(-1)
        assert r.dtype == np.float32 and a32.dtype == np.float32 and a64.dtype == np.float64 and r.shape == a64.shape, n
        spread = float(np.abs(a32.astype(np.float64) - a64).max())
        at = gc.sample(n, r.size)
        err = float(np.abs(r[at].astype(np.float64) - a64[at]).max())
        assert np.abs(a32[at].astype(np.float64) - r[at]).max() <= 4 * spread, (key, n)
        assert err <= 4 * spread, (key, n, err, spread)
        worst = max(worst, err / spread if spread > 0 else 0.0)
        out[f"{key}_at_{n}"], out[f"{key}_ref_{n}"] = at.astype(np.int32), r[at]
        out[f"{key}_f64_{n}"], out[f"{key}_spread_{n}"] = a64[at], np.float64(spread)
    print(f"{key}: {len(ref)} tensors, reference within {worst:.2f}x the float32 spread of the float64 restatement")


def save(name, out):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **out)
    print("wrote", name, "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 2 ** 20, name


def reference_grads(net, state, x, idxs, G):
    net.load_state_dict({n: T(v) for n, v in state.items()}, strict=True)
    net.train()
    xt = T(x).requires_grad_(True)
    out = net(xt, idxs) if isinstance(idxs, list) else net([xt, idxs])[0]
    (out * T(G)).sum().backward()
    grads = {n: p.grad.numpy() for n, p in net.named_parameters()}
    return dict(grads, x=xt.grad.numpy())


def part_a(vrc):
    for C in gc.A_C:
        out = {}
        for k in gc.A_K:
            key = f"sa{C}_{k}"
            for seed in range(CAP):
                state, x, idx, G = gc.inputs_a(C, k, seed)
                m, spread = qualifies(lambda dt, kinks: gh.sa_module(state, "", x, idx, False, dt, kinks))
                print(f"{key} seed {seed}: smallest non-zero ReLU input {m:.3g}, spread {spread:.3g}")
                if m > 4 * spread:
                    break
            else:
                raise SystemExit(f"{key}: no seed below {CAP} keeps every ReLU input clear of 0")
            ref = reference_grads(vrc.SA_module(C, C // 16, C // 4, C, 8, k), state, x, T(idx), G)

            def run(dt):
                gx, grads = gh.sa_module(state, "", x, idx, False, dt)[1](G)
                return dict(grads, x=gx)
            out[f"{key}_seed"], out[f"{key}_idx"], out[f"{key}_kink_spread"] = np.int32(seed), idx.astype(np.int16), np.float64(spread)
            store(out, key, ref, run)
        save(gc.file_a(C), out)


def part_b(vrc):
    u, out = gc.UNIT, {}
    for seed in range(CAP):
        state, x, idxs, G = gc.inputs_b(seed)
        m, spread = qualifies(lambda dt, kinks: gh.skn_res_unit(state, "", x, idxs, dt, kinks))
        print(f"unit seed {seed}: smallest non-zero ReLU input {m:.3g}, spread {spread:.3g}")
        if m > 4 * spread:
            break
    else:
        raise SystemExit(f"unit: no seed below {CAP} keeps every ReLU input clear of 0")
    ref = reference_grads(vrc.SKN_Res_unit(u["cin"], u["cout"], list(u["ks"]), u["layers"]), state, x, [T(i) for i in idxs], G)

    def run(dt):
        gx, grads = gh.skn_res_unit(state, "", x, idxs, dt)[1](G)
        return dict(grads, x=gx)
    out["unit_seed"], out["unit_kink_spread"] = np.int32(seed), np.float64(spread)
    for i, idx in enumerate(idxs):
        out[f"unit_idx{i}"] = idx.astype(np.int16)
    store(out, "unit", ref, run)
    save(gc.FILE_B, out)


def main():
    torch.manual_seed(0)
    mge.import_ecg()
    import models.vrcnet as vrc
    assert vrc.__file__.startswith(f"{mge.mg.REF}/completion")
    part_a(vrc)
    part_b(vrc)


if __name__ == "__main__":
    main()
