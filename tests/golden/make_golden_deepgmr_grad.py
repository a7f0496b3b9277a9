#!/usr/bin/env python3
"""Golden gradients of one DeepGMR training step from the REAL reference, CPU only.

    python tests/golden/make_golden_deepgmr_grad.py

The reference model of make_golden_deepgmr.py (same stubs, weights seed 2024, cloud rng 27, synth_pair(rng, N, 45)) in train()
mode: forward with prefix "train", loss.backward(), at (B, N) = (2, 64) and (3, 100), in float32 as it stands and converted to
float64 on the same fp32 inputs.  Stored in g2x_deepgmr_grad.npz per case: the inputs and T_gt, the reference's k-NN lists, the
loss in both precisions, the float64 gradient of all 23 parameters, the BatchNorm buffers after the step, the rows the max-pool
picked and, per parameter and per buffer, the fp32-vs-fp64 spread max|g32 - g64| / max|g64| that the tests' tolerances scale with.

The gradients hold 1.5 M numbers per case, more than a committed file may carry.  A parameter of at most FULL elements is stored
whole; of a larger one (five convolution weights) the SAMPLE entries at fixed random positions (`sample_<param>`, flat indices,
shared by the cases) plus its sum and sum of squares over all entries.  The float64 values are stored rounded to float32: 6e-8
relative, two orders below the smallest tolerance they are compared under; the sums stay float64."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import deepgmr_weights  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2024
CASES = {"n64": (2, 64), "n100": (3, 100)}
FULL, SAMPLE = 8192, 4096
MAX_SPREAD = 1e-4


def step(dg, src, tgt, T_gt, dtype):
    """A fresh reference model, one train-mode forward + backward in `dtype`."""
    torch.set_default_dtype(dtype)
    try:
        net = dg.Model(deepgmr_weights.Args)
        state = {k: torch.tensor(v) for k, v in deepgmr_weights.make_state(SEED).items()}
        missing, unexpected = net.load_state_dict(state, strict=False)
        assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing), (missing, unexpected)
        net = net.to(dtype).train()
        pools = []
        net.backbone.encoder.register_forward_hook(lambda m, i, o: pools.append(o.detach().argmax(dim=2).numpy().astype(np.int32)))
        loss = net(src.to(dtype), tgt.to(dtype), T_gt.to(dtype))[0]
        loss.backward()
        idx1 = dg.knn(src.to(dtype).transpose(1, 2).contiguous(), net.k + 1)[:, :, 1:]
        idx2 = dg.knn(tgt.to(dtype).transpose(1, 2).contiguous(), net.k + 1)[:, :, 1:]
    finally:
        torch.set_default_dtype(torch.float32)
    grads = {k: p.grad.detach().numpy() for k, p in net.named_parameters()}
    assert len(grads) == 23 and all(g.dtype == (np.float32 if dtype == torch.float32 else np.float64) for g in grads.values())
    bufs = {k: b.detach().numpy() for k, b in net.named_buffers()}
    return dict(loss=loss.detach().numpy(), grads=grads, bufs=bufs, pools=pools, knn1=idx1.numpy().astype(np.int32),
                knn2=idx2.numpy().astype(np.int32), keys=sorted(net.state_dict()))


def main():
    torch.set_num_threads(8)
    mg.import_reference()
    _arange = torch.arange
    torch.arange = lambda *a, **k: _arange(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
    import models.deepgmr as dg
    dg.np = np
    dg.torch = type("T", (), {"__getattr__": lambda self, n: getattr(torch, n),
                              "Tensor": staticmethod(lambda x: torch.tensor(x, dtype=torch.get_default_dtype()))})()
    pick = np.random.default_rng(9018)
    out, worst = {}, 0.0
    for name, (B, N) in CASES.items():
        rng = np.random.default_rng(27)                     # every case draws from a fresh stream
        pairs = [mg.synth_pair(rng, N, 45) for _ in range(B)]
        src, tgt, T_gt = (torch.tensor(np.stack([p[i] for p in pairs])) for i in range(3))
        r32 = step(dg, src, tgt, T_gt, torch.float32)
        r64 = step(dg, src, tgt, T_gt, torch.float64)
        for k in ("knn1", "knn2"):
            assert np.array_equal(r32[k], r64[k]), f"{name}: {k} differs between the precisions"
        assert all(np.array_equal(a, b) for a, b in zip(r32["pools"], r64["pools"])), f"{name}: max-pool rows differ"
        out.update({f"{name}_src": src.numpy(), f"{name}_tgt": tgt.numpy(), f"{name}_T_gt": T_gt.numpy(), f"{name}_knn1": r64["knn1"],
                    f"{name}_knn2": r64["knn2"], f"{name}_pool1": r64["pools"][0], f"{name}_pool2": r64["pools"][1],
                    f"{name}_loss_f32": r32["loss"], f"{name}_loss_f64": r64["loss"]})
        for k, g64 in r64["grads"].items():
            spread = float(np.abs(r32["grads"][k] - g64).max() / np.abs(g64).max())
            worst = max(worst, spread)
            out[f"{name}_spread_{k}"] = np.float64(spread)
            if g64.size <= FULL:
                out[f"{name}_grad_{k}"] = g64.astype(np.float32)
            else:
                if f"sample_{k}" not in out:
                    out[f"sample_{k}"] = np.sort(pick.choice(g64.size, SAMPLE, replace=False)).astype(np.int32)
                out[f"{name}_grad_{k}"] = g64.reshape(-1)[out[f"sample_{k}"]].astype(np.float32)
                out[f"{name}_gradsum_{k}"] = np.array([g64.sum(), (g64 * g64).sum()], dtype=np.float64)
        for k, b in r64["bufs"].items():
            out[f"{name}_buf_{k}"] = b
            if b.dtype != np.int64:
                out[f"{name}_bufspread_{k}"] = np.float64(np.abs(r32["bufs"][k] - b).max() / np.abs(b).max())
        print(name, "loss", float(r32["loss"]), float(r64["loss"]), "worst relative gradient spread so far", worst)
    out["param_names"] = np.array(sorted(r64["grads"]))
    out["state_keys"] = np.array(r64["keys"])
    out["worst_spread"] = np.float64(worst)
    assert worst < MAX_SPREAD, f"fp32-vs-fp64 gradient spread {worst}: a decision flips between the precisions"
    np.savez_compressed(f"{OUT}/g2x_deepgmr_grad.npz", **out)
    print("wrote g2x_deepgmr_grad.npz, worst spread", worst, "bytes", os.path.getsize(f"{OUT}/g2x_deepgmr_grad.npz"))


if __name__ == "__main__":
    main()
