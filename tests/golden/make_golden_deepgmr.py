#!/usr/bin/env python3
"""Golden vectors for the DeepGMR head from the REAL reference, CPU only.

    python tests/golden/make_golden_deepgmr.py

Imports registration/models/deepgmr.py with the stubs of make_golden.py (its `open3d` stub also serves visu_utils; `.cuda()` is
the identity), plus `torch.arange` ignoring device=, because get_edge_features hard-codes the device (deepgmr.py:20-22).  The
model is seeded-random-initialised from tests/golden/deepgmr_weights.py (BatchNorm running statistics randomised too, eval
mode) and run twice: in float32 as it stands, and the same model converted to float64 on the same fp32 inputs -- the spread
between the two is the fixture's own measure of how well-conditioned the random model is, and the tests' tolerances scale
with it.  Stored in g23_deepgmr.npz for B = 2 at N = 64 and N = 256: the clouds, the reference's own k-NN indices and RRI
features, gamma, pi / mu / sigma (the scalar of sigma * eye(3)) and T_12 in both precisions, the state_dict key list."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import deepgmr_weights  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepgmr_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = int(os.environ.get("DEEPGMR_SEED", "2024"))


def run(net, dg, src, tgt, dtype):
    """One test-prefix forward in `dtype`; the fp64 run needs the module's own `torch.eye(3)` / bottom row to follow the dtype."""
    torch.set_default_dtype(dtype)
    try:
        net = net.to(dtype)
        with torch.no_grad():
            T12 = net(src.to(dtype), tgt.to(dtype), prefix="test")
            f1 = dg.get_rri_cluster(src.to(dtype).transpose(1, 2).unsqueeze(-1), net.k).squeeze(-1)
            idx1 = dg.knn(src.to(dtype).transpose(1, 2).contiguous(), net.k + 1)[:, :, 1:]
            idx2 = dg.knn(tgt.to(dtype).transpose(1, 2).contiguous(), net.k + 1)[:, :, 1:]
    finally:
        torch.set_default_dtype(torch.float32)
    f = lambda t: t.detach().cpu().numpy()
    return dict(T12=f(T12), gamma1=f(net.gamma1), gamma2=f(net.gamma2), pi1=f(net.pi1), mu1=f(net.mu1),
                sigma1=f(net.sigma1[:, :, 0, 0]), pi2=f(net.pi2), mu2=f(net.mu2), sigma2=f(net.sigma2[:, :, 0, 0]),
                rri1=f(f1), knn1=f(idx1).astype(np.int32), knn2=f(idx2).astype(np.int32))


def main():
    torch.set_num_threads(8)
    mg.import_reference()
    _arange = torch.arange
    torch.arange = lambda *a, **k: _arange(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
    _Tensor = torch.Tensor
    import models.deepgmr as dg
    dg.np = np                                         # deepgmr.py uses `np` through `from train_utils import *`
    # `torch.Tensor([[[0,0,0,1]]])` (deepgmr.py:141) is always fp32: let it follow the default dtype in the fp64 run
    dg.torch = type("T", (), {"__getattr__": lambda self, n: getattr(torch, n),
                              "Tensor": staticmethod(lambda x: torch.tensor(x, dtype=torch.get_default_dtype()))})()

    net = dg.Model(deepgmr_weights.Args)
    state = {k: torch.tensor(v) for k, v in deepgmr_weights.make_state(SEED).items()}
    missing, unexpected = net.load_state_dict(state, strict=False)
    assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing), (missing, unexpected)
    net.eval()
    out = {"state_keys": np.array(sorted(k for k in net.state_dict() if not k.endswith("num_batches_tracked")))}
    # cloud seed: chosen so that at most 2 % of the (point, j) entries of every cloud have a psi next to the 0 / 2 pi wrap (the
    # precondition under which the phi rule of tests/deepgmr_cases.py is not vacuous; asserted below)
    rng = np.random.default_rng(27)
    spread = 0.0
    for name, (B, N) in {"n64": (2, 64), "n256": (2, 256)}.items():
        pairs = [mg.synth_pair(rng, N, 45) for _ in range(B)]
        src = torch.tensor(np.stack([p[0] for p in pairs]))
        tgt = torch.tensor(np.stack([p[1] for p in pairs]))
        r32 = run(net, dg, src, tgt, torch.float32)
        r64 = run(net, dg, src, tgt, torch.float64)
        net.to(torch.float32)
        out.update({f"{name}_src": src.numpy(), f"{name}_tgt": tgt.numpy(), f"{name}_T_gt": np.stack([p[2] for p in pairs])})
        out.update({f"{name}_{k}_f32": v for k, v in r32.items()})
        out.update({f"{name}_{k}_f64": v for k, v in r64.items() if not k.startswith("knn")})
        assert r32["T12"].dtype == np.float32 and r64["T12"].dtype == np.float64 and r64["gamma1"].dtype == np.float64
        same = float(np.mean([np.array_equal(r32[k], r64[k]) for k in ("knn1", "knn2")]))     # lists, order included
        s = float(np.abs(r32["T12"] - r64["T12"]).max())
        print(name, "T12 spread", s, "gamma spread", float(np.abs(r32["gamma1"] - r64["gamma1"]).max()), "knn lists equal in both precisions", same)
        spread = max(spread, s)
        for cloud in (src, tgt):
            nbr = dg.knn(cloud.transpose(1, 2).contiguous(), net.k + 1)[:, :, 1:].numpy()
            assert cases.rri_yardstick(cloud.numpy(), nbr, net.k)[2].mean() <= cases.MAX_FLAGGED
    out["t12_spread"] = np.float64(spread)
    assert spread < 1e-3, f"seed {SEED}: T_12 fp32-vs-fp64 spread {spread}: Ms is ill-conditioned under these weights"
    np.savez_compressed(f"{OUT}/g23_deepgmr.npz", **out)
    print("wrote g23_deepgmr.npz, t12_spread", spread, "bytes", os.path.getsize(f"{OUT}/g23_deepgmr.npz"))


if __name__ == "__main__":
    main()
