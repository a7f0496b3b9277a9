#!/usr/bin/env python3
"""Golden values and GRADIENTS of the latent head of VRCNet's "train" prefix from the REAL reference, CPU
only.

    python tests/golden/make_golden_vrcnet_train.py

completion/models/vrcnet.py is imported with the stand-ins of make_golden_ecg.py, as make_golden_vrcnet.py imports it.  The
reference's four Linear_ResBlocks are built at the real widths (1024 / 128) and loaded with the seeded weights of
tests/vrcnet_train_host.py `case` (vrcnet_weights.make_state).  Then the reference's OWN LINES run, read from its source file
at generation time and executed here in float32 -- nothing of them is restated in this script:

    vrcnet.py:578-593   o_x, q, o_y, p, the softplus, the four distributions, the two rsample calls, z, the doubled feat_x
    vrcnet.py:605       feat += generator(z)
    vrcnet.py:622-625   the two kl_divergence calls

Two things differ from Model.forward, both forced by torch: feat_x and feat_y enter as SEPARATE tensors, not as feat.chunk(2)
(line 577) -- torch 2.10 refuses the in-place ReLU of posterior_infer1 on a chunk view ("Output 0 of SplitBackward0 is a view
and is being modified inplace"), so the reference's branch does not run as it stands -- and each is a clone of its leaf, because
an in-place operation on a leaf that requires a gradient is refused as well.  Normal.rsample is wrapped so that it applies the
stored noise (loc + eps * scale, its own formula) instead of drawing.

    L = 20 (dl_rec.mean() + dl_g.mean()) + <G, feat>

Stored in g33_vrcnet_train_head.npz: the seed, the inputs, the reference's values (q_mu, q_std, p_mu, p_std, z before the
generator's in-place ReLU, dl_rec, dl_g, global_feat), its gradients of L with respect to both feature leaves and all 24
parameters (KEEP seeded entries of each large one, with their flat indices as `<name>_idx`), the float64 restatement of
tests/vrcnet_train_host.py at the same entries, and per tensor the float32-vs-float64 spread of the restatement.

A gradient is discontinuous at a ReLU kink, so the case is CHOSEN: seeds 0, 1, ... (cap 64) are walked for one whose non-zero
ReLU inputs all keep clear of 4x their float32 spread.  `qualifies` says whether one was found; if none, the seed with the widest
margin is stored.  The script asserts that the reference lies within 4x the spread of the float64 restatement on everything it
stores, and that the file stays under 1 MiB."""
import os
import sys
import textwrap

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_ecg as mge  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrcnet_train_host as host  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FILE = "g33_vrcnet_train_head.npz"
CAP, KEEP = 64, 2048
T = torch.tensor


def choose():
    best = None
    for seed in range(CAP):
        m = host.margins(seed)
        score = min(k / s for k, s in m)
        print(f"seed {seed}: smallest ReLU input over 4x its spread, worst array: {score / 4:.3g}: "
              f"{'qualifies' if score > 4 else 'fails'}", flush=True)
        if score > 4:
            return seed, True
        if best is None or score > best[1]:
            best = (seed, score)
    return best[0], False


def sample(name, size):
    if size <= 2 * KEEP:                                          # the values, the feature gradients and the biases: whole
        return np.arange(size)
    rng = np.random.default_rng(sum(map(ord, name)))
    return np.sort(rng.choice(size, KEEP, replace=False))


def reference(vrc, state, feat_x, feat_y, eps_q, eps_p, G):
    net = torch.nn.Module()
    net.size_z = host.SIZE_Z
    net.posterior_infer1 = vrc.Linear_ResBlock(input_size=host.WIDTH, output_size=host.WIDTH)
    net.posterior_infer2 = vrc.Linear_ResBlock(input_size=host.WIDTH, output_size=2 * host.SIZE_Z)
    net.prior_infer = vrc.Linear_ResBlock(input_size=host.WIDTH, output_size=2 * host.SIZE_Z)
    net.generator = vrc.Linear_ResBlock(input_size=host.SIZE_Z, output_size=host.WIDTH)
    net.load_state_dict({k: T(v) for k, v in state.items()}, strict=True)
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in host.spec()]
    lines = open(vrc.__file__).read().splitlines()
    # a shifted source file must fail here, not generate a wrong fixture: a word of each block's first and last line
    for at, word in ((578, "posterior_infer2"), (593, "feat_x, feat_x"), (605, "generator(z)"), (622, "dl_rec"), (625, "q_distribution")):
        assert word in lines[at - 1], f"{vrc.__file__}:{at} is not the expected line: {lines[at - 1]!r}"
    block = lambda a, b: textwrap.dedent("\n".join(lines[a - 1:b]))
    noise = [T(eps_q), T(eps_p)]
    rsample = torch.distributions.Normal.rsample
    torch.distributions.Normal.rsample = lambda d, *a, **k: d.loc + noise.pop(0) * d.scale
    try:
        leaf_x, leaf_y = T(feat_x).requires_grad_(True), T(feat_y).requires_grad_(True)
        ns = dict(self=net, torch=torch, F=F, feat_x=leaf_x.clone(), feat_y=leaf_y.clone())
        exec(block(578, 593), ns)
        assert not noise
        vals = {n: ns[n].detach().numpy().copy() for n in ("q_mu", "q_std", "p_mu", "p_std", "z")}
        exec(block(605, 605), ns)
        exec(block(622, 625), ns)
    finally:
        torch.distributions.Normal.rsample = rsample
    vals.update(dl_rec=ns["dl_rec"].detach().numpy().copy(), dl_g=ns["dl_g"].detach().numpy().copy(),
                global_feat=ns["feat"].detach().numpy().copy())
    (20 * (ns["dl_rec"].mean() + ns["dl_g"].mean()) + (T(G) * ns["feat"]).sum()).backward()
    grads = {n: p.grad.numpy().copy() for n, p in net.named_parameters()}
    grads.update(feat_x=leaf_x.grad.numpy().copy(), feat_y=leaf_y.grad.numpy().copy())
    return vals, grads


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mge.import_ecg()
    import models.vrcnet as vrc
    assert vrc.__file__.startswith(f"{mge.mg.REF}/completion")
    seed, ok = choose()
    a = host.case(seed)
    state, feat_x, feat_y, eps_q, eps_p, G = a
    rv, rg = reference(vrc, *a)
    v64, g64 = host.head(*a, np.float64)
    v32, g32 = host.head(*a, np.float32)
    out = dict(seed=np.int32(seed), qualifies=np.bool_(ok), feat_x=feat_x, feat_y=feat_y, eps_q=eps_q, eps_p=eps_p)
    worst = 0.0
    for kind, ref, f64, f32 in (("", rv, v64, v32), ("grad_", rg, g64, g32)):
        assert sorted(ref) == sorted(f64), (sorted(ref), sorted(f64))
        for n in ref:
            r_, a64, a32 = ref[n], f64[n], f32[n]
            assert r_.dtype == np.float32 and a32.dtype == np.float32 and a64.dtype == np.float64 and r_.shape == a64.shape, n
            spread = float(np.abs(a32.astype(np.float64) - a64).max())
            err = float(np.abs(r_.astype(np.float64) - a64).max())
            print(f"{kind}{n}: |.| max {np.abs(a64).max():.3g}; float32 restatement vs float64 {spread:.3g}; reference vs float64 "
                  f"{err:.3g} ({err / spread:.2f}x)")
            assert err <= 4 * spread, (kind + n, err, spread)
            worst = max(worst, err / spread)
            at = sample(n, r_.size)
            out[f"spread_{kind}{n}"] = np.float64(spread)
            out[f"ref_{kind}{n}"], out[f"f64_{kind}{n}"] = r_.reshape(-1)[at], a64.reshape(-1)[at]
            if at.size < r_.size:
                out[f"{kind}{n}_idx"] = at.astype(np.int32)
    path = os.path.join(OUT, FILE)
    np.savez_compressed(path, **out)
    print(f"wrote {FILE}: seed {seed} qualifies={ok}, reference within {worst:.2f}x the float32 spread of the float64 restatement, "
          f"{os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
