"""Shared by tests/test_gpu_ef_expand*.py and scripts/perf_ef_expand.py: the shapes of the op sweep, the case generator and the torch
composition that the fused node (_EFExpandFunction) is measured against."""
import numpy as np

import ef_expand_host as host

# (C, O, r, k, N, B): the product of (C,O) in {(256,64), (64,256), (64,64)}, r in {1,2,3,8}, k in {1,4,8}, N in {1,5,63,64,65,130},
# B in {1,3}, thinned so that every value of every parameter, every O with every N on both sides of the 16-point tile and k > N occur
SWEEP = [(256, 64, 2, 4, 130, 3), (256, 64, 1, 1, 1, 1), (256, 64, 3, 8, 5, 1), (256, 64, 8, 4, 63, 1), (256, 64, 2, 8, 64, 3),
         (256, 64, 1, 4, 65, 1), (64, 256, 1, 4, 65, 1), (64, 256, 2, 1, 63, 1), (64, 256, 3, 4, 5, 3), (64, 256, 8, 8, 1, 1),
         (64, 256, 2, 8, 130, 1), (64, 256, 1, 1, 64, 1), (64, 64, 2, 4, 64, 1), (64, 64, 3, 1, 130, 3), (64, 64, 8, 8, 5, 1),
         (64, 64, 1, 8, 63, 3), (64, 64, 2, 4, 1, 1), (64, 64, 3, 4, 65, 1)]


def make_case(C, O, r, k, N, B, seed=0):
    """float32 operands of the op: proj from a random cloud of features through random convolutions (so that U, V, P, Q have the
    scale and the sign pattern they have in the block), lists with the point itself first, and a gradient."""
    rng = np.random.default_rng([seed, C, O, r, k, N, B])
    s = lambda *shape: (rng.standard_normal(shape) / np.sqrt(shape[-1])).astype(np.float32)
    x = rng.standard_normal((B, N, C)).astype(np.float32)
    W1, b1, W2, b2 = s(O, 2 * C), s(O), s(O * r, O + 2 * C), s(O * r)
    proj, W2a = host.projections(x, W1, b1, W2, b2, np.float32)
    idx = rng.integers(0, N, size=(B, N, k)).astype(np.int32)
    idx[:, :, 0] = np.arange(N)
    return dict(proj=proj, idx=idx, W2a=W2a, W3=s(O, O), b3=s(O), g=rng.standard_normal((B, N * r, O)).astype(np.float32), r=r,
                x=x, W1=W1, b1=b1, W2=W2, b2=b2)


def composed_rows(net, rows, idx):
    """EF_expansion.forward_rows rewritten for autograd with the pieces ECG trains with: _RowGather for the neighbours,
    _LinearRowsFunction for the three convolutions over every edge, torch.max over the slots.  The yardstick of the node's
    memory and time."""
    import torch
    from houv_amd.model_utils_completion import _LinearRowsFunction, _RowGather
    B, N, C = rows.shape
    k, O, r = idx.shape[2], net.output_size, net.step_ratio
    nb = _RowGather.apply(rows, idx).permute(0, 2, 1, 3)                          # (B,k,N,C)
    edge = torch.cat((rows.unsqueeze(1).expand_as(nb), nb), dim=3)
    h1 = _LinearRowsFunction.apply(edge.reshape(-1, 2 * C), net.conv1.matrix(), net.conv1.bias, False)
    cat = torch.relu(torch.cat((h1.view(B, k, N, O), edge), dim=3))
    e = _LinearRowsFunction.apply(cat.reshape(-1, O + 2 * C), net.conv2.matrix(), net.conv2.bias, True)
    e = _LinearRowsFunction.apply(e.view(-1, O), net.conv3.matrix(), net.conv3.bias, False)
    return e.view(B, k, N * r, O).max(dim=1).values


# ---- the reference fixture (tests/golden/make_golden_ef_expand_grad.py) ----
GRAD_FILES = {"a": "g32_ef_expand_grad_a.npz", "b": "g32_ef_expand_grad_b.npz"}
GRAD_CFG = {"a": dict(C=256, O=64, r=2, k=4), "b": dict(C=64, O=256, r=2, k=4)}     # VRCNet's expansion1 and expansion2
GRAD_N, GRAD_B, GRAD_KEEP = 128, 2, 1024
PARAMS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias")


def grad_case(name, seed):
    """The seeded case of one configuration: x[B,N,C], the lists (each point's k nearest points in feature space, itself first,
    distinct), nn.Conv2d-shaped weights as [out, in] matrices and the output's gradient G.  float32."""
    c = GRAD_CFG[name]
    C, O, r, k = c["C"], c["O"], c["r"], c["k"]
    rng = np.random.default_rng([32, ord(name), seed])
    x = rng.standard_normal((GRAD_B, GRAD_N, C)).astype(np.float32)
    d = ((x[:, :, None, :].astype(np.float64) - x[:, None, :, :]) ** 2).sum(-1)
    d[:, np.arange(GRAD_N), np.arange(GRAD_N)] = -1.0
    idx = np.argsort(d, axis=2, kind="stable")[:, :, :k].astype(np.int32)
    u = lambda n_out, n_in: (rng.uniform(-1, 1, (n_out, n_in)) / np.sqrt(n_in)).astype(np.float32)
    w = {"conv1.weight": u(O, 2 * C), "conv1.bias": u(1, O)[0], "conv2.weight": u(O * r, O + 2 * C), "conv2.bias": u(1, O * r)[0],
         "conv3.weight": u(O, O), "conv3.bias": u(1, O)[0]}
    G = rng.standard_normal((GRAD_B, GRAD_N * r, O)).astype(np.float32)
    return x, idx, w, G, r


def sample(name, size, keep=GRAD_KEEP):
    """At most `keep` distinct flat indices into a tensor of `size` elements, seeded by the tensor's name."""
    if size <= keep:
        return np.arange(size)
    return np.sort(np.random.default_rng([7] + [ord(ch) for ch in name]).choice(size, keep, replace=False))
