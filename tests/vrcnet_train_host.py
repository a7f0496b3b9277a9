"""NumPy restatement of the latent head of VRCNet's "train" prefix (completion/models/vrcnet.py:577-605 and :622-625; DESIGN.md
section 9.17), forward and backward, parametrised by dtype: the four Linear_ResBlocks, the two softplus, the two reparametrised
draws with the noise given, relu(feat_x) doubled plus the generator's output, and the two KL terms.  The reference's in-place
ReLUs are restated as the values and gradients they denote: posterior_infer1 and prior_infer see relu(feat_x) and relu(feat_y),
and so does everything after them.

    L = 20 (mean dl_rec + mean dl_g) + <G, global_feat>

`head` returns the values and the gradients of L with respect to both feature leaves and the 24 parameters.  float32 products
are summed the way vrcnet_host.linear_resblock sums them; float64 is the yardstick."""
import numpy as np

import vrcnet_host as vh

BLOCKS = ("posterior_infer1", "posterior_infer2", "prior_infer", "generator")
VALUES = ("q_mu", "q_std", "p_mu", "p_std", "z", "dl_rec", "dl_g", "global_feat")
SIZE_Z, WIDTH = 128, 1024


def spec(size_z=SIZE_Z, width=WIDTH):
    """(name, shape) of the 24 parameters, in the reference's state_dict order."""
    out = []
    for blk, (n_in, n_out) in zip(BLOCKS, ((width, width), (width, 2 * size_z), (width, 2 * size_z), (size_z, width))):
        for layer, (o, i) in (("conv1", (n_in, n_in)), ("conv2", (n_out, n_in)), ("conv_res", (n_out, n_in))):
            out += [(f"{blk}.{layer}.weight", (o, i)), (f"{blk}.{layer}.bias", (o,))]
    return out


def case(seed, B=2):
    """(state, feat_x, feat_y, eps_q, eps_p, G) of the stored fixture: the 24 parameters from vrcnet_weights.make_state (its
    gains, seed SEED + 17: one set of weights for every case seed), features, noise and G standard normal from `seed`."""
    from vrcnet_cases import vrcnet_weights as W
    state = W.make_state(spec(), W.SEED + 17)
    rng = np.random.default_rng(1700 + seed)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    return state, n(B, WIDTH), n(B, WIDTH), n(B, SIZE_Z), n(B, SIZE_Z), n(2 * B, WIDTH)


def margins(seed):
    """Per array that enters a ReLU past the leaves: (its smallest non-zero |element| in float64, its float32-vs-float64
    spread).  A gradient is continuous across the float32 roundings when every first exceeds 4x its second."""
    a = case(seed)
    r64, r32 = [], []
    head(*a, np.float64, relu_inputs=r64)
    head(*a, np.float32, relu_inputs=r32)
    return [(float(np.abs(t[t != 0]).min()), float(np.abs(u.astype(np.float64) - t).max())) for t, u in zip(r64, r32)]


def _block(state, prefix, feature, dtype):
    W = lambda n: vh._wb(state, prefix, n, dtype)
    lin = lambda n, t: vh.rows_times(t, W(n)[0]) + W(n)[1]
    r = vh.relu(feature)
    a = lin("conv1", r)
    ra = vh.relu(a)
    return lin("conv2", ra) + lin("conv_res", r), (prefix, feature, r, a, ra)


def _mm(a, b):
    """a[m,k] . b[k,n] with vrcnet_host's sums (float32: k ascending, the same on every host)."""
    return vh.rows_times(np.ascontiguousarray(a), np.ascontiguousarray(b.T))


def _block_backward(state, cache, gy, dtype, grads):
    prefix, feature, r, a, ra = cache
    W1, W2, Wr = (vh._wb(state, prefix, n, dtype)[0] for n in ("conv1", "conv2", "conv_res"))
    g_a = _mm(gy, W2) * (a > 0)
    grads[prefix + "conv2.weight"], grads[prefix + "conv2.bias"] = _mm(gy.T, ra), gy.sum(0)
    grads[prefix + "conv_res.weight"], grads[prefix + "conv_res.bias"] = _mm(gy.T, r), gy.sum(0)
    grads[prefix + "conv1.weight"], grads[prefix + "conv1.bias"] = _mm(g_a.T, r), g_a.sum(0)
    return (_mm(g_a, W1) + _mm(gy, Wr)) * (feature > 0)


def _sigmoid(s):
    return (1 / (1 + np.exp(-s))).astype(s.dtype)


def _kl(m1, s1, m2, s2):
    """torch.distributions.kl_divergence(Normal(m1, s1), Normal(m2, s2)), its expression."""
    ratio = (s1 / s2) ** 2
    t1 = ((m1 - m2) / s2) ** 2
    return (0.5 * (ratio + t1 - 1 - np.log(ratio))).astype(m2.dtype)


def head(state, feat_x, feat_y, eps_q, eps_p, G, dtype=np.float64, relu_inputs=None, prior_fix=None):
    """-> (values, grads).  relu_inputs, when a list, collects every array that enters a ReLU after the leaves.  dl_g's first
    distribution is DETACHED in the reference, and the gradients here leave it out accordingly; prior_fix = (p_mu, p_std), when
    given, stands in its place, so that a finite difference of the loss can hold it still as well."""
    f = dtype
    fx, fy, eq, ep, G = (np.asarray(t, f) for t in (feat_x, feat_y, eps_q, eps_p, G))
    B, Z = eq.shape
    h1, c1 = _block(state, "posterior_infer1.", fx, f)
    o_x, c2 = _block(state, "posterior_infer2.", h1, f)
    o_y, c3 = _block(state, "prior_infer.", fy, f)
    q_mu, q_raw, p_mu, p_raw = o_x[:, :Z], o_x[:, Z:], o_y[:, :Z], o_y[:, Z:]
    q_std, p_std = vh.softplus(q_raw), vh.softplus(p_raw)
    z = np.concatenate((q_mu + eq * q_std, p_mu + ep * p_std), 0)
    gen, c4 = _block(state, "generator.", z, f)
    rx = vh.relu(fx)
    global_feat = np.concatenate((rx, rx), 0) + gen
    dl_rec = _kl(np.zeros_like(p_mu), np.ones_like(p_std), p_mu, p_std)
    dl_g = _kl(*((p_mu, p_std) if prior_fix is None else (np.asarray(t, f) for t in prior_fix)), q_mu, q_std)
    values = dict(q_mu=q_mu, q_std=q_std, p_mu=p_mu, p_std=p_std, z=z, dl_rec=dl_rec, dl_g=dl_g, global_feat=global_feat)
    if relu_inputs is not None:
        relu_inputs += [c1[3], h1, c2[3], c3[3], z, c4[3]]
    # backward
    grads = {}
    gz = _block_backward(state, c4, G, f, grads)
    w = f(20) / f(B * Z)
    g_pm = w * p_mu / p_std ** 2 + gz[B:]
    g_ps = w * (1 / p_std - (1 + p_mu ** 2) / p_std ** 3) + gz[B:] * ep
    g_qm = -w * (p_mu - q_mu) / q_std ** 2 + gz[:B]
    g_qs = w * (1 / q_std - (p_std ** 2 + (p_mu - q_mu) ** 2) / q_std ** 3) + gz[:B] * eq
    g_ox = np.concatenate((g_qm, g_qs * _sigmoid(q_raw)), 1)
    g_oy = np.concatenate((g_pm, g_ps * _sigmoid(p_raw)), 1)
    grads["feat_y"] = _block_backward(state, c3, g_oy, f, grads)
    g_h1 = _block_backward(state, c2, g_ox, f, grads)
    grads["feat_x"] = _block_backward(state, c1, g_h1, f, grads) + (G[:B] + G[B:]) * (fx > 0)
    return values, {n: np.asarray(v, f) for n, v in grads.items()}
