"""Restatements for VRCNet training in the REFERENCE's materialising form, beside the forwards of
vrcnet_host.py: the backward passes of sa_module, sk_sa_module and skn_res_unit in NumPy, parametrised by dtype.  The real
[B, C, k, N] edge tensor, its two projections, the repeated [B, mid, k, N] weight tensor, their product and the gradients of all
of them exist, and the neighbour path is a scatter-add over the edges in ascending (point, slot).  Neighbour indices outside
0..N-1 are clamped, as houv_sa_attn clamps them.

Every function returns its output and a closure that maps the output's gradient to (the input's gradient, {parameter name:
gradient}); `kinks`, when a list, receives (name, array) for every ReLU input, so that a caller can ask how far each lies from 0.

sa_attn_backward is the contract of houv_sa_attn_backward on rows: (P, idx, Ww1, Ww2, bw2, G) -> gP, ro, gWw1, gWw2, gbw2.

float32 products are summed over k ascending, one product and one addition per term (pcn_host.rows_times: the same spread on
every host); float64, the yardstick, uses matmul."""
import numpy as np

import ecg_host as eh
import vrcnet_host as vh

relu, conv, SHARE = vh.relu, vh.conv, vh.SHARE


def _rows(a):
    """a[B,C,...] -> [B * ..., C]."""
    return np.ascontiguousarray(np.moveaxis(a, 1, -1)).reshape(-1, a.shape[1])


def _rt(x, W):
    return eh.rows_times(np.ascontiguousarray(x), np.ascontiguousarray(W))


def conv_bw(x, W, gy):
    """The backward of y = conv(x, W, b): (gx, gW[Cout,Cin], gb[Cout])."""
    gyr = _rows(gy)
    return conv(gy, np.ascontiguousarray(W.T), np.zeros(W.shape[1], W.dtype)), _rt(gyr.T, _rows(x).T), gyr.sum(0)


def _edges(x, j):
    """get_edge_features for clamped lists j: x[B,C,N] -> [B,C,k,N]."""
    return vh.get_edge_features(x, j)


def _scatter(g, j):
    """The transpose of _edges: g[B,C,k,N] summed into [B,C,N] at destination j[b,n,slot], sources in ascending (n, slot)."""
    B, C, k, N = g.shape
    out = np.zeros((B, N, C), g.dtype)
    ge = np.ascontiguousarray(np.transpose(g, (0, 3, 2, 1)))                      # [B,N,k,C]
    for b in range(B):
        np.add.at(out[b], j[b].reshape(-1), ge[b].reshape(-1, C))
    return np.ascontiguousarray(np.swapaxes(out, 1, 2))


def _attn(x1, x2n, x3n, Ww1, Ww2, bw2, kinks=None, tag=""):
    """SA_module.forward between the projections and conv_out: x1[B,rel,1,N], x2n[B,rel,k,N], x3n[B,mid,k,N] -> (o[B,mid,1,N]
    BEFORE its ReLU, backward(g of relu(o)) -> (g_x1, g_x2n, g_x3n, gWw1, gWw2, gbw2))."""
    dtype = x1.dtype
    B, rel, k, N = x2n.shape
    t = np.concatenate([x1, np.ascontiguousarray(x2n).reshape(B, -1, 1, N)], 1)   # B rel(k+1) 1 N
    rt = relu(t)
    pre = conv(rt, Ww1, np.zeros(Ww1.shape[0], dtype))
    h = relu(pre)
    wv = conv(h, Ww2, bw2)                                                        # B km 1 N
    w = np.tile(np.ascontiguousarray(wv).reshape(B, -1, k, N), (1, SHARE, 1, 1))
    assert w.shape == x3n.shape
    o = np.zeros((B, w.shape[1], 1, N), dtype)
    for j in range(k):
        o[:, :, 0] += w[:, :, j] * x3n[:, :, j]
    if kinks is not None:
        kinks += [(tag + "t", t), (tag + "pre", pre), (tag + "o", o)]

    def backward(gro):
        go = gro * (o > 0)                                                        # B mid 1 N
        gw_full = go * x3n                                                        # B mid k N: the repeated weights' gradient
        g_x3n = go * w
        m = w.shape[1] // SHARE
        gw = np.zeros((B, m, k, N), dtype)
        for s in range(SHARE):                                                    # repeat's backward: the tiles are added
            gw += gw_full[:, s * m:(s + 1) * m]
        gwv = gw.reshape(B, m * k, 1, N)
        gh, gWw2, gbw2 = conv_bw(h, Ww2, gwv)
        gpre = gh * (pre > 0)
        grt, gWw1, _ = conv_bw(rt, Ww1, gpre)
        gt = grt * (t > 0)
        return gt[:, :rel], np.ascontiguousarray(gt[:, rel:]).reshape(B, rel, k, N), g_x3n, gWw1, gWw2, gbw2
    return o, backward


def sa_attn_backward(P, idx, Ww1, Ww2, bw2, G, dtype=np.float64):
    """The contract of houv_sa_attn_backward: P[B,N,2 rel + mid] rows, idx[B,N,k], G[B,N,mid] -> dict(gP, ro, gWw1, gWw2, gbw2,
    and the ReLU inputs t, pre, o)."""
    P, Ww1, Ww2, bw2, G = (np.asarray(a, dtype=dtype) for a in (P, Ww1, Ww2, bw2, G))
    B, N, wp = P.shape
    rel = wp // 6
    j = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    Pc = np.ascontiguousarray(np.swapaxes(P, 1, 2))
    kinks = []
    o, bw = _attn(Pc[:, :rel, None, :], _edges(Pc[:, rel:2 * rel], j), _edges(Pc[:, 2 * rel:], j), Ww1, Ww2, bw2, kinks)
    g1, g2, g3, gWw1, gWw2, gbw2 = bw(np.ascontiguousarray(np.swapaxes(G, 1, 2))[:, :, None, :])
    gP = np.concatenate([g1[:, :, 0], _scatter(g2, j), _scatter(g3, j)], 1)
    res = dict(gP=np.ascontiguousarray(np.swapaxes(gP, 1, 2)), ro=np.ascontiguousarray(np.swapaxes(relu(o)[:, :, 0], 1, 2)),
               gWw1=gWw1, gWw2=gWw2, gbw2=gbw2, **{n: a for n, a in kinks})
    assert all(res[n].dtype == dtype for n in OP_GRADS)
    return res


OP_GRADS = ("gP", "ro", "gWw1", "gWw2", "gbw2")


def sa_module(state, prefix, x, idx, relu_out=False, dtype=np.float64, kinks=None):
    """vrcnet_host.sa_module (followed by relu when relu_out: SK_SA_module's activation) -> (out[B,C,1,N], backward)."""
    x = np.asarray(x, dtype=dtype)
    B, _, _, N = x.shape
    j = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    wb = lambda n: vh._wb(state, prefix, n, dtype)
    xr = relu(x)
    xn = _edges(xr[:, :, 0], j)                                                   # B C K N
    (W1, b1), (W2, b2), (W3, b3), (Wo, bo) = wb("conv1"), wb("conv2"), wb("conv3"), wb("conv_out")
    Ww1, (Ww2, bw2) = wb("conv_w.1")[0], wb("conv_w.3")
    tag = prefix
    o, attn_bw = _attn(conv(xr, W1, b1), conv(xn, W2, b2), conv(xn, W3, b3), Ww1, Ww2, bw2, kinks, tag)
    ro = relu(o)
    y = conv(ro, Wo, bo) + x
    if kinks is not None:
        kinks.append((tag + "x", x))
        if relu_out:
            kinks.append((tag + "y", y))
    out = relu(y) if relu_out else y
    assert out.dtype == dtype

    def backward(gout):
        gy = np.asarray(gout, dtype=dtype) * (y > 0) if relu_out else np.asarray(gout, dtype=dtype)
        gro, gWo, gbo = conv_bw(ro, Wo, gy)
        g1, g2, g3, gWw1, gWw2, gbw2 = attn_bw(gro)
        gxr, gW1, gb1 = conv_bw(xr, W1, g1)
        gxn2, gW2, gb2 = conv_bw(xn, W2, g2)
        gxn3, gW3, gb3 = conv_bw(xn, W3, g3)
        gxr = gxr + _scatter(gxn2 + gxn3, j)[:, :, None, :]
        gx = gxr * (x > 0) + gy
        shaped = lambda n, g: g.reshape(np.asarray(state[prefix + n]).shape)
        grads = {prefix + n: shaped(n, g) for n, g in (
            ("conv1.weight", gW1), ("conv1.bias", gb1), ("conv2.weight", gW2), ("conv2.bias", gb2), ("conv3.weight", gW3),
            ("conv3.bias", gb3), ("conv_w.1.weight", gWw1), ("conv_w.3.weight", gWw2), ("conv_w.3.bias", gbw2),
            ("conv_out.weight", gWo), ("conv_out.bias", gbo))}
        return gx, grads
    return out, backward


def sk_sa_module(state, prefix, x, idxs, dtype=np.float64, kinks=None):
    """vrcnet_host.sk_sa_module -> (out, backward).  With one list the softmax is exactly 1 and fc / fcs receive exact zeros."""
    x = np.asarray(x, dtype=dtype)
    branches = [sa_module(state, f"{prefix}sams.{i}.", x, idx, True, dtype, kinks) for i, idx in enumerate(idxs)]
    feas = np.stack([b[0] for b in branches], 1)                                  # B n C 1 N
    N = x.shape[-1]
    fea_s = feas.sum(1).mean(-1).mean(-1)
    W, b = vh._wb(state, prefix, "fc", dtype)
    fea_z = eh.rows_times(fea_s, W) + b
    Ws = [vh._wb(state, prefix, f"fcs.{i}", dtype) for i in range(len(idxs))]
    vec = np.stack([eh.rows_times(fea_z, Wi) + bi for Wi, bi in Ws], 1)
    e = np.exp(vec - vec.max(1, keepdims=True))
    att = e / e.sum(1, keepdims=True)                                             # B n C
    out = (feas * att[:, :, :, None, None]).sum(1)
    assert out.dtype == dtype

    def backward(gout):
        gout = np.asarray(gout, dtype=dtype)
        g_att = (gout[:, None] * feas).sum((3, 4))                                # B n C
        g_vec = att * (g_att - (att * g_att).sum(1, keepdims=True))
        grads = {}
        g_fea_z = np.zeros_like(fea_z)
        for i, (Wi, _) in enumerate(Ws):
            g_fea_z = g_fea_z + _rt(g_vec[:, i], Wi.T)
            grads[f"{prefix}fcs.{i}.weight"] = _rt(g_vec[:, i].T, fea_z.T)
            grads[f"{prefix}fcs.{i}.bias"] = g_vec[:, i].sum(0)
        grads[prefix + "fc.weight"], grads[prefix + "fc.bias"] = _rt(g_fea_z.T, fea_s.T), g_fea_z.sum(0)
        g_mean = (_rt(g_fea_z, W.T) / dtype(N))[:, :, None, None]
        gx = np.zeros_like(x)
        for i, (_, bw) in enumerate(branches):
            gxi, gi = bw(gout * att[:, i][:, :, None, None] + g_mean)
            gx = gx + gxi
            grads.update(gi)
        return gx, grads
    return out, backward


def skn_res_unit(state, prefix, feat, idxs, dtype=np.float64, kinks=None, af_mask=True):
    """vrcnet_host.skn_res_unit -> (out, backward); the number of SK_SA_modules is read off the state.  af_mask=False leaves
    self.af's mask out of the backward (what the device module does: its input is >= 0, and the tests show nothing changes)."""
    feat = np.asarray(feat, dtype=dtype)
    Wc1, Wc2, Wr = (vh._wb(state, prefix, n, dtype)[0] for n in ("conv1", "conv2", "conv_res"))
    zero = lambda W: np.zeros(W.shape[0], dtype)
    x = conv(feat, Wc1, zero(Wc1))
    layers = []
    while f"{prefix}sam.{len(layers)}.fc.weight" in state:
        x, bw = sk_sa_module(state, f"{prefix}sam.{len(layers)}.", x, idxs, dtype, kinks)
        layers.append(bw)
    assert layers
    if kinks is not None:
        kinks.append((prefix + "af", x))
    xa = relu(x)
    out = conv(xa, Wc2, zero(Wc2)) + conv(feat, Wr, zero(Wr))
    assert out.dtype == dtype

    def backward(gout):
        gout = np.asarray(gout, dtype=dtype)
        gxa, gW2, _ = conv_bw(xa, Wc2, gout)
        gfeat, gWr, _ = conv_bw(feat, Wr, gout)
        g = gxa * (x > 0) if af_mask else gxa
        grads = {}
        for bw in reversed(layers):
            g, gi = bw(g)
            grads.update(gi)
        g0, gW1, _ = conv_bw(feat, Wc1, g)
        shaped = lambda n, a: a.reshape(np.asarray(state[prefix + n]).shape)
        grads.update({prefix + "conv1.weight": shaped("conv1.weight", gW1), prefix + "conv2.weight": shaped("conv2.weight", gW2),
                      prefix + "conv_res.weight": shaped("conv_res.weight", gWr)})
        return gfeat + g0, grads
    return out, backward


def margin(kinks):
    """The smallest |ReLU input| that is not exactly 0 (an exact 0 is no kink of the gradient: both sides agree it is 0)."""
    best = np.inf
    for _, a in kinks:
        nz = np.abs(a[a != 0])
        if nz.size:
            best = min(best, float(nz.min()))
    return best


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def sa_state(rng, prefix, C, k):
    rel, mid, m = C // 16, C // 4, C // 32
    u = lambda shape, fan: ((rng.random(shape) * 2 - 1) / np.sqrt(fan)).astype(np.float32)
    s = {}
    for n, co, ci, bias in (("conv1", rel, C, True), ("conv2", rel, C, True), ("conv3", mid, C, True),
                            ("conv_w.1", m, rel * (k + 1), False), ("conv_w.3", k * m, m, True), ("conv_out", C, mid, True)):
        s[f"{prefix}{n}.weight"] = u((co, ci, 1, 1), ci)
        if bias:
            s[f"{prefix}{n}.bias"] = u((co,), ci)
    return s


def sk_state(rng, prefix, C, ks):
    d = max(C // 2, 32)
    u = lambda shape, fan: ((rng.random(shape) * 2 - 1) / np.sqrt(fan)).astype(np.float32)
    s = {}
    for i, k in enumerate(ks):
        s.update(sa_state(rng, f"{prefix}sams.{i}.", C, k))
    s[prefix + "fc.weight"], s[prefix + "fc.bias"] = u((d, C), C), u((d,), C)
    for i in range(len(ks)):
        s[f"{prefix}fcs.{i}.weight"], s[f"{prefix}fcs.{i}.bias"] = u((C, d), d), u((C,), d)
    return s


def unit_state(rng, prefix, cin, cout, ks, layers):
    u = lambda shape, fan: ((rng.random(shape) * 2 - 1) / np.sqrt(fan)).astype(np.float32)
    s = {prefix + "conv1.weight": u((cout, cin, 1, 1), cin)}
    for l in range(layers):
        s.update(sk_state(rng, f"{prefix}sam.{l}.", cout, ks))
    s[prefix + "conv2.weight"], s[prefix + "conv_res.weight"] = u((cout, cout, 1, 1), cout), u((cout, cin, 1, 1), cin)
    return s


def op_case(seed, B, N, C, k, min_margin=1e-5, idx=None):
    """Seeded inputs of houv_sa_attn_backward whose float64 ReLU inputs t, pre and o stay >= min_margin from 0: the seed is
    advanced until they do.  -> dict(P, idx, Ww1, Ww2, bw2, G)."""
    rel, mid, m = C // 16, C // 4, C // 32
    for s in range(seed * 64, seed * 64 + 64):
        rng = np.random.default_rng(s)
        c = dict(P=rng.standard_normal((B, N, 2 * rel + mid)).astype(np.float32),
                 idx=rng.integers(0, N, (B, N, k)).astype(np.int32) if idx is None else np.asarray(idx, dtype=np.int32),
                 Ww1=(rng.standard_normal((m, rel * (k + 1))) / np.sqrt(rel * (k + 1))).astype(np.float32),
                 Ww2=(rng.standard_normal((k * m, m)) / np.sqrt(m)).astype(np.float32),
                 bw2=(0.1 * rng.standard_normal(k * m)).astype(np.float32),
                 G=rng.standard_normal((B, N, mid)).astype(np.float32))
        r = sa_attn_backward(**c)
        if min(np.abs(r[n]).min() for n in ("t", "pre", "o")) >= min_margin:
            return c
    raise AssertionError("no seed keeps the ReLU inputs away from 0")
