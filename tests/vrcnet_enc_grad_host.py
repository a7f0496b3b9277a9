"""The NumPy backward of vrcnet_grad_host.py extended to SA_SKN_Res_encoder: vrcnet_host.encoder's
forward, given every discrete decision, with a closure that maps the output's gradient to (the input's gradient, {parameter name:
gradient}).  The four SKN_Res_units are vrcnet_grad_host's, the three poolings edge_pool_host's (the contract of houv_edge_pool
and its backward, in the caller's dtype), the rest is written out here: the maximum over points behind conv5 (the first maximum
takes the gradient), the two fc layers (dropout is the identity: eval()), conv6 on cat(global, x4), and three up-samplings whose
weights are constants.

`kinks`, when a list, receives (name, array) for every ReLU input; `tops`, when a list, receives (name, gap) for every maximum,
gap = the winner's lead over its runner-up (the poolings over each list, conv5 over the points)."""
import numpy as np

import ecg_host as eh
import edge_pool_host as ep
import vrcnet_grad_host as gh
import vrcnet_host as vh

relu, conv, conv_bw = vh.relu, vh.conv, gh.conv_bw
DECISIONS = tuple(f"{n}{l}" for l in (1, 2, 3) for n in ("fps", "knn_pt", "three_nn"))


def decision_names(knn_list):
    return [f"knn{l}_{i}" for l in (1, 2, 3, 4) for i in range(len(knn_list))] + list(DECISIONS)


def _rows(a):
    """[B,C,1,N] -> rows [B,N,C]."""
    return np.ascontiguousarray(np.swapaxes(a[:, :, 0], 1, 2))


def _chan(r):
    """rows [B,N,C] -> [B,C,1,N]."""
    return np.ascontiguousarray(np.swapaxes(r, 1, 2))[:, :, None, :]


def _gap(cand, axis):
    """The lead of the largest candidate over the second along `axis` (inf with a single candidate)."""
    if cand.shape[axis] < 2:
        return np.full(np.delete(cand.shape, axis), np.inf)
    s = np.sort(cand, axis=axis)
    return np.take(s, -1, axis=axis) - np.take(s, -2, axis=axis)


def _pool(x, p_idx, pn_idx, tops, name):
    rows = _rows(x)
    out, arg = ep.forward(rows, p_idx, pn_idx)
    if tops is not None:
        B, N, C = rows.shape
        nb = np.stack([rows[b, ep.clamp(pn_idx[b], N)] for b in range(B)])         # [B,S,pk,C]
        tops.append((name, _gap(nb, 2)))
    return _chan(out), lambda g: _chan(ep.backward(_rows(g).astype(rows.dtype), p_idx, pn_idx, arg, rows.shape[1]))


def _upsample(x, target, source, idx):
    """three_interpolate with constant weights: x[B,C,1,M] at `source` -> [B,C,1,N] at `target`."""
    w = eh.three_nn_weights(target, source, idx)
    out = eh.three_interpolate(x[:, :, 0], idx, w)[:, :, None, :]
    B, C, _, M = x.shape

    def backward(g):
        gx = np.zeros((B, M, C), x.dtype)
        gr = _rows(g)                                                              # [B,N,C]
        for b in range(B):
            np.add.at(gx[b], idx[b].reshape(-1), (gr[b][:, None, :] * w[b][:, :, None]).reshape(-1, C))
        return _chan(gx)
    return out, backward


def _linear(x, W, b):
    y = eh.rows_times(x, W) + b
    return y, lambda g: (gh._rt(g, W.T), gh._rt(g.T, x.T), g.sum(0))


def encoder(state, features, decisions, knn_list, pk, pts_num, dtype=np.float64, prefix="", kinks=None, tops=None, coords=None):
    """features[B,Cin,N], coordinates in channels 0..2, and every decision of decision_names(knn_list) -> (out[B,Cout,N],
    backward(gout) -> (gfeatures[B,Cin,N], grads)).  The interpolation weights are constants of the backward (the reference's
    three_nn is not differentiable); `coords`[B,3,N], when given, are the points they are computed from in place of
    features[:, :3] -- a difference quotient in `features` must hold them fixed."""
    features = np.asarray(features, dtype=dtype)
    B = features.shape[0]
    dec = {n: np.asarray(decisions[n]).astype(np.int64) for n in decision_names(knn_list)}
    wb = lambda n: vh._wb(state, prefix, n, dtype)
    pts = [np.ascontiguousarray(np.swapaxes(features[:, 0:3] if coords is None else np.asarray(coords, dtype=dtype), 1, 2))]
    kink = (lambda n, a: kinks.append((prefix + n, a))) if kinks is not None else (lambda n, a: None)

    units, pools, xs = [], [], []
    x = features[:, :, None, :]
    for level in (1, 2, 3, 4):
        lists = [dec[f"knn{level}_{i}"] for i in range(len(knn_list))]
        y, bw = gh.skn_res_unit(state, f"{prefix}sam_res{level}.", x, lists, dtype, kinks)
        kink(f"x{level}", y)
        units.append((y, bw))
        xs.append(relu(y))
        if level < 4:
            p_idx, pn_idx = dec[f"fps{level}"], dec[f"knn_pt{level}"]
            x, pbw = _pool(xs[-1], p_idx, pn_idx, tops, f"{prefix}pool{level}")
            pools.append(pbw)
            pts.append(np.stack([pts[-1][b, p_idx[b]] for b in range(B)]))
    x1, x2, x3, x4 = xs

    W5, b5 = wb("conv5")
    y5 = conv(x4, W5, b5)[:, :, 0]                                                 # [B,1024,S]
    if tops is not None:
        tops.append((prefix + "conv5", _gap(y5, 2)))
    a5 = y5.argmax(2)                                                              # the first maximum
    g0 = np.take_along_axis(y5, a5[:, :, None], 2)[:, :, 0]
    (Wf1, bf1), (Wf2, bf2) = wb("fc1"), wb("fc2")
    z1, l1 = _linear(g0, Wf1, bf1)
    z2, l2 = _linear(relu(z1), Wf2, bf2)
    kink("fc1", z1), kink("fc2", z2)
    g2 = relu(z2)
    S4 = x4.shape[-1]
    cat6 = np.concatenate([np.repeat(g2[:, :, None], S4, axis=2)[:, :, None, :], x4], 1)
    W6, b6 = wb("conv6")
    y6 = conv(cat6, W6, b6)
    kink("conv6", y6)
    ups, cats, ys = [], [cat6], [y6]
    y = relu(y6)
    for i, (name, skip) in enumerate((("conv7", x3), ("conv8", x2), ("conv9", x1)), start=1):
        u, ubw = _upsample(y, pts[3 - i], pts[4 - i], dec[f"three_nn{i}"])
        ups.append(ubw)
        cats.append(np.concatenate([u, skip], 1))
        ys.append(conv(cats[-1], *wb(name)))
        kink(name, ys[-1])
        y = relu(ys[-1])
    Wo, bo = wb("conv_out")
    out = conv(y, Wo, bo)[:, :, 0]
    assert out.dtype == dtype

    def backward(gout):
        grads = {}

        def put(name, gW, gb):
            grads[f"{prefix}{name}.weight"] = gW.reshape(np.asarray(state[f"{prefix}{name}.weight"]).shape)
            grads[f"{prefix}{name}.bias"] = gb

        g, gW, gb = conv_bw(relu(ys[3]), Wo, np.asarray(gout, dtype=dtype)[:, :, None, :])
        put("conv_out", gW, gb)
        skips = [None] * 4                                                         # the gradients of x1 .. x4 from the decoder half
        for i, name in ((3, "conv9"), (2, "conv8"), (1, "conv7")):
            g, gW, gb = conv_bw(cats[i], wb(name)[0], g * (ys[i] > 0))
            put(name, gW, gb)
            cu = g.shape[1] - xs[3 - i].shape[1]
            skips[3 - i] = g[:, cu:]
            g = ups[i - 1](np.ascontiguousarray(g[:, :cu]))
        g, gW, gb = conv_bw(cat6, W6, g * (y6 > 0))
        put("conv6", gW, gb)
        gx4 = g[:, 1024:]
        gg2 = g[:, :1024, 0].sum(2)                                                # repeat's backward: the points are added
        gz, gW, gb = l2(gg2 * (z2 > 0))
        grads[prefix + "fc2.weight"], grads[prefix + "fc2.bias"] = gW, gb
        gz, gW, gb = l1(gz * (z1 > 0))
        grads[prefix + "fc1.weight"], grads[prefix + "fc1.bias"] = gW, gb
        gy5 = np.zeros_like(y5)
        np.put_along_axis(gy5, a5[:, :, None], gz[:, :, None], 2)
        g, gW, gb = conv_bw(x4, W5, gy5[:, :, None, :])
        put("conv5", gW, gb)
        skips[3] = gx4 + g
        g = None
        for level in (4, 3, 2, 1):
            gx = skips[level - 1] if g is None else skips[level - 1] + g
            yl, bw = units[level - 1]
            g, gi = bw(gx * (yl > 0))
            grads.update(gi)
            if level > 1:
                g = pools[level - 2](g)
        return g[:, :, 0], grads
    return out, backward


def spread(a32, a64):
    """max |float32 restatement - float64 restatement|: the yardstick of the model-level bound."""
    return float(np.abs(np.asarray(a32, dtype=np.float64) - a64).max())
