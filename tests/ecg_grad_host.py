"""Restatements for ECG training in the REFERENCE's materialising form.

dense_conv_backward: the backward pass of ecg_host.dense_conv (the contract of houv_dense_conv_backward) in NumPy, parametrised
by dtype -- the [B, N, k, 2C] edge tensor, the three growing concatenations and their gradients all exist, and the neighbour
path is a scatter-add over the edges.  The arg-max of the pooling may be INJECTED (`arg=`), as the network's other discrete
decisions are: given it, the gradient is a continuous function of the inputs away from the ReLU kinks.

float32 products are summed over k ascending, one product and one addition per term (pcn_host.rows_times: the same spread on
every host); float64, the yardstick, uses matmul."""
import numpy as np

import ecg_host as host

G = host.G


def _rt(x, W):
    return host.rows_times(np.ascontiguousarray(x), np.ascontiguousarray(W))


def dense_conv_forward_rows(x, idx, W0, b0, W1, b1, W2, b2, dtype=np.float64):
    """x[B,N,C] rows, idx[B,N,k] (clamped into 0..N-1) -> dict of the materialised tensors: e[B,N,k,2C], z0, z1 (the ReLU
    inputs), full[B,N,k,C+72] = cat(y0, x_i, s1, s2), c1, c2."""
    x, W0, b0, W1, b1, W2, b2 = (np.asarray(a, dtype=dtype) for a in (x, W0, b0, W1, b1, W2, b2))
    B, N, C = x.shape
    k = idx.shape[2]
    j = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    xi = np.repeat(x[:, :, None, :], k, axis=2)
    xj = x[np.arange(B)[:, None, None], j]
    e = np.concatenate([xi, xj - xi], 3)
    z0 = _rt(e, W0) + b0
    y0 = np.maximum(z0, 0)
    c1 = np.concatenate([y0, xi], 3)
    z1 = _rt(c1, W1) + b1
    s1 = np.maximum(z1, 0)
    c2 = np.concatenate([c1, s1], 3)
    s2 = _rt(c2, W2) + b2
    full = np.concatenate([c2, s2], 3)
    assert full.dtype == dtype
    return dict(j=j, e=e, z0=z0, z1=z1, c1=c1, c2=c2, full=full)


def pooled_columns(C):
    """The columns of out that are maxima over the neighbours (y0, s1, s2), in the order of arg's 72 entries."""
    return np.concatenate([np.arange(G), G + C + np.arange(2 * G)])


def dense_conv_backward(x, idx, W0, b0, W1, b1, W2, b2, gout, relu_out=False, arg=None, dtype=np.float64):
    """-> dict(out[B,N,C+72], arg[B,N,72] (the one used), gx[B,N,C], gW0, gb0, gW1, gb1, gW2, gb2, z0, z1).  `arg` None: the
    first maximum (torch.max's rule on the CPU)."""
    f = dense_conv_forward_rows(x, idx, W0, b0, W1, b1, W2, b2, dtype)
    W0, W1, W2, gout = (np.asarray(a, dtype=dtype) for a in (W0, W1, W2, gout))
    B, N, C = np.asarray(x).shape
    k = idx.shape[2]
    full = f["full"]
    out = full.max(2)
    cols = pooled_columns(C)
    if arg is None:
        arg = full[..., cols].argmax(2)
    arg = np.asarray(arg, dtype=np.int64)
    if relu_out:
        g = gout * (out > 0)
        out = np.maximum(out, 0)
    else:
        g = gout
    gfull = np.zeros_like(full)
    onehot = (arg[:, :, None, :] == np.arange(k)[None, None, :, None])           # [B,N,k,72]; arg = -1 selects nothing
    gfull[..., cols] = onehot * g[:, :, None, cols]
    gfull[:, :, 0, G:G + C] = g[..., G:G + C]                                    # the pass-through columns: every edge ties, the first wins
    flat = lambda a: a.reshape(-1, a.shape[-1])
    gs2 = gfull[..., 2 * G + C:]
    gc2 = gfull[..., :2 * G + C] + _rt(gs2, W2.T)
    gW2, gb2 = _rt(flat(gs2).T, flat(f["c2"]).T), flat(gs2).sum(0)
    gz1 = gc2[..., G + C:] * (f["z1"] > 0)
    gc1 = gc2[..., :G + C] + _rt(gz1, W1.T)
    gW1, gb1 = _rt(flat(gz1).T, flat(f["c1"]).T), flat(gz1).sum(0)
    gz0 = gc1[..., :G] * (f["z0"] > 0)
    ge = _rt(gz0, W0.T)
    gW0, gb0 = _rt(flat(gz0).T, flat(f["e"]).T), flat(gz0).sum(0)
    gx = (gc1[..., G:] + ge[..., :C] - ge[..., C:]).sum(2)
    for b in range(B):                                                           # the neighbour path, to the clamped row
        np.add.at(gx[b], f["j"][b].reshape(-1), ge[b, :, :, C:].reshape(-1, C))
    res = dict(out=out, arg=arg, gx=gx, gW0=gW0, gb0=gb0, gW1=gW1, gb1=gb1, gW2=gW2, gb2=gb2, z0=f["z0"], z1=f["z1"], full=full)
    assert gx.dtype == dtype and gW0.dtype == dtype
    return res


def loss(x, idx, W0, b0, W1, b1, W2, b2, gout, relu_out=False):
    """L = <gout, out> in float64: what dense_conv_backward differentiates."""
    f = dense_conv_forward_rows(x, idx, W0, b0, W1, b1, W2, b2, np.float64)
    out = f["full"].max(2)
    if relu_out:
        out = np.maximum(out, 0)
    return float((np.asarray(gout, dtype=np.float64) * out).sum())


GRADS = ("gx", "gW0", "gb0", "gW1", "gb1", "gW2", "gb2")


def random_case(seed, B, N, C, k, margin=1e-5, idx=None):
    """Seeded inputs whose float64 ReLU inputs stay >= `margin` from 0 (asserted by the caller through res['z0'], res['z1']):
    the seed is advanced until they do.  -> dict(x, idx, W0, b0, W1, b1, W2, b2, gout)."""
    for s in range(seed * 64, seed * 64 + 64):
        rng = np.random.default_rng(s)
        c = dict(x=rng.standard_normal((B, N, C)).astype(np.float32),
                 idx=rng.integers(0, N, (B, N, k)).astype(np.int32),
                 W0=(rng.standard_normal((G, 2 * C)) / np.sqrt(2 * C)).astype(np.float32),
                 b0=(0.1 * rng.standard_normal(G)).astype(np.float32),
                 W1=(rng.standard_normal((G, G + C)) / np.sqrt(G + C)).astype(np.float32),
                 b1=(0.1 * rng.standard_normal(G)).astype(np.float32),
                 W2=(rng.standard_normal((G, 2 * G + C)) / np.sqrt(2 * G + C)).astype(np.float32),
                 b2=(0.1 * rng.standard_normal(G)).astype(np.float32),
                 gout=rng.standard_normal((B, N, C + 3 * G)).astype(np.float32))
        if idx is not None:                      # drawn all the same, so that x does not depend on whether lists are given
            c["idx"] = np.ascontiguousarray(idx(c["x"]) if callable(idx) else idx, dtype=np.int32)   # a callable: lists made from x
        f = dense_conv_forward_rows(c["x"], c["idx"], c["W0"], c["b0"], c["W1"], c["b1"], c["W2"], c["b2"])
        if min(np.abs(f["z0"]).min(), np.abs(f["z1"]).min()) >= margin:
            return c
    raise AssertionError("no seed keeps the ReLU inputs away from 0")


# ---------------------------------------------------------------------------------------------------------------------------
# the whole network in torch on the CPU, the reference's materialising form, every decision INJECTED; autograd is its backward
# ---------------------------------------------------------------------------------------------------------------------------
def torch_model(state, x, num_points, num_coarse, decisions, dtype=None, encoder_only=None, kinks=None):
    """ecg_host.model restated in torch (scale 1): state maps parameter names to torch tensors (leaves that require grad, of the
    dtype wanted), x[B,3,N] array, decisions as ecg_host.model takes them (all of them: nothing is searched here).
    -> dict(feat[B,1024], out1[B,nc,3], out2[B,num_points,3]) of torch tensors carrying the graph.
    encoder_only: a parameter prefix ("" for a bare EF_encoder's state): x[B,3,N] goes straight into EF_encoder.forward and the
    result is dict(out[B,256,N]).  kinks, when a dict, receives under "relu" every ReLU input and under "pool" every pool's
    candidates with the pooled axis last (detached arrays, in call order): where the gradient is discontinuous."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or next(iter(state.values())).dtype
    x = torch.as_tensor(np.asarray(x), dtype=dtype)
    dec = {n: torch.as_tensor(np.asarray(v).astype(np.int64)) for n, v in decisions.items()}
    B = x.shape[0]
    w = lambda n: state[n + ".weight"].reshape(state[n + ".weight"].shape[0], -1)
    b = lambda n: state[n + ".bias"]
    conv = lambda n, t: torch.einsum("oc,bc...->bo...", w(n), t) + b(n).reshape((1, -1) + (1,) * (t.dim() - 2))
    lin = lambda n, t: t @ w(n).T + b(n)

    def relu(t):
        if kinks is not None:
            kinks.setdefault("relu", []).append(t.detach().numpy())
        return F.relu(t)

    def pool(t, dim):
        if kinks is not None:
            kinks.setdefault("pool", []).append(np.moveaxis(t.detach().numpy(), dim, -1))
        return t.max(dim).values

    def take(t, idx):                                                            # t[B,C,N], idx[B,...] -> [B,C,...]
        flat = idx.reshape(B, 1, -1).expand(-1, t.shape[1], -1)
        return torch.gather(t, 2, flat).reshape((B, t.shape[1]) + tuple(idx.shape[1:]))

    def dense(prefix, t, idx):
        k = idx.shape[2]
        nb = take(t, idx)                                                        # [B,C,N,k]
        centre = t.unsqueeze(3).expand(-1, -1, -1, k)
        y = relu(conv(prefix + "first_conv", torch.cat((centre, nb - centre), 1)))
        y = torch.cat((y, centre), 1)
        y = torch.cat((y, relu(conv(prefix + "model.stack_conv_1.model.conv", y))), 1)
        y = torch.cat((y, conv(prefix + "model.stack_conv_2.model.conv", y)), 1)
        return pool(y, 3)

    if encoder_only is None:
        y = conv("encoder.conv2", relu(conv("encoder.conv1", x)))
        g = pool(y, 2)
        y = torch.cat((y, g.unsqueeze(2).expand(-1, -1, y.shape[2])), 1)
        feat = pool(conv("encoder.conv4", relu(conv("encoder.conv3", y))), 2)
        c = relu(lin("decoder.fc2", relu(lin("decoder.fc1", feat))))
        coarse = lin("decoder.fc3", c).reshape(B, 3, num_coarse)
        pts = torch.cat((coarse, x), 2)
        e = "decoder.encoder."
    else:
        pts, e = x, encoder_only
    pc = [pts.detach()]

    def sample(i, feat_):
        p_idx, pn_idx = dec[f"fps{i}"], dec[f"knn_pt{i}"]
        pc.append(take(pc[-1], p_idx))
        return torch.cat((take(feat_, p_idx), pool(take(feat_, pn_idx), 3)), 1)

    def level(i, t):
        t = relu(conv(e + f"conv{i}", t))
        return relu(dense(e + f"dense_conv{i}.", t, dec[f"knn_feat{i}"])), t
    x1, x0 = level(1, pts)
    x1 = torch.cat((x1, x0), 1)
    x1d = sample(1, x1)
    x2 = torch.cat((level(2, x1d)[0], x1d), 1)
    x2d = sample(2, x2)
    x3 = torch.cat((level(3, x2d)[0], x2d), 1)
    x3d = sample(3, x3)
    x4 = torch.cat((level(4, x3d)[0], x3d), 1)
    gf = pool(conv(e + "gf_conv", x4), 2)
    gf = relu(lin(e + "fc2", relu(lin(e + "fc1", gf))))
    x4 = relu(conv(e + "conv5", torch.cat((gf.unsqueeze(2).expand(-1, -1, x4.shape[2]), x4), 1)))

    def up(i, f, target, source):
        idx = dec[f"three_nn{i}"]
        nb = take(source, idx)                                                   # [B,3,N,3]
        d = nb - target.unsqueeze(3)
        dist = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        inv = 1 / dist.clamp_min(1e-10)
        wgt = (inv / inv.sum(2, keepdim=True)).unsqueeze(1)
        fn = take(f, idx)
        return (wgt[..., 0] * fn[..., 0] + wgt[..., 1] * fn[..., 1]) + wgt[..., 2] * fn[..., 2]
    x4 = up(1, x4, pc[2], pc[3])
    x3 = up(2, relu(conv(e + "conv6", torch.cat((x3, x4), 1))), pc[1], pc[2])
    x2 = up(3, relu(conv(e + "conv7", torch.cat((x2, x3), 1))), pc[0], pc[1])
    dense_out = conv(e + "conv8", torch.cat((x1, x2), 1))
    if encoder_only is not None:
        return dict(out=dense_out)
    fine = conv("decoder.conv2", relu(conv("decoder.conv1", dense_out)))
    if fine.shape[2] > num_points:
        fine = take(fine, dec["fps_out"])
    return dict(feat=feat, out1=coarse.transpose(1, 2), out2=fine.transpose(1, 2))


def torch_model_grads(state_np, x, num_points, num_coarse, decisions, G1, G2, dtype):
    """(outputs as arrays, the gradients of L = <G1, out1> + <G2, out2> per parameter name as arrays) of torch_model."""
    import torch
    state = {n: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for n, v in state_np.items()}
    res = torch_model(state, x, num_points, num_coarse, decisions, dtype)
    loss = (res["out1"] * torch.as_tensor(G1, dtype=dtype)).sum() + (res["out2"] * torch.as_tensor(G2, dtype=dtype)).sum()
    loss.backward()
    return {n: v.detach().numpy() for n, v in res.items()}, {n: v.grad.numpy() for n, v in state.items()}


def torch_encoder_grads(state_np, x, decisions, G, dtype, kinks=None):
    """(out[B,256,N], the gradients of L = <G, out> per parameter name) of the bare EF_encoder (torch_model(encoder_only=""))."""
    import torch
    state = {n: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for n, v in state_np.items()}
    out = torch_model(state, x, None, None, decisions, dtype, encoder_only="", kinks=kinks)["out"]
    (out * torch.as_tensor(G, dtype=dtype)).sum().backward()
    return out.detach().numpy(), {n: v.grad.numpy() for n, v in state.items()}
