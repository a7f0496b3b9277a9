"""NumPy restatement of the VRCNet completion network (completion/models/vrcnet.py, completion/model_utils.py) in the
REFERENCE's materialising form -- channel-major [B, C, 1, N] activations, the real [B, C, k, N] edge tensor with its two
projections, `view` / `repeat` of the attention weights, `repeat` + `cat` of the global feature and of Folding's input --
parametrised by dtype, so that what houv_sa_attn fuses away and the splits the model relies on are tested, not assumed.  Built on
ecg_host.py and pcn_host.py the way ecg_host.py is built on pcn_host.py.

Every discrete decision can be INJECTED (`decisions`: names as `decision_names` lists them); whatever is missing is computed
here (direct squared distances, stable sort).  The decisions that were used are always returned.  The latent sample z is an input.

float32 products are summed over k ascending, one product and one addition per term (pcn_host.rows_times); float64, the
yardstick, uses matmul."""
import types

import numpy as np

import ecg_host as eh
import pcn_host
from pointops_host import fps as _fps

relu, conv, take, rows_times, nearest = eh.relu, eh.conv, eh.take, eh.rows_times, eh.nearest
SHARE = 8
PTS_NUM = (3072, 1536, 768, 384)      # SA_SKN_Res_encoder's default, which MSAP_SKN_decoder never overrides


def cfg(layers=(1, 1, 1, 1), knn_list=(16,), pk=10, points_label=True, local_folding=True, num_coarse_raw=1024, num_input=2048,
        num_fps=2048, num_coarse=2048, num_points=2048):
    return types.SimpleNamespace(layers=tuple(layers), knn_list=tuple(knn_list), pk=pk, points_label=points_label,
                                 local_folding=local_folding, num_coarse_raw=num_coarse_raw, num_input=num_input, num_fps=num_fps,
                                 num_coarse=num_coarse, num_points=num_points,
                                 up_scale=int(np.ceil(num_points / (num_coarse_raw + 2048))))


def decision_names(c):
    """The decisions of one forward, in the order in which the network takes them."""
    n_enc = c.num_coarse_raw + c.num_input
    names = []
    for level in (1, 2, 3, 4):
        names += [f"knn{level}_{i}" for i in range(len(c.knn_list))]
        if level < 4:
            names += [f"fps{level}", f"knn_pt{level}"]
    names += ["three_nn1", "three_nn2", "three_nn3"]
    if c.up_scale >= 2:
        names.append("knn_exp1")
    n_high = n_enc * max(c.up_scale, 1)
    if n_high > c.num_fps:
        names.append("fps_out")
    if min(n_high, c.num_fps) > c.num_coarse:
        names.append("topk")
    if c.num_coarse < c.num_points and not c.local_folding:
        names.append("knn_exp2")
    return names


def _wb(state, prefix, name, dtype):
    w = np.asarray(state[prefix + name + ".weight"], dtype=dtype)
    b = state.get(prefix + name + ".bias")
    return w.reshape(w.shape[0], -1), (np.zeros(w.shape[0], dtype) if b is None else np.asarray(b, dtype=dtype))


def get_edge_features(x, idx):
    """model_utils.py:119-132: x[B,C,N], idx[B,N,k] -> [B,C,k,N]."""
    return np.ascontiguousarray(np.swapaxes(take(x, idx), 2, 3))


def sa_module(state, prefix, x, idx, dtype=np.float64):
    """SA_module.forward (vrcnet.py:49-67) as written: x[B,C,1,N], idx[B,N,k] -> [B,C,1,N]."""
    x = np.asarray(x, dtype=dtype)
    B, _, _, N = x.shape
    k = idx.shape[2]
    identity = x
    x = relu(x)
    xn = get_edge_features(x[:, :, 0], idx)                                       # B C K N
    x1, x2, x3 = conv(x, *_wb(state, prefix, "conv1", dtype)), conv(xn, *_wb(state, prefix, "conv2", dtype)), \
        conv(xn, *_wb(state, prefix, "conv3", dtype))
    x2 = np.ascontiguousarray(x2).reshape(B, -1, 1, N)                            # B kC 1 N
    w = relu(conv(relu(np.concatenate([x1, x2], 1)), *_wb(state, prefix, "conv_w.1", dtype)))
    w = np.ascontiguousarray(conv(w, *_wb(state, prefix, "conv_w.3", dtype))).reshape(B, -1, k, N)
    w = np.tile(w, (1, SHARE, 1, 1))                                              # repeat(1, share_planes, 1, 1)
    assert w.shape == x3.shape
    out = np.zeros((B, w.shape[1], 1, N), dtype)
    for j in range(k):                                                            # torch.sum(dim=2), one term at a time
        out[:, :, 0] += w[:, :, j] * x3[:, :, j]
    out = conv(relu(out), *_wb(state, prefix, "conv_out", dtype)) + identity
    assert out.dtype == dtype
    return out


def sk_sa_module(state, prefix, x, idxs, dtype=np.float64):
    """SK_SA_module.forward (vrcnet.py:161-188): the softmax over the branches is evaluated even for one branch."""
    feas = np.stack([relu(sa_module(state, f"{prefix}sams.{i}.", x, idx, dtype)) for i, idx in enumerate(idxs)], 1)
    fea_s = feas.sum(1).mean(-1).mean(-1)
    W, b = _wb(state, prefix, "fc", dtype)
    fea_z = rows_times(fea_s, W) + b
    vec = np.stack([rows_times(fea_z, _wb(state, prefix, f"fcs.{i}", dtype)[0]) + _wb(state, prefix, f"fcs.{i}", dtype)[1]
                    for i in range(len(idxs))], 1)
    e = np.exp(vec - vec.max(1, keepdims=True))
    att = e / e.sum(1, keepdims=True)
    out = (feas * att[:, :, :, None, None]).sum(1)
    assert out.dtype == dtype
    return out


def skn_res_unit(state, prefix, feat, idxs, dtype=np.float64):
    """SKN_Res_unit.forward (vrcnet.py:221-224); the number of SK_SA_modules is read off the state."""
    feat = np.asarray(feat, dtype=dtype)
    x = conv(feat, *_wb(state, prefix, "conv1", dtype))
    layer = 0
    while f"{prefix}sam.{layer}.fc.weight" in state:
        x = sk_sa_module(state, f"{prefix}sam.{layer}.", x, idxs, dtype)
        layer += 1
    assert layer >= 1
    return conv(relu(x), *_wb(state, prefix, "conv2", dtype)) + conv(feat, *_wb(state, prefix, "conv_res", dtype))


def encoder(state, features, dec, knn_list, pk, pts_num=PTS_NUM, dtype=np.float64, prefix="decoder.encoder.", rows_of=None):
    """SA_SKN_Res_encoder.forward (vrcnet.py:303-362): features[B,Cin,N], coordinates in channels 0..2 -> [B,out,N].  `rows_of`,
    when a dict, receives the points every k-NN list was computed from under the list's name."""
    features = np.asarray(features, dtype=dtype)
    B = features.shape[0]
    pts = [np.ascontiguousarray(np.swapaxes(features[:, 0:3], 1, 2))]
    c4 = lambda n, t: conv(t, *_wb(state, prefix, n, dtype))

    def lists(level):
        p = pts[-1]
        if rows_of is not None:
            rows_of.update({f"knn{level}_{i}": p for i in range(len(knn_list))})
        return [dec(f"knn{level}_{i}", lambda k=k: nearest(p, p, k)) for i, k in enumerate(knn_list)]

    def pool(level, feat):
        p, S = pts[-1], pts_num[level]
        p_idx = dec(f"fps{level}", lambda: np.stack([_fps(q, S, dtype) for q in p]))
        centres = np.ascontiguousarray(np.swapaxes(take(np.swapaxes(p, 1, 2), p_idx), 1, 2))
        pn_idx = dec(f"knn_pt{level}", lambda: nearest(centres, p, min(pk, p.shape[1])))
        net, out = eh.edge_preserve_sampling(feat[:, :, 0], p, p_idx, pn_idx)
        pts.append(out)
        return net[:, :, None, :]

    def up(i, feat, target, source):
        idx = dec(f"three_nn{i}", lambda: nearest(target, source, 3))
        return eh.three_interpolate(feat[:, :, 0], idx, eh.three_nn_weights(target, source, idx))[:, :, None, :]

    x = features[:, :, None, :]
    x1 = relu(skn_res_unit(state, prefix + "sam_res1.", x, lists(1), dtype))
    x = pool(1, x1)
    x2 = relu(skn_res_unit(state, prefix + "sam_res2.", x, lists(2), dtype))
    x = pool(2, x2)
    x3 = relu(skn_res_unit(state, prefix + "sam_res3.", x, lists(3), dtype))
    x = pool(3, x3)
    x4 = relu(skn_res_unit(state, prefix + "sam_res4.", x, lists(4), dtype))
    g = c4("conv5", x4).max(-1).reshape(B, -1)
    W, b = _wb(state, prefix, "fc1", dtype)
    g = relu(rows_times(g, W) + b)
    W, b = _wb(state, prefix, "fc2", dtype)
    g = relu(rows_times(g, W) + b)
    g = np.repeat(g[:, :, None], pts_num[3], axis=2)[:, :, None, :]
    x = relu(c4("conv6", np.concatenate([g, x4], 1)))
    x = up(1, x, pts[2], pts[3])
    x = relu(c4("conv7", np.concatenate([x, x3], 1)))
    x = up(2, x, pts[1], pts[2])
    x = relu(c4("conv8", np.concatenate([x, x2], 1)))
    x = up(3, x, pts[0], pts[1])
    x = relu(c4("conv9", np.concatenate([x, x1], 1)))
    out = c4("conv_out", x)[:, :, 0]
    assert out.dtype == dtype
    return out


def folding(point_feat, global_feat, W, b, step_ratio, dtype=np.float64):
    """Folding.forward (vrcnet.py:101-113) as written: point_feat[B,F,n], global_feat[B,G] -> [B,out,n*step_ratio]; the grid is the
    reference's float32 one."""
    point_feat, global_feat, W, b = (np.asarray(a, dtype=dtype) for a in (point_feat, global_feat, W, b))
    B, F, n = point_feat.shape
    grid = pcn_host.gen_grid_up(step_ratio, 0.2, dtype)                           # [2, step]
    pf = np.repeat(np.swapaxes(point_feat, 1, 2)[:, :, None, :], step_ratio, axis=2).reshape(B, -1, F)
    pf = np.ascontiguousarray(np.swapaxes(pf, 1, 2))
    gf = np.repeat(global_feat[:, :, None], n * step_ratio, axis=2)
    grid_feat = np.tile(grid[None], (B, 1, n))
    out = relu(conv(np.concatenate([gf, pf, grid_feat], 1), W, b))
    assert out.dtype == dtype
    return out


def pcn_encoder(state, x, dtype=np.float64, prefix="encoder."):
    """PCN_encoder.forward (pcn.py:20-29): x[B,3,N] -> [B,1024]; pcn_host.encoder with float64 products through matmul."""
    c1 = lambda n, t: conv(t, *_wb(state, prefix, n, dtype))
    x = np.asarray(x, dtype=dtype)
    x = c1("conv2", relu(c1("conv1", x)))
    x = np.concatenate([x, np.repeat(x.max(2)[:, :, None], x.shape[2], axis=2)], 1)
    return c1("conv4", relu(c1("conv3", x))).max(2)


def linear_resblock(state, prefix, feature, dtype=np.float64):
    """Linear_ResBlock.forward (vrcnet.py:125-127): its ReLU is in place, so conv_res sees relu(feature) too."""
    lin = lambda n, t: rows_times(t, _wb(state, prefix, n, dtype)[0]) + _wb(state, prefix, n, dtype)[1]
    r = relu(np.asarray(feature, dtype=dtype))
    return lin("conv2", relu(lin("conv1", r))) + lin("conv_res", r)


def softplus(s):
    return np.where(s > 20, s, np.log1p(np.exp(np.minimum(s, 20)))).astype(s.dtype)


def decoder(state, c, global_feat, x, dec, dtype=np.float64, features=None):
    """MSAP_SKN_decoder.forward (vrcnet.py:439-507): -> coarse_raw, coarse_high, coarse, fine, all [B,3,.].  `features`, when a
    dict, receives the rows (points or features) every k-NN decision was computed from under the decision's name."""
    p = "decoder."
    lin = lambda n, t: rows_times(t, _wb(state, p, n, dtype)[0]) + _wb(state, p, n, dtype)[1]
    c1 = lambda n, t: conv(t, *_wb(state, p, n, dtype))
    global_feat, x = np.asarray(global_feat, dtype=dtype), np.asarray(x, dtype=dtype)
    B = x.shape[0]
    coarse_raw = lin("fc3", relu(lin("fc2", relu(lin("fc1", global_feat))))).reshape(B, 3, c.num_coarse_raw)
    coarse_input, org = coarse_raw, x
    if c.points_label:
        coarse_input = np.concatenate([coarse_raw, np.zeros((B, 1, c.num_coarse_raw), dtype)], 1)
        org = np.concatenate([x, np.ones((B, 1, x.shape[2]), dtype)], 1)
    points = np.concatenate([coarse_input, org], 2)
    dense = encoder(state, points, dec, c.knn_list, c.pk, PTS_NUM, dtype, rows_of=features)

    def expansion(name, prefix, t, step):
        rows = np.ascontiguousarray(np.swapaxes(t, 1, 2))
        if features is not None:
            features[name] = rows
        idx = dec(name, lambda: nearest(rows, rows, 4))
        w = [a for n in ("conv1", "conv2", "conv3") for a in _wb(state, prefix, n, dtype)]
        return eh.ef_expansion(t, idx, *w, step, dtype)

    if c.up_scale >= 2:
        dense = expansion("knn_exp1", p + "expansion1.", dense, c.up_scale)
    feats = relu(c1("conv_cup1", dense))
    coarse_high = c1("conv_cup2", feats)
    coarse = coarse_high
    if coarse.shape[2] > c.num_fps:
        rows = np.swapaxes(coarse_high, 1, 2)
        idx = dec("fps_out", lambda: np.stack([_fps(q, c.num_fps, dtype) for q in rows]))
        coarse, feats = take(coarse_high, idx), take(feats, idx)
    if coarse.shape[2] > c.num_coarse:
        s = softplus(c1("conv_s3", relu(c1("conv_s2", relu(c1("conv_s1", feats))))))
        idx = dec("topk", lambda: np.argsort(-s[:, 0], axis=-1, kind="stable")[:, :c.num_coarse])
        coarse, feats = take(coarse, idx), take(feats, idx)
    if coarse.shape[2] < c.num_points:
        step = c.num_points // c.num_coarse
        if c.local_folding:
            up = folding(feats, global_feat, *_wb(state, p, "expansion2.conv", dtype), step, dtype)
            centre = np.repeat(np.swapaxes(coarse, 1, 2)[:, :, None, :], step, axis=2).reshape(B, c.num_points, 3)
            fine = c1("conv_f2", relu(c1("conv_f1", up))) + np.swapaxes(centre, 1, 2)
        else:
            up = expansion("knn_exp2", p + "expansion2.", feats, step)
            fine = c1("conv_f2", relu(c1("conv_f1", up)))
    else:
        assert coarse.shape[2] == c.num_points
        fine = coarse
    return coarse_raw, coarse_high, coarse, fine


STAGES = ("feat", "coarse_raw", "coarse_high", "coarse", "fine")


def model(state, x, c, z, dtype=np.float64, decisions=None, features=None):
    """Model.forward's tensors under "test" (vrcnet.py:595-611) with the latent sample z[B,size_z] given -> (dict(feat[B,1024],
    coarse_raw, coarse_high, coarse, fine as rows [B,.,3]), the decisions used).  `feat` is the PCN encoder's output;
    posterior_infer1's in-place ReLU rectifies it before the generator's output is added."""
    dec = eh._Decisions(decisions)
    feat = pcn_encoder(state, x, dtype)
    gen = linear_resblock(state, "generator.", np.asarray(z, dtype=dtype), dtype)
    outs = decoder(state, c, relu(feat) + gen, x, dec, dtype, features)
    res = dict(feat=feat, **{n: np.ascontiguousarray(np.swapaxes(t, 1, 2)) for n, t in zip(STAGES[1:], outs)})
    assert all(v.dtype == dtype for v in res.values())
    return res, dec.used


def posterior(state, x, dtype=np.float64):
    """(q_mu, softplus(q_std)) of Model.forward's posterior (vrcnet.py:596-598)."""
    feat = pcn_encoder(state, x, dtype)
    o = linear_resblock(state, "posterior_infer2.", linear_resblock(state, "posterior_infer1.", feat, dtype), dtype)
    h = o.shape[1] // 2
    return o[:, :h], softplus(o[:, h:])
