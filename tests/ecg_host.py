"""NumPy restatement of the ECG completion network (completion/models/ecg.py, completion/model_utils.py) in the REFERENCE's
materialising form -- channel-major [B, C, N] activations, the [B, 2C, N, k] edge tensor, `repeat` + `cat` of the centre and of the
global feature -- parametrised by dtype, so that what the kernels fuse away (houv_dense_conv) and the splits the model relies on
are tested, not assumed.

Every discrete decision (furthest-point samples, k-NN lists, three-NN lists) can be INJECTED: `decisions` maps the names
fps1..3, knn_pt1..3, knn_feat1..4, knn_exp, three_nn1..3, fps_out to index arrays, and whatever is missing is computed here
(direct squared distances, stable sort: the lower index first among equals).  The decisions that were used are always
returned.  Given the decisions the network is a continuous function of its input, which is what a tolerance can be set for.

float32 products are summed over k ascending, one product and one addition per term (pcn_host.rows_times: the same spread on
every host); float64, the yardstick, uses matmul."""
import numpy as np

import pcn_host
from pointops_host import fps as _fps

G = 24          # growth rate of every Dense_conv in ECG
DENSE_K = 16    # neighbours of Dense_conv and of edge_preserve_sampling in EF_encoder
HIERARCHY = (1024, 256, 64)
DECISIONS = ("fps1", "knn_pt1", "fps2", "knn_pt2", "fps3", "knn_pt3", "knn_feat1", "knn_feat2", "knn_feat3", "knn_feat4",
             "three_nn1", "three_nn2", "three_nn3", "knn_exp", "fps_out")
relu = pcn_host.relu


def rows_times(x, W):
    """x[..., K] . W[C, K]^T -> [..., C]."""
    if x.dtype == np.float64:
        return x @ W.T
    return pcn_host.rows_times(x, W)


def conv(x, W, b):
    """A 1x1 convolution over axis 1 of x[B,Cin,...]: W[Cout,Cin] (trailing unit axes of a Conv1d / Conv2d weight dropped),
    b[Cout] added after the sum."""
    W = W.reshape(W.shape[0], -1)
    y = rows_times(np.ascontiguousarray(np.moveaxis(x, 1, -1)), W) + b
    return np.ascontiguousarray(np.moveaxis(y, -1, 1))


def sqdist_rows(a, b):
    """a[B,N,C], b[B,M,C] -> [B,N,M] direct squared distances, channel by channel (no [B,N,M,C] tensor)."""
    d = np.zeros(a.shape[:2] + (b.shape[1],), a.dtype)
    for c in range(a.shape[2]):
        t = b[:, None, :, c] - a[:, :, None, c]
        d += t * t
    return d


def nearest(a, b, k):
    """The k nearest rows of b for every row of a, nearest first, the lower index first among equals: [B,N,k] int64."""
    return np.argsort(sqdist_rows(a, b), axis=-1, kind="stable")[..., :k]


class _Decisions:
    def __init__(self, given):
        self.given = {} if given is None else given
        self.used = {}

    def __call__(self, name, compute):
        v = self.given[name] if name in self.given else compute()
        self.used[name] = np.asarray(v).astype(np.int64)
        return self.used[name]


def take(x, idx):
    """x[B,C,N], idx[B,...] -> [B,C,...] = x[b,:,idx[b,...]]."""
    B, C, _ = x.shape
    flat = idx.reshape(B, 1, -1)
    return np.take_along_axis(x, np.broadcast_to(flat, (B, C, flat.shape[2])), axis=2).reshape((B, C) + idx.shape[1:])


def get_graph_feature(x, idx, minus_center=True):
    """model_utils.py:164-187 given the k-NN lists: x[B,C,N], idx[B,N,k] -> [B,2C,N,k] = cat(x_i, x_j - x_i) (or x_j)."""
    k = idx.shape[2]
    feature = np.moveaxis(take(x, idx), 1, 3)                                   # [B,N,k,C]
    centre = np.repeat(np.swapaxes(x, 1, 2)[:, :, None, :], k, axis=2)
    cat = np.concatenate([centre, feature - centre if minus_center else feature], axis=3)
    return np.ascontiguousarray(np.transpose(cat, (0, 3, 1, 2)))


def dense_conv(x, idx, W0, b0, W1, b1, W2, b2, dtype=np.float64):
    """ecg.py:58-65 as written: x[B,C,N] -> [B,C+72,N]; the contract of houv_dense_conv (relu_out = 0) in channel-major form."""
    x, W0, b0, W1, b1, W2, b2 = (np.asarray(a, dtype=dtype) for a in (x, W0, b0, W1, b1, W2, b2))
    k = idx.shape[2]
    y = relu(conv(get_graph_feature(x, idx), W0, b0))
    y = np.concatenate([y, np.repeat(x[:, :, :, None], k, axis=3)], 1)
    y = np.concatenate([y, relu(conv(y, W1, b1))], 1)                   # Stack_conv: cat((x, act(conv(x))), 1)
    y = np.concatenate([y, conv(y, W2, b2)], 1)                         # the last one has no activation
    assert y.dtype == dtype
    return y.max(3)


def edge_preserve_sampling(feature, points, p_idx, pn_idx):
    """model_utils.py:90-116 given the samples p_idx[B,S] and their neighbour lists pn_idx[B,S,pk]: feature[B,C,N],
    points[B,N,3] -> (net[B,2C,S], point_output[B,S,3])."""
    point_output = np.swapaxes(take(np.swapaxes(points, 1, 2), p_idx), 1, 2)
    return np.concatenate([take(feature, p_idx), take(feature, pn_idx).max(3)], 1), np.ascontiguousarray(point_output)


def three_nn_weights(target, source, idx):
    """three_nn_upsampling (model_utils.py:307-314) given the lists: the L2 distances of the listed points, clamped at 1e-10,
    inverted and normalised."""
    nb = np.moveaxis(take(np.swapaxes(source, 1, 2), idx), 1, 3)                # [B,N,3,3]
    d = nb - target[:, :, None, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    inv = 1 / np.maximum(dist, target.dtype.type(1e-10))
    return inv / inv.sum(2, keepdims=True)


def three_interpolate(features, idx, weight):
    f = take(features, idx)                                                     # [B,C,N,3]
    w = weight[:, None]
    return (w[..., 0] * f[..., 0] + w[..., 1] * f[..., 1]) + w[..., 2] * f[..., 2]


def ef_expansion(x, idx, W1, b1, W2, b2, W3, b3, step_ratio, dtype=np.float64):
    """EF_expansion.forward (model_utils.py:37-55) given the k-NN lists: x[B,C,N] -> [B,64,N*step_ratio]."""
    x, W1, b1, W2, b2, W3, b3 = (np.asarray(a, dtype=dtype) for a in (x, W1, b1, W2, b2, W3, b3))
    B, _, N = x.shape
    k = idx.shape[2]
    f = np.ascontiguousarray(np.transpose(get_graph_feature(x, idx, minus_center=False), (0, 1, 3, 2)))    # B C K N
    e = relu(np.concatenate([conv(f, W1, b1), f], 1))
    e = relu(conv(e, W2, b2))
    out_size = W3.shape[0]
    e = np.ascontiguousarray(np.transpose(e, (0, 2, 3, 1))).reshape(B, k, N * step_ratio, out_size)       # the reinterpretation
    e = conv(np.ascontiguousarray(np.transpose(e, (0, 3, 1, 2))), W3, b3)
    assert e.dtype == dtype
    return e.max(2)


def _params(state, prefix, dtype):
    w = lambda n: np.asarray(state[prefix + n + ".weight"], dtype=dtype)
    b = lambda n: np.asarray(state[prefix + n + ".bias"], dtype=dtype)
    return w, b


def _dense(state, prefix, x, idx, dtype):
    w, b = _params(state, prefix, dtype)
    return dense_conv(x, idx, w("first_conv"), b("first_conv"), w("model.stack_conv_1.model.conv"), b("model.stack_conv_1.model.conv"),
                      w("model.stack_conv_2.model.conv"), b("model.stack_conv_2.model.conv"), dtype)


def ef_encoder(state, x, dec, dtype=np.float64, prefix="decoder.encoder.", features=None):
    """EF_encoder.forward (ecg.py:114-159): x[B,3,N] -> [B,256,N].  `features`, when a dict, receives the input of every
    feature-space k-NN under its decision's name."""
    w, b = _params(state, prefix, dtype)
    c1 = lambda n, t: conv(t, w(n), b(n))
    x = np.asarray(x, dtype=dtype)
    pc = [np.ascontiguousarray(np.swapaxes(x[:, 0:3], 1, 2))]
    rows = lambda t: np.swapaxes(t, 1, 2)

    def knn_feat(name, t):
        if features is not None:
            features[name] = np.ascontiguousarray(rows(t))
        return dec(name, lambda: nearest(rows(t), rows(t), min(DENSE_K, t.shape[2])))

    def sample(i, feat):
        p = pc[-1]
        p_idx = dec(f"fps{i}", lambda: np.stack([_fps(q, HIERARCHY[i - 1], dtype) for q in p]))
        centres = np.ascontiguousarray(np.swapaxes(take(np.swapaxes(p, 1, 2), p_idx), 1, 2))
        pn_idx = dec(f"knn_pt{i}", lambda: nearest(centres, p, min(DENSE_K, p.shape[1])))
        net, out = edge_preserve_sampling(feat, p, p_idx, pn_idx)
        pc.append(out)
        return net

    x0 = relu(c1("conv1", x))
    x1 = relu(_dense(state, prefix + "dense_conv1.", x0, knn_feat("knn_feat1", x0), dtype))
    x1 = np.concatenate([x1, x0], 1)
    x1d = sample(1, x1)
    x2 = relu(c1("conv2", x1d))
    x2 = relu(_dense(state, prefix + "dense_conv2.", x2, knn_feat("knn_feat2", x2), dtype))
    x2 = np.concatenate([x2, x1d], 1)
    x2d = sample(2, x2)
    x3 = relu(c1("conv3", x2d))
    x3 = relu(_dense(state, prefix + "dense_conv3.", x3, knn_feat("knn_feat3", x3), dtype))
    x3 = np.concatenate([x3, x2d], 1)
    x3d = sample(3, x3)
    x4 = relu(c1("conv4", x3d))
    x4 = relu(_dense(state, prefix + "dense_conv4.", x4, knn_feat("knn_feat4", x4), dtype))
    x4 = np.concatenate([x4, x3d], 1)

    g = c1("gf_conv", x4).max(-1)
    g = relu(rows_times(g, w("fc1")) + b("fc1"))
    g = relu(rows_times(g, w("fc2")) + b("fc2"))
    x4 = np.concatenate([np.repeat(g[:, :, None], x4.shape[2], axis=2), x4], 1)
    x4 = relu(c1("conv5", x4))

    def up(i, feat, target, source):
        idx = dec(f"three_nn{i}", lambda: nearest(target, source, 3))
        return three_interpolate(feat, idx, three_nn_weights(target, source, idx))

    x4 = up(1, x4, pc[2], pc[3])
    x3 = relu(c1("conv6", np.concatenate([x3, x4], 1)))
    x3 = up(2, x3, pc[1], pc[2])
    x2 = relu(c1("conv7", np.concatenate([x2, x3], 1)))
    x2 = up(3, x2, pc[0], pc[1])
    out = c1("conv8", np.concatenate([x1, x2], 1))
    assert out.dtype == dtype
    return out


def ecg_decoder(state, feat, x, num_coarse, num_fine, dec, dtype=np.float64, features=None):
    """ECG_decoder.forward (ecg.py:190-210): feat[B,1024], x[B,3,num_input] -> (coarse[B,3,nc], fine[B,3,num_fine or fewer])."""
    w, b = _params(state, "decoder.", dtype)
    feat, x = np.asarray(feat, dtype=dtype), np.asarray(x, dtype=dtype)
    B = feat.shape[0]
    scale = int(np.ceil(num_fine / (num_coarse + x.shape[2])))
    c = relu(rows_times(feat, w("fc1")) + b("fc1"))
    c = relu(rows_times(c, w("fc2")) + b("fc2"))
    coarse = (rows_times(c, w("fc3")) + b("fc3")).reshape(B, 3, num_coarse)
    dense = ef_encoder(state, np.concatenate([coarse, x], 2), dec, dtype, features=features)
    if scale >= 2:
        rows = np.ascontiguousarray(np.swapaxes(dense, 1, 2))
        if features is not None:
            features["knn_exp"] = rows
        idx = dec("knn_exp", lambda: nearest(rows, rows, 4))
        dense = ef_expansion(dense, idx, w("expansion.conv1"), b("expansion.conv1"), w("expansion.conv2"), b("expansion.conv2"),
                             w("expansion.conv3"), b("expansion.conv3"), scale, dtype)
    fine = conv(relu(conv(dense, w("conv1"), b("conv1"))), w("conv2"), b("conv2"))
    if fine.shape[2] > num_fine:
        pts = np.swapaxes(fine, 1, 2)
        fine = take(fine, dec("fps_out", lambda: np.stack([_fps(q, num_fine, dtype) for q in pts])))
    return coarse, fine


def model(state, x, num_points, num_coarse, dtype=np.float64, decisions=None, features=None):
    """Model.forward's tensors (ecg.py:226-229) -> (dict(feat[B,1024], out1[B,nc,3], out2[B,num_points,3]), the decisions used)."""
    dec = _Decisions(decisions)
    feat = pcn_host.encoder(state, x, dtype)
    coarse, fine = ecg_decoder(state, feat, x, num_coarse, num_points, dec, dtype, features)
    res = dict(feat=feat, out1=np.ascontiguousarray(np.swapaxes(coarse, 1, 2)), out2=np.ascontiguousarray(np.swapaxes(fine, 1, 2)))
    assert all(v.dtype == dtype for v in res.values())
    return res, dec.used
