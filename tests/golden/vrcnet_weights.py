"""Deterministic VRCNet weights shared by tests/golden/make_golden_vrcnet.py (which loads them into the REFERENCE modules), the
tests (which load them into houv_amd.models.vrcnet and into the NumPy restatement tests/vrcnet_host.py) and
scripts/perf_vrcnet.py: the repository ships no trained VRCNet checkpoint.  Names / shapes / order = the reference's state_dict
(completion/models/vrcnet.py) for the given options.

As in ecg_weights.py every weight is uniform(-1, 1) * g / sqrt(fan_in), biases uniform(-0.1, 0.1), with g = GAIN_FIRST on the
convolutions of 3 or 4 input channels and GAIN elsewhere, so activations stay O(1) through the network.  Inside an SA_module the
attention weights are a sum over k neighbours on top of that: conv_w's second convolution and conv_out take GAIN_ATT, which
leaves the attention branch and the residual of comparable size (the generator asserts the ratio): a block whose output is all
identity would test nothing.  The attention branch is bilinear in the features, so a stack of blocks blows up once activations
pass 1 (GAIN throughout gives |fine| ~ 1e5): the other convolutions of the SKN_Res_units take GAIN_UNIT, and decoder.fc3 takes
GAIN_RAW so that coarse_raw has the size of the input points it is concatenated with.  Changing a constant here means regenerating g27_vrcnet.npz."""
import numpy as np

GAIN_FIRST, GAIN, GAIN_ATT, GAIN_UNIT, GAIN_RAW = 4.0, 2.0, 1.0, 1.6, 0.5
SEED = 2027


def _conv(name, n_out, n_in, dims, bias=True):
    return [(name + ".weight", (n_out, n_in) + (1,) * dims)] + ([(name + ".bias", (n_out,))] if bias else [])


def sa_spec(p, C, k):
    rel, mid, m = C // 16, C // 4, C // 32
    return (_conv(p + "conv1", rel, C, 2) + _conv(p + "conv2", rel, C, 2) + _conv(p + "conv3", mid, C, 2)
            + _conv(p + "conv_w.1", m, rel * (k + 1), 2, bias=False) + _conv(p + "conv_w.3", k * m, m, 2) + _conv(p + "conv_out", C, mid, 2))


def sk_spec(p, C, ks):
    d = max(C // 2, 32)
    s = []
    for i, k in enumerate(ks):
        s += sa_spec(f"{p}sams.{i}.", C, k)
    s += _conv(p + "fc", d, C, 0)
    for i in range(len(ks)):
        s += _conv(f"{p}fcs.{i}", C, d, 0)
    return s


def unit_spec(p, c_in, c_out, ks, layers):
    s = _conv(p + "conv1", c_out, c_in, 2, bias=False)
    for layer in range(layers):
        s += sk_spec(f"{p}sam.{layer}.", c_out, ks)
    return s + _conv(p + "conv2", c_out, c_out, 2, bias=False) + _conv(p + "conv_res", c_out, c_in, 2, bias=False)


def encoder_spec(p, c_in, ks, layers, c_out):
    return (unit_spec(p + "sam_res1.", c_in, 64, ks, layers[0]) + unit_spec(p + "sam_res2.", 128, 128, ks, layers[1])
            + unit_spec(p + "sam_res3.", 256, 256, ks, layers[2]) + unit_spec(p + "sam_res4.", 512, 512, ks, layers[3])
            + _conv(p + "conv5", 1024, 512, 2) + _conv(p + "fc1", 512, 1024, 0) + _conv(p + "fc2", 1024, 512, 0)
            + _conv(p + "conv6", 512, 512 + 1024, 2) + _conv(p + "conv7", 256, 256 + 512, 2) + _conv(p + "conv8", 128, 128 + 256, 2)
            + _conv(p + "conv9", 64, 64 + 128, 2) + _conv(p + "conv_out", c_out, 64, 2))


def _resblock(p, n_in, n_out):
    return _conv(p + "conv1", n_in, n_in, 0) + _conv(p + "conv2", n_out, n_in, 0) + _conv(p + "conv_res", n_out, n_in, 0)


def _expansion(p, n_in, n_out, step):
    return _conv(p + "conv1", n_out, 2 * n_in, 2) + _conv(p + "conv2", n_out * step, 2 * n_in + n_out, 2) + _conv(p + "conv3", n_out, n_out, 2)


def spec(c, size_z=128):
    """c: vrcnet_host.cfg(...)."""
    d = "decoder."
    s = (_conv("encoder.conv1", 128, 3, 1) + _conv("encoder.conv2", 256, 128, 1) + _conv("encoder.conv3", 512, 512, 1)
         + _conv("encoder.conv4", 1024, 512, 1) + _resblock("posterior_infer1.", 1024, 1024) + _resblock("posterior_infer2.", 1024, 2 * size_z)
         + _resblock("prior_infer.", 1024, 2 * size_z) + _resblock("generator.", size_z, 1024)
         + _conv(d + "fc1", 1024, 1024, 0) + _conv(d + "fc2", 1024, 1024, 0) + _conv(d + "fc3", c.num_coarse_raw * 3, 1024, 0)
         + encoder_spec(d + "encoder.", 4 if c.points_label else 3, c.knn_list, c.layers, 256))
    if c.up_scale >= 2:
        s += _expansion(d + "expansion1.", 256, 64, c.up_scale) + _conv(d + "conv_cup1", 64, 64, 1)
    else:
        s += _conv(d + "conv_cup1", 64, 256, 1)
    s += _conv(d + "conv_cup2", 3, 64, 1) + _conv(d + "conv_s1", 16, 64, 1) + _conv(d + "conv_s2", 8, 16, 1) + _conv(d + "conv_s3", 1, 8, 1)
    step = c.num_points // c.num_coarse
    s += _conv(d + "expansion2.conv", 256, 64 + 1024 + 2, 1) if c.local_folding else _expansion(d + "expansion2.", 64, 256, step)
    return s + _conv(d + "conv_f1", 64, 256, 1) + _conv(d + "conv_f2", 3, 64, 1)


def _in_attention(name):
    """conv_w's second convolution and conv_out of an SA_module (alone, prefix '', or under an SK_SA_module's `sams.`)."""
    in_sa = ".sams." in "." + name or name.startswith(("conv_w.", "conv_out."))
    return in_sa and ("conv_w.3." in name or "conv_out." in name)


def make_state(spec_list, seed=SEED):
    rng = np.random.default_rng(seed)
    st = {}
    for name, shape in spec_list:
        if name.endswith("bias"):
            v = rng.uniform(-0.1, 0.1, shape)
        else:
            g = (GAIN_FIRST if shape[1] in (3, 4) else GAIN_ATT if _in_attention(name) else GAIN_UNIT if "sam_res" in name
                 else GAIN_RAW if name.startswith("decoder.fc3.") else GAIN)
            v = rng.uniform(-1, 1, shape) * g / np.sqrt(shape[1])
        st[name] = v.astype(np.float32)
    return st


class Args:
    """The options models/vrcnet.py reads (cfgs/vrcnet_mi355x.yaml's keys)."""
    layers, knn_list, pk, points_label, local_folding = "1,1,1,1", "16", 10, True, True
    num_coarse_raw, num_fps, num_coarse, num_points = 1024, 2048, 2048, 2048
    distribution_loss, loss, eval_emd, batch_size = "KLD", "cd", False, 24


def args(c=None, **kw):
    """Args for a vrcnet_host.cfg (or the shipped values), with overrides."""
    d = {} if c is None else dict(layers=",".join(map(str, c.layers)), knn_list=",".join(map(str, c.knn_list)), pk=c.pk,
                                  points_label=c.points_label, local_folding=c.local_folding, num_coarse_raw=c.num_coarse_raw,
                                  num_fps=c.num_fps, num_coarse=c.num_coarse, num_points=c.num_points)
    d.update(kw)
    return type("Args", (Args,), d)
