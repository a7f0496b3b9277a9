"""Deterministic ECG weights shared by tests/golden/make_golden_ecg.py (which loads them into the REFERENCE model), the tests
(which load them into houv_amd.models.ecg.Model and into the NumPy restatement tests/ecg_host.py) and scripts/perf_ecg.py: the
repository ships no trained ECG checkpoint.  Names/shapes = the reference's state_dict (completion/models/ecg.py) for the given
num_coarse and scale = ceil(num_points / (num_coarse + num_input)).

As in pcn_weights.py the scale matters: torch's default initialisation leaves |out2| <= 0.13, mostly bias.  Every weight is
uniform(-1, 1) * g / sqrt(fan_in) with g = GAIN_FIRST on the two 3-input convolutions and GAIN elsewhere, biases uniform(-0.1,
0.1): activations stay O(1) through the network.  Changing a constant here means regenerating g26_ecg.npz."""
import numpy as np

GAIN_FIRST, GAIN = 4.0, 2.0
SEED = 2026
G, INIT = 24, 24


def _conv(name, n_out, n_in, dims):
    return [(name + ".weight", (n_out, n_in) + (1,) * dims), (name + ".bias", (n_out,))]


def _dense(prefix, c):
    return (_conv(prefix + ".first_conv", G, 2 * c, 2) + _conv(prefix + ".model.stack_conv_1.model.conv", G, c + G, 2)
            + _conv(prefix + ".model.stack_conv_2.model.conv", G, c + 2 * G, 2))


def spec(num_coarse, scale=1):
    c1 = 2 * INIT + 3 * G
    c2 = 2 * c1 + 2 * G + 3 * G
    c3 = 2 * c2 + 2 * G + 3 * G
    c4 = 2 * c3 + 2 * G + 3 * G
    e = "decoder.encoder."
    s = (_conv("encoder.conv1", 128, 3, 1) + _conv("encoder.conv2", 256, 128, 1) + _conv("encoder.conv3", 512, 512, 1)
         + _conv("encoder.conv4", 1024, 512, 1)
         + _conv("decoder.fc1", 1024, 1024, 0) + _conv("decoder.fc2", 1024, 1024, 0) + _conv("decoder.fc3", num_coarse * 3, 1024, 0)
         + _conv(e + "conv1", INIT, 3, 1) + _dense(e + "dense_conv1", INIT)
         + _conv(e + "conv2", 2 * G, 2 * c1, 1) + _dense(e + "dense_conv2", 2 * G)
         + _conv(e + "conv3", 2 * G, 2 * c2, 1) + _dense(e + "dense_conv3", 2 * G)
         + _conv(e + "conv4", 2 * G, 2 * c3, 1) + _dense(e + "dense_conv4", 2 * G)
         + _conv(e + "gf_conv", 1024, c4, 1) + _conv(e + "fc1", 512, 1024, 0) + _conv(e + "fc2", 1024, 512, 0)
         + _conv(e + "conv5", 1024, c4 + 1024, 1) + _conv(e + "conv6", 768, c3 + 1024, 1) + _conv(e + "conv7", 512, c2 + 768, 1)
         + _conv(e + "conv8", 256, c1 + 512, 1))
    if scale >= 2:
        s += (_conv("decoder.expansion.conv1", 64, 512, 2) + _conv("decoder.expansion.conv2", 64 * scale, 512 + 64, 2)
              + _conv("decoder.expansion.conv3", 64, 64, 2) + _conv("decoder.conv1", 64, 64, 1))
    else:
        s += _conv("decoder.conv1", 64, 256, 1)
    return s + _conv("decoder.conv2", 3, 64, 1)


def make_state(num_coarse, scale=1, seed=SEED, gain_first=GAIN_FIRST, gain=GAIN):
    rng = np.random.default_rng(seed + num_coarse + 100000 * scale)
    st = {}
    for name, shape in spec(num_coarse, scale):
        if name.endswith("bias"):
            v = rng.uniform(-0.1, 0.1, shape)
        else:
            g = gain_first if shape[1] == 3 else gain
            v = rng.uniform(-1, 1, shape) * g / np.sqrt(shape[1])
        st[name] = v.astype(np.float32)
    return st


class Args:
    """The options models/ecg.py reads (cfgs/ecg_mi355x.yaml's keys)."""
    num_points, loss, eval_emd, batch_size = 2048, "cd", False, 32


def args(num_points, **kw):
    return type("Args", (Args,), dict(num_points=num_points, **kw))
