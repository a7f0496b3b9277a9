"""Deterministic PCN weights shared by tests/golden/make_golden_pcn.py (which loads them into the REFERENCE model), the tests
(which load them into houv_amd.models.pcn.Model and into the NumPy restatement tests/pcn_host.py) and scripts/perf_pcn.py: the
repository ships no trained PCN checkpoint.  Names/shapes = the reference's state_dict (registration/models/pcn.py:12-19,
:86-100) for the given num_coarse.

The scale matters.  Under torch's default initialisation (uniform +-1/sqrt(fan_in), biases of the same size) the inputs of
+-0.5 give first-layer activations of ~0.3 beside biases of ~0.5, every later layer shrinks them by ~1/sqrt(3) again, and the
outputs are ~0.1 of mostly bias: such a fixture pins little.  Here every weight is uniform(-1, 1) * g / sqrt(fan_in) with
g = GAIN_FIRST on encoder.conv1 (3 inputs of ~0.3) and GAIN elsewhere (sqrt(3) keeps the variance of a uniform draw; ReLU halves
it, hence a little more), and the biases are uniform(-0.1, 0.1): activations stay O(1) through all eleven layers and a pooled
feature is a maximum of data, not a bias.  Changing a constant here means regenerating g25_pcn.npz."""
import numpy as np

GAIN_FIRST, GAIN = 4.0, 2.0
SEED = 2025


def spec(num_coarse):
    return [("encoder.conv1.weight", (128, 3, 1)), ("encoder.conv1.bias", (128,)),
            ("encoder.conv2.weight", (256, 128, 1)), ("encoder.conv2.bias", (256,)),
            ("encoder.conv3.weight", (512, 512, 1)), ("encoder.conv3.bias", (512,)),
            ("encoder.conv4.weight", (1024, 512, 1)), ("encoder.conv4.bias", (1024,)),
            ("decoder.fc1.weight", (1024, 1024)), ("decoder.fc1.bias", (1024,)),
            ("decoder.fc2.weight", (1024, 1024)), ("decoder.fc2.bias", (1024,)),
            ("decoder.fc3.weight", (num_coarse * 3, 1024)), ("decoder.fc3.bias", (num_coarse * 3,)),
            ("decoder.conv1.weight", (512, 1029, 1)), ("decoder.conv1.bias", (512,)),
            ("decoder.conv2.weight", (512, 512, 1)), ("decoder.conv2.bias", (512,)),
            ("decoder.conv3.weight", (3, 512, 1)), ("decoder.conv3.bias", (3,))]


def make_state(num_coarse, seed=SEED, gain_first=GAIN_FIRST, gain=GAIN):
    rng = np.random.default_rng(seed + num_coarse)
    st = {}
    for name, shape in spec(num_coarse):
        if name.endswith("bias"):
            v = rng.uniform(-0.1, 0.1, shape)
        else:
            g = gain_first if name == "encoder.conv1.weight" else gain
            v = rng.uniform(-1, 1, shape) * g / np.sqrt(shape[1])
        st[name] = v.astype(np.float32)
    return st


class Args:
    """The options models/pcn.py reads (cfgs/pcn_mi355x.yaml's keys)."""
    num_points, loss, eval_emd, batch_size = 2048, "cd", False, 32


def args(num_points):
    return type("Args", (Args,), dict(num_points=num_points))
