"""Deterministic IDAM weights shared by tests/golden/make_golden_idam.py (which loads them into the REFERENCE model), the tests
(which load them into houv_amd.models.idam.Model and into the NumPy restatement tests/idam_host.py) and scripts/perf_idam.py:
the repository ships no trained IDAM checkpoint.  Names/shapes = the reference's state_dict
(registration/models/idam.py:115-201) for descriptor_size 64, num_iters 3, no FPFH.

The scale matters.  Under torch's default initialisation the model is degenerate: neighbour differences are ~0.02, the biases
dominate, the significance scores of a cloud span ~5e-7 and the kept sets differ between a float32 and a float64 run of the
same weights.  Here every weight is uniform(-1, 1) * g / sqrt(fan_in) with g = GAIN_FIRST on the first Propagate convolution
(whose inputs are the small coordinate differences), GAIN_SIM on the similarity layers (their inputs are the embeddings, which
span about +-100: at 2.5 nearly every row of scores of a small cloud clamps at +-20), GAIN_W on weight_fc (at 2.5 the float32
sigmoid saturates to exactly 1 on many rows and `w >= median` keeps another set than in float64) and GAIN elsewhere, biases are
uniform(-0.1, 0.1), and the BatchNorm statistics are randomised so that eval-mode BatchNorm is not the identity.
make_golden_idam.py asserts the conditions under which the fixture pins the model and not noise; changing a constant here means
regenerating g24_idam.npz."""
import numpy as np

DESCRIPTOR_SIZE, NUM_ITERS = 64, 3
GAIN_FIRST, GAIN, GAIN_SIM, GAIN_W = 40.0, 2.5, 1.8, 0.3
SEED = 2024


def spec(emb=DESCRIPTOR_SIZE, num_iters=NUM_ITERS):
    s = []

    def bnrelu(prefix, c_in, c_out, tail):
        s.append((f"{prefix}.conv.weight", (c_out, c_in) + tail))
        for n in ("weight", "bias", "running_mean", "running_var"):
            s.append((f"{prefix}.bn.{n}", (c_out,)))

    def block(prefix, channels, tail):
        for i in range(len(channels) - 2):
            bnrelu(f"{prefix}.conv.{i}", channels[i], channels[i + 1], tail)
        i = len(channels) - 2
        s.append((f"{prefix}.conv.{i}.weight", (channels[-1], channels[-2]) + tail))
        s.append((f"{prefix}.conv.{i}.bias", (channels[-1],)))
    for l, (a, b) in enumerate(((3, 64), (64, 64), (64, 64), (64, 64), (64, emb)), start=1):
        block(f"emb_nn.propogate{l}.conv2d", (a, b, b), (1, 1))
        block(f"emb_nn.propogate{l}.conv1d", (b, b), (1,))
    block("significance_fc", (emb, 64, 32, 1), (1,))
    for i in range(num_iters):
        block(f"sim_mat_conv1.{i}", (2 * emb + 4, 32, 32), (1, 1))
    for i in range(num_iters):
        block(f"sim_mat_conv2.{i}", (32, 32, 1), (1, 1))
    for i in range(num_iters):
        block(f"weight_fc.{i}", (32, 32, 1), (1,))
    return s


def make_state(seed=SEED, gain_first=GAIN_FIRST, gain=GAIN, gain_sim=GAIN_SIM, gain_w=GAIN_W):
    rng = np.random.default_rng(seed)
    st = {}
    for name, shape in spec():
        if name.endswith("running_var") or name.endswith("bn.weight"):
            v = rng.uniform(0.5, 1.5, shape)
        elif name.endswith("running_mean"):
            v = rng.normal(0, 0.2, shape)
        elif name.endswith("bias"):
            v = rng.uniform(-0.1, 0.1, shape)
        else:
            g = gain_first if name == "emb_nn.propogate1.conv2d.conv.0.conv.weight" else gain
            if name.startswith("sim_mat_conv"):
                g = gain_sim
            if name.startswith("weight_fc"):
                g = gain_w
            v = rng.uniform(-1, 1, shape) * g / np.sqrt(shape[1])
        st[name] = v.astype(np.float32)
    reflect = np.eye(3, dtype=np.float32)
    reflect[2, 2] = -1
    st["head.reflect"] = reflect
    return st


class Args:
    """The options models/idam.py reads (cfgs/idam_mi355x.yaml's values)."""
    descriptor_size, num_iters, use_fpfh = DESCRIPTOR_SIZE, NUM_ITERS, False
