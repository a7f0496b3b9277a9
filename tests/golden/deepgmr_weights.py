"""Deterministic DeepGMR weights shared by tests/golden/make_golden_deepgmr.py (which loads them into the REFERENCE model) and
by the tests (which load them into houv_amd.models.deepgmr.Model): the repository ships no trained DeepGMR checkpoint.
Names/shapes = the reference's state_dict (registration/models/deepgmr.py:174-204) for use_rri with rri_size 20, 16 groups, no
T-Net.  BatchNorm running statistics are randomised so that eval-mode BatchNorm is not the identity."""
import numpy as np

RRI_SIZE, NUM_GROUPS = 20, 16


def spec(rri_size=RRI_SIZE, num_groups=NUM_GROUPS):
    s = []

    def block(prefix, c_in, c_out):
        s.append((f"{prefix}.conv.weight", (c_out, c_in, 1)))
        for n in ("weight", "bias", "running_mean", "running_var"):
            s.append((f"{prefix}.bn.{n}", (c_out,)))
    for i, (a, b) in enumerate(((4 * rri_size, 64), (64, 128), (128, 256), (256, 1024))):
        block(f"backbone.encoder.{i}", a, b)
    for i, (a, b) in enumerate(((2048, 512), (512, 256), (256, 128))):
        block(f"backbone.decoder.{i}", a, b)
    s += [("backbone.decoder.3.weight", (num_groups, 128, 1)), ("backbone.decoder.3.bias", (num_groups,))]
    return s


def make_state(seed):
    rng = np.random.default_rng(seed)
    st = {}
    for name, shape in spec():
        if name.endswith("running_var") or name.endswith("bn.weight"):
            v = rng.uniform(0.5, 1.5, shape)
        elif name.endswith("running_mean") or name.endswith("bias"):
            v = rng.normal(0, 0.2, shape)
        else:
            v = rng.uniform(-1, 1, shape) * np.sqrt(3.0 / shape[1])
        st[name] = v.astype(np.float32)
    return st


class Args:
    """The options models/deepgmr.py reads (cfgs/deepgmr_mi355x.yaml's values)."""
    use_rri, rri_size, num_groups, use_tnet = True, RRI_SIZE, NUM_GROUPS, False
