"""CPU: the NumPy restatements of the DeepGMR contracts (tests/deepgmr_host.py) against golden vectors from the reference's
deepgmr.py (tests/golden/g23_deepgmr.npz, tests/golden/make_golden_deepgmr.py), and the C ABI of the three new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

import deepgmr_cases as cases
import deepgmr_host as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20


@pytest.mark.parametrize("name", ["n64", "n256"])
def test_rri_restatement_in_float32_matches_the_reference(golden, name):
    """Fed the reference's own neighbour lists, the float32 restatement reproduces the reference's float32 features: |p|, |q| to
    4 ulp, theta and phi by the rules of the GPU test (deepgmr_cases.check_rri; the yardstick that decides which phi entries sit
    next to the 0 / 2 pi wrap is the float64 restatement)."""
    g = golden("g23_deepgmr.npz")
    xyz, nbr = g[f"{name}_src"], g[f"{name}_knn1_f32"]
    ref = np.transpose(g[f"{name}_rri1_f32"], (0, 2, 1))                   # [B,4k,N] -> [B,N,4k]
    mine = host.rri_features(xyz, nbr, K, np.float32)
    assert mine.dtype == np.float32 and mine.shape == ref.shape
    feat64, psi64, flagged = cases.rri_yardstick(xyz, nbr, K)
    want = ref.astype(np.float64).reshape(feat64.shape[:2] + (K, 4))
    got = mine.astype(np.float64).reshape(want.shape)
    ulp = np.abs(got[..., :2] - want[..., :2]) / (np.finfo(np.float32).eps * np.abs(want[..., :2]))
    theta = np.abs(got[..., 2] - want[..., 2]) * np.maximum(np.sin(feat64.reshape(want.shape)[..., 2]), 1e-3)
    dphi = np.abs(got[..., 3] - want[..., 3])
    cand = np.concatenate([psi64, np.zeros_like(psi64[..., :1]), np.full_like(psi64[..., :1], 2 * np.pi)], axis=-1)
    near = lambda v: np.abs(v[..., None] - cand).min(-1)
    print(name, "ulp", ulp.max(), "theta", theta.max(), "phi unflagged", np.where(flagged, 0, dphi).max(), "flagged share", flagged.mean())
    assert ulp.max() <= 4
    assert theta.max() <= cases.TOL_DOT
    assert np.where(flagged, 0, dphi).max() <= cases.TOL_PHI
    assert np.where(flagged, near(got[..., 3]), 0).max() <= cases.TOL_PHI
    assert flagged.mean() <= cases.MAX_FLAGGED


@pytest.mark.parametrize("name", ["n64", "n256"])
def test_gmm_restatements_in_float64_match_the_reference(golden, name):
    g = golden("g23_deepgmr.npz")
    for c, pts in (("1", "src"), ("2", "tgt")):
        pi, mu, sigma = host.gmm_params(g[f"{name}_gamma{c}_f64"], g[f"{name}_{pts}"], np.float64)
        np.testing.assert_allclose(pi, g[f"{name}_pi{c}_f64"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(mu, g[f"{name}_mu{c}_f64"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(sigma, g[f"{name}_sigma{c}_f64"], rtol=0, atol=1e-10)
    T = host.gmm_register(g[f"{name}_pi1_f64"], g[f"{name}_mu1_f64"], g[f"{name}_mu2_f64"], g[f"{name}_sigma2_f64"], np.float64)
    np.testing.assert_allclose(T, g[f"{name}_T12_f64"], rtol=0, atol=1e-10)


def test_fixture_is_well_conditioned(golden):
    g = golden("g23_deepgmr.npz")
    spread = max(float(np.abs(g[f"{n}_T12_f32"] - g[f"{n}_T12_f64"]).max()) for n in ("n64", "n256"))
    assert spread == float(g["t12_spread"]) < 1e-3


def test_state_dict_names_equal_reference(golden):
    from argparse import Namespace
    from houv_amd.models.deepgmr import Model
    net = Model(Namespace(use_rri=True, rri_size=20, num_groups=16, use_tnet=False))
    mine = sorted(k for k in net.state_dict() if not k.endswith("num_batches_tracked"))
    assert mine == [str(k) for k in golden("g23_deepgmr.npz")["state_keys"]]
    tn = Model(Namespace(use_rri=False, rri_size=20, num_groups=8, use_tnet=True)).state_dict()
    assert tn["backbone.tnet.decoder.2.bias"].shape == (6,) and tn["backbone.encoder.0.conv.weight"].shape == (64, 3, 1)
    assert tn["backbone.decoder.3.weight"].shape == (8, 128, 1) and "backbone.tnet.decoder.0.linear.weight" in tn


_PROTOS = {
    "houv_rri_features": (9, r"const float\s*\*\s*xyz,\s*const int32_t\s*\*\s*idx,\s*int B,\s*int N,\s*int k,\s*int idx_ld,\s*"
                             r"int idx_skip,\s*float\s*\*\s*out,\s*void\s*\*\s*stream"),
    "houv_gmm_params": (9, r"const float\s*\*\s*gamma,\s*const float\s*\*\s*pts,\s*int B,\s*int N,\s*int J,\s*float\s*\*\s*pi,\s*"
                           r"float\s*\*\s*mu,\s*float\s*\*\s*sigma,\s*void\s*\*\s*stream"),
    "houv_gmm_register": (8, r"const float\s*\*\s*pi_s,\s*const float\s*\*\s*mu_s,\s*const float\s*\*\s*mu_t,\s*"
                             r"const float\s*\*\s*sigma_t,\s*int B,\s*int J,\s*float\s*\*\s*T,\s*void\s*\*\s*stream"),
}


@pytest.mark.parametrize("name", sorted(_PROTOS))
def test_deepgmr_entry_points_are_declared_exported_and_bound(name):
    from houv_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    nargs, proto = _PROTOS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "houv_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + proto + r"\s*\)", header)
    assert name in _lib.exported_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    fn = getattr(_lib.load(), name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert _lib.load().houv_abi_version() == _lib.ABI_VERSION == 2          # additive: the ABI version stays
