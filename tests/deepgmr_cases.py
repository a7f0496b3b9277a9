"""Inputs, yardsticks and bounds shared by tests/test_deepgmr_host.py (CPU) and tests/test_gpu_deepgmr.py (GPU).

The bounds TOL_DOT, TOL_PHI and TOL_REG are NOT taken from the kernels: `python tests/deepgmr_cases.py` measures what the
float32 NumPy restatement (tests/deepgmr_host.py) loses against its float64 run on exactly the inputs below, and the bounds are
4x the maxima over all cases (another libm, another summation order -- nothing beyond that).  Measured maxima:

    theta   |theta32 - theta64| * max(sin theta64, 1e-3)   2.50e-07 at (3, 64, 20)      -> TOL_DOT = 1.0e-06
            (unscaled |theta32 - theta64| reaches 3.7e-05 at (1, 2048, 20): acos near +-1, hence the sin scaling)
    phi     |phi32 - phi64| on unflagged entries            9.70e-06 at (1, 2048, 20)    -> TOL_PHI = 3.9e-05
    T       |T32 - T64| of gmm_register                     2.14e-07 at (257, 32)        -> TOL_REG = 8.6e-07
    flagged share of (point, j) entries: 0 .. 0.95 % (largest at (1, 21, 20)); 0.78 % at (1, 2048, 20)
"""
import numpy as np

import deepgmr_host as host

RRI_SHAPES = [(1, 21, 20), (3, 64, 20), (2, 65, 20), (2, 300, 5), (2, 33, 31), (1, 129, 2), (1, 2048, 20)]   # (B, N, k)
GMM_SHAPES = [(1, 1, 1), (2, 63, 16), (2, 64, 16), (3, 1025, 16), (1, 2048, 32), (1, 16384, 5)]              # (B, N, J)
REG_SHAPES = [(1, 4), (5, 16), (64, 16), (257, 32)]                                                           # (B, J)

TOL_DOT = 1.0e-06
TOL_PHI = 3.9e-05
TOL_REG = 8.6e-07
FLAG_DELTA = 1e-3           # an entry is flagged when some psi[j,i], i != j, lies this close to 0 or 2 pi in float64
MAX_FLAGGED = 0.02

_cache = {}


def surface_cloud(B, N, seed):
    """fp32 [B,N,3]: points of a bumpy closed surface of radius 0.3..0.5 around a centre 0.2 away from the origin: |p| and the
    angle between p and the surface vary over the cloud, and the origin stays inside (seen from outside, the surface is edge-on
    along its silhouette, where all tangent vectors of a point are coplanar with p and the share of flagged entries grows)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((B, N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    r = 0.5 * (0.8 + 0.2 * np.sin(3 * d[..., :1]) * np.cos(2 * d[..., 1:2]))
    return (d * r + np.array([0.12, -0.1, 0.12])).astype(np.float32)


def knn_lists(xyz, L):
    """idx[B,N,L] int32: the L nearest points of each point in its own cloud by (float64 squared distance, index), itself first."""
    x = xyz.astype(np.float64)
    out = np.empty(xyz.shape[:2] + (L,), np.int32)
    for b in range(x.shape[0]):
        d2 = ((x[b][:, None, :] - x[b][None, :, :]) ** 2).sum(-1)
        d2[np.arange(len(d2)), np.arange(len(d2))] = -1.0
        out[b] = np.argsort(d2, axis=1, kind="stable")[:, :L]
    return out


def rri_case(B, N, k):
    """(xyz fp32, idx[B,N,k+1] with the point itself first) of one RRI shape; the yardsticks come from `rri_yardstick`."""
    key = ("rri", B, N, k)
    if key not in _cache:
        xyz = surface_cloud(B, N, seed=1000 * N + k)
        _cache[key] = (xyz, knn_lists(xyz, k + 1))
    return _cache[key]


def rri_yardstick(xyz, nbr, k):
    """float64 restatement on the fp32 inputs: (features[B,N,4k], psi[B,N,k,k], flagged[B,N,k])."""
    rp, rq, theta, psi = host.rri_psi(xyz, nbr, k, np.float64)
    feat = host.rri_features(xyz, nbr, k, np.float64)
    off = ~np.eye(k, dtype=bool)
    with np.errstate(invalid="ignore"):
        near = (np.minimum(psi, 2 * np.pi - psi) < FLAG_DELTA) & off
    return feat, psi, near.any(-1)


def check_rri(got, feat64, psi64, flagged, k, label=""):
    """The RRI acceptance rule: returns the measured figures and raises AssertionError when a bound is missed.  `got` [B,N,4k]."""
    got = np.asarray(got, dtype=np.float64).reshape(feat64.shape[:2] + (k, 4))
    want = feat64.reshape(got.shape)
    eps = float(np.finfo(np.float32).eps)
    fig = {}
    for f, name in ((0, "rp"), (1, "rq")):
        ulp = np.abs(got[..., f] - want[..., f]) / (eps * np.abs(want[..., f]))     # >= the error in ulps of the fp32 value
        fig[name + "_ulp"] = float(np.nanmax(ulp))
    nan_same = np.array_equal(np.isnan(got), np.isnan(want))
    with np.errstate(invalid="ignore"):
        th = np.abs(got[..., 2] - want[..., 2]) * np.maximum(np.sin(want[..., 2]), 1e-3)
        fig["theta"] = float(np.nanmax(th)) if np.isfinite(th).any() else 0.0
        dphi = np.abs(got[..., 3] - want[..., 3])
        fig["phi_unflagged"] = float(np.nanmax(np.where(flagged, 0.0, dphi))) if (~flagged).any() else 0.0
        # flagged entries: phi must be one of the row's psi values, or 0 / 2 pi (the wrap a rounding can cross)
        cand = np.concatenate([psi64, np.zeros_like(psi64[..., :1]), np.full_like(psi64[..., :1], 2 * np.pi)], axis=-1)
        dmin = np.nanmin(np.abs(got[..., 3][..., None] - cand), axis=-1)
        fig["phi_flagged"] = float(np.nanmax(np.where(flagged, dmin, 0.0))) if flagged.any() else 0.0
    fig["flagged_share"] = float(flagged.mean())
    print(label, {n: float(f"{v:.3g}") for n, v in fig.items()})
    assert nan_same, f"{label}: NaN pattern differs"
    assert fig["rp_ulp"] <= 4 and fig["rq_ulp"] <= 4, (label, fig)
    assert fig["theta"] <= TOL_DOT, (label, fig)
    assert fig["phi_unflagged"] <= TOL_PHI and fig["phi_flagged"] <= TOL_PHI, (label, fig)
    assert fig["flagged_share"] <= MAX_FLAGGED, (label, fig)
    return fig


def gmm_case(B, N, J):
    """gamma[B,N,J] fp32 = row softmax of seeded logits, pts[B,N,3] fp32."""
    rng = np.random.default_rng(7 * N + J)
    logits = rng.normal(0, 1.5, (B, N, J))
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32), surface_cloud(B, N, seed=N + J)


def reg_case(B, J, mirrored=False):
    """fp32 (pi_s[B,J], mu_s[B,J,3], mu_t = R_gt mu_s + t_gt, sigma_t[B,J] in [0.01, 0.1], T_gt[B,4,4] fp64): poses of up to 180
    degrees; `mirrored`: mu_t is a REFLECTION of mu_s instead.  Asserted in float64: the two smallest singular values of Ms differ
    by a factor >= 1.5 (otherwise U, V are not determined and the case tests nothing)."""
    rng = np.random.default_rng(100 * B + J + (5000 if mirrored else 0))
    out = []
    while len(out) < B:
        w = rng.uniform(0.5, 1.5, J); w /= w.sum()
        ms = rng.uniform(-0.5, 0.5, (J, 3)) * np.array([1.0, 0.6, 0.35])
        ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(0, np.pi)
        A = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * A @ A
        if mirrored:
            R = R @ np.diag([1.0, 1.0, -1.0])
        t = rng.uniform(-0.5, 0.5, 3)
        mt = ms @ R.T + t
        sg = rng.uniform(0.01, 0.1, J)
        one = [a.astype(np.float32) for a in (w, ms, mt, sg)]
        _, _, S, _ = host.gmm_register(*[a[None] for a in one], np.float64, return_svd=True)
        if S[0, 1] < 1.5 * S[0, 2] or S[0, 0] < 1.5 * S[0, 1]:
            continue                                   # ill-determined singular vectors: draw again (the seed fixes the sequence)
        Tg = np.eye(4); Tg[:3, :3] = R; Tg[:3, 3] = t
        out.append(one + [Tg])
    cols = [np.stack(c) for c in zip(*out)]
    _, _, S, _ = host.gmm_register(*cols[:4], np.float64, return_svd=True)
    assert (S[:, 1] >= 1.5 * S[:, 2]).all()
    return cols


def measure():
    worst = {"theta": 0.0, "phi": 0.0, "reg": 0.0}
    for B, N, k in RRI_SHAPES:
        xyz, idx = rri_case(B, N, k)
        nbr = idx[..., 1:]
        feat64, psi64, flagged = rri_yardstick(xyz, nbr, k)
        f32 = host.rri_features(xyz, nbr, k, np.float32).astype(np.float64).reshape(B, N, k, 4)
        w = feat64.reshape(B, N, k, 4)
        th = float((np.abs(f32[..., 2] - w[..., 2]) * np.maximum(np.sin(w[..., 2]), 1e-3)).max())
        ph = float(np.where(flagged, 0, np.abs(f32[..., 3] - w[..., 3])).max())
        print((B, N, k), "theta", th, "unscaled", float(np.abs(f32[..., 2] - w[..., 2]).max()), "phi", ph, "flagged", float(flagged.mean()))
        worst["theta"] = max(worst["theta"], th); worst["phi"] = max(worst["phi"], ph)
    for B, J, mirrored in [s + (False,) for s in REG_SHAPES] + [(8, 16, True)]:
        c = reg_case(B, J, mirrored)
        T32 = host.gmm_register(*c[:4], np.float32)
        T64 = host.gmm_register(*c[:4], np.float64)
        e = float(np.abs(T32 - T64).max())
        print("register", (B, J, mirrored), e, "vs pose", float(np.abs(T64 - c[4]).max()))
        worst["reg"] = max(worst["reg"], e)
    print({k: f"{v:.3g} -> x4 = {4 * v:.3g}" for k, v in worst.items()})


if __name__ == "__main__":
    measure()
