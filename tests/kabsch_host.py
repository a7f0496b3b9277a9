"""NumPy restatement of houv_kabsch's contract (SVDHead.forward, registration/model_utils.py:220-255; include/houv_hip.h), two
passes, with the arithmetic type as an argument as in tests/deepgmr_host.py: float64 is the yardstick the kernel is held to,
float32 shows what the formula itself loses in fp32.  Also the input builders of tests/test_gpu_kabsch.py."""
import functools

import numpy as np

EPS32 = 2.0 ** -24
SCALES = (1.0, 0.6, 0.3)          # axis scales of the source cloud: distinct singular values of H


def kabsch(src, corr, w=None, dtype=np.float64):
    """src, corr [B,3,N]; w [B,1,N], [B,N] or None -> R[B,3,3], t[B,3] in dtype.
    Centre both clouds by their UNWEIGHTED means; H = (src_c * w) corr_c^T; H = U S V^T; R = V diag(1, 1, det(V U^T)) U^T;
    t = -R mean(src) + mean(corr), or with weights t = -R sum(w src) + sum(w corr) (sums, not means)."""
    s = np.asarray(src, dtype=dtype)
    c = np.asarray(corr, dtype=dtype)
    B, _, N = s.shape
    ms = s.mean(axis=2, keepdims=True, dtype=dtype)
    mc = c.mean(axis=2, keepdims=True, dtype=dtype)
    sc, cc = s - ms, c - mc
    if w is not None:
        w = np.asarray(w, dtype=dtype).reshape(B, 1, N)
        sc = sc * w
    H = np.matmul(sc, np.swapaxes(cc, 1, 2)).astype(dtype)
    U, _, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, 1, 2)
    Ut = np.swapaxes(U, 1, 2)
    d = np.linalg.det(np.matmul(V, Ut)).astype(dtype)
    D = np.tile(np.eye(3, dtype=dtype), (B, 1, 1))
    D[:, 2, 2] = d
    R = np.matmul(np.matmul(V, D), Ut).astype(dtype)
    if w is None:
        t = mc - np.matmul(R, ms)
    else:
        t = (w * c).sum(axis=2, keepdims=True, dtype=dtype) - np.matmul(R, (w * s).sum(axis=2, keepdims=True, dtype=dtype))
    assert R.dtype == dtype and t.dtype == dtype
    return R, t[:, :, 0]


def _rotations(rng, B):
    q, _ = np.linalg.qr(rng.standard_normal((B, 3, 3)))
    return q * np.sign(np.linalg.det(q))[:, None, None]


def polar_gap(src, corr, w=None):
    """min over the batch of (sigma2 + det * sigma3) / sigma1 of H in float64: R is the (det-fixed) polar factor of H^T, whose
    sensitivity to a perturbation of H is 1 / (sigma_i + sigma_j), the last sigma counted negative under a reflection."""
    s = np.asarray(src, np.float64)
    c = np.asarray(corr, np.float64)
    sc = s - s.mean(2, keepdims=True)
    if w is not None:
        sc = sc * np.asarray(w, np.float64).reshape(len(s), 1, -1)
    H = sc @ np.swapaxes(c - c.mean(2, keepdims=True), 1, 2)
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)))
    return float(((S[:, 1] + d * S[:, 2]) / S[:, 0]).min())


@functools.lru_cache(maxsize=None)
def make_case(B, N, weighted=False, offset=False, reflect=False):
    """-> (src[B,3,N], corr[B,3,N], w[B,1,N] or None) fp32, read-only, well conditioned by construction:
    src uniform in a box of extent (1, 0.6, 0.3), centred at the origin or (offset) at (100, -100, 100);
    corr = R0 src + t0 + 1e-3 * noise with a random rotation R0 and |t0| ~ 1, then (reflect) mirrored through the plane z = 0,
    so that det(V U^T) < 0 and the reflection fix fires; w uniform in [0, 1) with floor(N / 10) entries per sample exactly 0.
    With a handful of points a draw can still be nearly flat; such draws (polar_gap < 0.05) are drawn again (N >= 2 only:
    one point gives H = 0 whatever it is)."""
    rng = np.random.default_rng([B, N, int(weighted), int(offset), int(reflect)])
    while True:
        src = (rng.random((B, 3, N)) - 0.5) * np.array(SCALES)[None, :, None]
        if offset:
            src = src + np.array([100.0, -100.0, 100.0])[None, :, None]
        corr = _rotations(rng, B) @ src + rng.standard_normal((B, 3, 1)) + 1e-3 * rng.standard_normal((B, 3, N))
        if reflect:
            corr[:, 2] = -corr[:, 2]
        w = None
        if weighted:
            w = rng.random((B, 1, N))
            for b in range(B):
                w[b, 0, rng.permutation(N)[:N // 10]] = 0.0
            w = w.astype(np.float32)
        src, corr = src.astype(np.float32), corr.astype(np.float32)
        if N == 1 or polar_gap(src, corr, w) >= 0.05:
            break
    for a in (src, corr, w):
        if a is not None:
            a.setflags(write=False)
    return src, corr, w


def errors(R, t, R64, t64):
    """(max |R - R64|, max |t - t64|) over the batch."""
    return (float(np.abs(np.asarray(R, np.float64) - R64).max()), float(np.abs(np.asarray(t, np.float64) - t64).max()))


@functools.lru_cache(maxsize=None)
def reference_and_bounds(B, N, weighted=False, offset=False, reflect=False):
    """-> (R64, t64, (yardstick_R, yardstick_t), (bound_R, bound_t)) for make_case(...): the float64 reference, the error of the
    SAME two-pass formula in float32 against it, and bound = 4 x yardstick + 8 x 2^-24 x max |value| (R and t separately).
    The x4 is the project's margin for a different summation order; the floor is eight roundings of the
    largest value, for cases where the float32 reference happens to land on the float64 one."""
    src, corr, w = make_case(B, N, weighted, offset, reflect)
    R64, t64 = kabsch(src, corr, w, np.float64)
    yard = errors(*kabsch(src, corr, w, np.float32), R64, t64)
    bound = (4 * yard[0] + 8 * EPS32 * float(np.abs(R64).max()), 4 * yard[1] + 8 * EPS32 * float(np.abs(t64).max()))
    return R64, t64, yard, bound
