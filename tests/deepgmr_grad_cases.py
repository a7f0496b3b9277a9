"""Inputs, yardsticks and bounds shared by the DeepGMR training tests (test_deepgmr_grad_host.py on the CPU, test_gpu_deepgmr_grad.py
and test_gpu_deepgmr_train.py on the GPU).

Kernel bounds are not taken from the kernels: every case runs the restatement of tests/deepgmr_grad_host.py in float64 (the
yardstick) and in float32 on the same fp32 inputs.  Per output the difference between the two is divided by the case's scale for
that output (below), the maximum of that figure over ALL cases is taken, and a kernel output may differ from the yardstick by
KERNEL_FACTOR = 4 x that maximum times its case's scale -- the rule of tests/deepgmr_cases.py, 4 x the maxima over all cases.
`python tests/deepgmr_grad_cases.py` prints the tables (DESIGN.md section 9.18 quotes them).

Scales.  The rounding error of a sum is proportional to the sum of the magnitudes of its terms, not to its value, which may
cancel: mean -> max over columns of mean |z|; gbias -> of sum |g|; gweight -> of sum |g xhat|; var -> its largest value (the
terms are squares); gz -> the largest of (weight rstd) (|g| + |mean g| + |xhat mean(g xhat)|), the magnitudes of the three
terms it is the difference of (with two rows they cancel to zero).  Every other output -> the largest magnitude of the yardstick's output.  Columns whose result is exact in both
precisions (the constant column, the column the ReLU zeroes) are additionally held to exact equality by the GPU test.

Whole-step gradients are held to GRAD_SPREADS = 8 x the fp32-vs-fp64 spread the reference itself shows for that parameter
(recorded in the fixture), the multiple the forward's tests use."""
import functools
import os
import sys

import numpy as np

import deepgmr_grad_host as host

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import deepgmr_weights  # noqa: E402

CHUNK = host.CHUNK
FIXTURE_CASES = ("n64", "n100")
WEIGHT_SEED, K = 2024, 20
GRAD_SPREADS = 8.0
KERNEL_FACTOR = 4.0
F32, F64 = np.float32, np.float64


# ---- the whole training step against the fixture ----------------------------------------------------------------------------
def restated_step(g, name, dtype):
    return host.train_step(deepgmr_weights.make_state(WEIGHT_SEED), g[f"{name}_src"], g[f"{name}_tgt"], g[f"{name}_T_gt"],
                           g[f"{name}_knn1"], g[f"{name}_knn2"], K, dtype)


def against_golden(g, name, param, grad):
    """(the entries of `grad` the fixture holds, the fixture's float64 values, max |golden|), all flat float64."""
    got = np.asarray(grad, F64).reshape(-1)
    if f"sample_{param}" in g.files:
        got = got[g[f"sample_{param}"]]
    ref = g[f"{name}_grad_{param}"].astype(F64).reshape(-1)
    return got, ref, float(np.abs(ref).max())


def golden_buffers(g, name):
    prefix = f"{name}_buf_"
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def buffer_tolerance(g, name, key):
    """GRAD_SPREADS x the buffer's recorded fp32-vs-fp64 spread, absolute."""
    return GRAD_SPREADS * float(g[f"{name}_bufspread_{key}"]) * float(np.abs(g[f"{name}_buf_{key}"]).max())


def buffers_after(stats):
    """The BatchNorm buffers after the step, from the restatement's record of batch statistics (layer, mean, biased var, rows)
    in call order: nn.BatchNorm1d's update, momentum 0.1, the variance unbiased."""
    state = {k: v.astype(F64) for k, v in deepgmr_weights.make_state(WEIGHT_SEED).items()}
    out = {}
    for layer, mean, var, rows in stats:
        rm, rv, nb = (f"{layer}.bn.running_mean", f"{layer}.bn.running_var", f"{layer}.bn.num_batches_tracked")
        out[rm] = 0.9 * out.get(rm, state[rm]) + 0.1 * np.asarray(mean, F64)
        out[rv] = 0.9 * out.get(rv, state[rv]) + 0.1 * np.asarray(var, F64) * (rows / (rows - 1))
        out[nb] = out.get(nb, 0) + 1
    return out


# ---- houv_bn_rows_stats / houv_bn_relu_rows / houv_bn_relu_rows_backward ----------------------------------------------------
BN_ROWS = (2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 300)
BN_COLS = (1, 16, 64, 100, 1024)
BN_PADS = (4, 1)                       # ld = C + pad: rows stay 16-byte aligned (the 16-byte path) / do not (the scalar path)
BN_GROUP = {2: 1, 63: 21, 64: 32, 65: 13, CHUNK - 1: CHUNK - 1, CHUNK: 64, CHUNK + 1: 43, 2 * CHUNK + 3: 37, 300: 150}
BN_KINK = 0.02                         # no |y| of a case lies nearer the ReLU's kink than this (so fp32 and fp64 agree on the mask)
BN_EPS = 1e-5
BN_OUTPUTS = ("mean", "var", "y", "lin", "gz", "gweight", "gbias")
assert all(r % n == 0 for r, n in BN_GROUP.items()) and CHUNK % 21 and CHUNK % 37 and 150 > CHUNK


def _figure(a32, a64, scale):
    return float(np.abs(np.asarray(a32, F64) - np.asarray(a64, F64)).max()) / scale if scale > 0 else 0.0


@functools.lru_cache(maxsize=None)
def _bn_core(R, C):
    rng = np.random.default_rng(1000 * R + C)
    n_group = BN_GROUP[R]
    z = (rng.standard_normal((R, C)) * rng.uniform(0.5, 2.0, C) + rng.standard_normal(C)).astype(F32)
    weight = rng.uniform(0.5, 1.5, C).astype(F32)
    bias = rng.uniform(-0.4, 0.4, C).astype(F32)
    special = C >= 4
    if special:
        z[:, 1] = 1.5
        bias[1] = 0.3
        z[:, 2] = (100 + 0.01 * rng.standard_normal(R)).astype(F32)
        weight[3], bias[3] = 0.5, -10.0

    def impose(z):
        h = n_group // 2
        v = z.reshape(R // n_group, n_group, C)
        v[:, h:2 * h] = v[:, :h]
        return z

    for _ in range(50):
        z = impose(z)
        mean, var = host.bn_rows_stats(z, F64)
        y = host.bn_relu_rows(z, mean, var, weight, bias, BN_EPS, False, 0, F64)
        close = np.abs(y) < BN_KINK
        if not close.any():
            break
        z = (z + close * (0.1 * np.sqrt(var) + 1e-3)).astype(F32)
    kink = float(np.abs(y).min())
    assert kink >= BN_KINK, (R, C, kink)
    gy = rng.standard_normal((R, C)).astype(F32)
    # the kernels' inputs: mean / var as float32 (what houv_bn_rows_stats hands on), each kernel judged on the inputs it gets
    mean_in, var_in = mean.astype(F32), var.astype(F32)
    res = {}
    for dt in (F64, F32):
        m, v = host.bn_rows_stats(z, dt)
        yy, gmax, garg = host.bn_relu_rows(z, mean_in, var_in, weight, bias, BN_EPS, True, n_group, dt)
        lin = host.bn_relu_rows(z, mean_in, var_in, weight, bias, BN_EPS, False, 0, dt)
        gz, gw, gb = host.bn_relu_rows_backward(gy, z, mean_in, var_in, weight, bias, BN_EPS, True, dt)
        res[dt] = dict(mean=m, var=v, y=yy, gmax=gmax, garg=garg, lin=lin, gz=gz, gweight=gw, gbias=gb)
    assert np.array_equal(res[F32]["y"] > 0, res[F64]["y"] > 0)
    ref = res[F64]
    g = gy.astype(F64) * (ref["y"] > 0)
    xhat = (z.astype(F64) - mean_in) / np.sqrt(var_in.astype(F64) + BN_EPS)
    coef = weight.astype(F64) / np.sqrt(var_in.astype(F64) + BN_EPS)
    scales = dict(mean=float(np.abs(z.astype(F64)).mean(0).max()), var=float(ref["var"].max()), y=float(np.abs(ref["lin"]).max()),
                  lin=float(np.abs(ref["lin"]).max()), gz=float((coef * (np.abs(g) + np.abs(g.mean(0)) + np.abs(xhat * (g * xhat).mean(0)))).max()),
                  gweight=float(np.abs(g * xhat).sum(0).max()), gbias=float(np.abs(g).sum(0).max()))
    figures = {k: _figure(res[F32][k], ref[k], scales[k]) for k in BN_OUTPUTS}
    return dict(R=R, C=C, z=z, gy=gy, weight=weight, bias=bias, n_group=n_group, mean_in=mean_in, var_in=var_in, ref=ref,
                scales=scales, figures=figures, kink=kink, constant_column=1 if special else None,
                masked_column=3 if special else None)


@functools.lru_cache(maxsize=None)
def bn_table():
    """Per output: (the largest float32-vs-float64 figure over all BatchNorm cases, the (R, C) it occurs at)."""
    best = {k: (0.0, None) for k in BN_OUTPUTS}
    for R in BN_ROWS:
        for C in BN_COLS:
            for k, f in _bn_core(R, C)["figures"].items():
                if f > best[k][0]:
                    best[k] = (f, (R, C))
    return best


@functools.lru_cache(maxsize=None)
def bn_case(R, C, pad=4):
    """One BatchNorm case: z[R, C + pad] float32 (the last `pad` columns are padding the kernels must not touch), gy likewise,
    weight / bias, the group size, the float64 yardsticks `ref`, and `bounds` (absolute, for this case).  With C >= 4: column 1 is
    constant (variance 0), column 2 has mean 100 and deviation 0.01 (cancellation), column 3 is zeroed by the ReLU everywhere.
    Within every group the second half of the rows repeats the first, so every maximum is attained twice and garg must name
    the lower row."""
    c = dict(_bn_core(R, C))
    table = bn_table()
    c["bounds"] = {k: KERNEL_FACTOR * table[k][0] * c["scales"][k] for k in BN_OUTPUTS}
    c["pad_fill"] = np.float32(777.0)
    wide = lambda a: np.concatenate([a, np.full((R, pad), c["pad_fill"], F32)], 1)
    c.update(ld=C + pad, z=wide(c["z"]), gy=wide(c["gy"]))
    return c


# ---- houv_gmm_params_backward ----------------------------------------------------------------------------------------------
PARAMS_SHAPES = ((1, 1, 1), (2, 33, 16), (1, 257, 32), (3, 64, 5))


@functools.lru_cache(maxsize=None)
def _params_core(B, N, J):
    import deepgmr_host as fwd
    rng = np.random.default_rng(100 * N + J)
    logits = rng.standard_normal((B, N, J)) * 2
    e = np.exp(logits - logits.max(-1, keepdims=True))
    gamma = (e / e.sum(-1, keepdims=True)).astype(F32)
    pts = (rng.standard_normal((B, N, 3)) * 0.5).astype(F32)
    pi, mu, sigma = fwd.gmm_params(gamma, pts, F32)
    g = [rng.standard_normal(s).astype(F32) for s in ((B, J), (B, J, 3), (B, J))]
    args = (gamma, pts, pi, mu, sigma, *g)
    r64, r32 = host.gmm_params_backward(*args, dtype=F64), host.gmm_params_backward(*args, dtype=F32)
    scale = float(np.abs(r64).max())
    return dict(args=args, ref=r64, scale=scale, figure=_figure(r32, r64, scale))


@functools.lru_cache(maxsize=None)
def params_table():
    return max((_params_core(*s)["figure"], s) for s in PARAMS_SHAPES)


def params_case(B, N, J):
    """gamma of a softmax, pi / mu / sigma of the float32 forward.  (1, 1, 1): one component, the gradient is exactly zero."""
    c = dict(_params_core(B, N, J))
    c["bound"] = KERNEL_FACTOR * params_table()[0] * c["scale"]
    return c


# ---- houv_gmm_register_backward --------------------------------------------------------------------------------------------
REGISTER_SHAPES = tuple((B, J) for J in (4, 16, 32) for B in (1, 65))
REGISTER_OUTPUTS = ("g_pi_s", "g_mu_s", "g_mu_t", "g_sigma_t")
REGISTER_GAP = 0.01                    # min over pairs and i != j of lam_i + lam_j, asserted by the generator


def _pair(rng, J, reflect):
    """One pair whose target means are the source's under a rotation (or, `reflect`, a reflection: det(V U^T) < 0) plus noise."""
    pi = rng.uniform(0.5, 1.5, J)
    pi /= pi.sum()
    ms = rng.standard_normal((J, 3)) * np.array([1.0, 0.7, 0.4])
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if (np.linalg.det(Q) < 0) != reflect:
        Q[:, 0] = -Q[:, 0]
    mt = ms @ Q.T + 0.05 * rng.standard_normal((J, 3)) + rng.standard_normal(3)
    return pi.astype(F32), ms.astype(F32), mt.astype(F32), rng.uniform(0.5, 1.5, J).astype(F32)


@functools.lru_cache(maxsize=None)
def _register_core(B, J):
    import deepgmr_host as fwd
    rng = np.random.default_rng(10 * B + J)
    pairs = []
    while len(pairs) < B:
        p = _pair(rng, J, reflect=len(pairs) % 3 == 0)
        _, gap = host.gmm_register_backward(*(a[None] for a in p), np.zeros((1, 4, 4)), F64, return_gap=True)
        if gap >= 2 * REGISTER_GAP:
            pairs.append(p)
    pi_s, mu_s, mu_t, sigma_t = (np.stack([p[i] for p in pairs]) for i in range(4))
    g_T = rng.standard_normal((B, 4, 4)).astype(F32)
    args = (pi_s, mu_s, mu_t, sigma_t, g_T)
    r64, gap = host.gmm_register_backward(*args, F64, return_gap=True)
    r32 = host.gmm_register_backward(*args, F32)
    det = fwd.gmm_register(pi_s, mu_s, mu_t, sigma_t, F64, return_svd=True)[3]
    assert gap >= REGISTER_GAP and (det < 0).sum() >= 1, (B, J, gap)
    scales = [float(np.abs(r).max()) for r in r64]
    return dict(pi_s=pi_s, mu_s=mu_s, mu_t=mu_t, sigma_t=sigma_t, g_T=g_T, ref=r64, scales=scales,
                figures=[_figure(a, b, s) for a, b, s in zip(r32, r64, scales)], gap=gap, negative=int((det < 0).sum()))


@functools.lru_cache(maxsize=None)
def register_table():
    return [max((_register_core(*s)["figures"][i], s) for s in REGISTER_SHAPES) for i in range(4)]


def register_case(B, J):
    """Every third pair (the only one, when B = 1) is a reflection.  A drawn pair is kept when its lam_i + lam_j all exceed twice
    REGISTER_GAP; the gap of the whole case is then asserted on the float32 inputs."""
    c = dict(_register_core(B, J))
    c["bounds"] = [KERNEL_FACTOR * register_table()[i][0] * c["scales"][i] for i in range(4)]
    return c


if __name__ == "__main__":
    print("BatchNorm rows: largest |float32 - float64| / scale over", len(BN_ROWS) * len(BN_COLS), "cases")
    for k, (f, at) in bn_table().items():
        print(f"    {k:8s} {f:.2e} at (R, C) = {at}   -> bound {KERNEL_FACTOR * f:.2e} x scale")
    f, at = params_table()
    print(f"houv_gmm_params_backward   g_logits {f:.2e} at (B, N, J) = {at}   -> bound {KERNEL_FACTOR * f:.2e} x scale")
    for name, (f, at) in zip(REGISTER_OUTPUTS, register_table()):
        print(f"houv_gmm_register_backward {name:9s} {f:.2e} at (B, J) = {at}   -> bound {KERNEL_FACTOR * f:.2e} x scale")
