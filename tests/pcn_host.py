"""NumPy restatement of the PCN contracts (include/houv_hip.h: houv_mlp2_max, houv_pcn_fold) and of the whole model
(registration/models/pcn.py), parametrised by dtype.  Everything is written in the REFERENCE's formulation -- channel-major
[B, C, N] activations, `repeat` + `cat` of the pooled / global features, the 1029-channel folding feature -- so the algebraic
splits the kernels rely on (one 512-vector per cloud instead of the concatenated channels) are tested, not assumed."""
import math

import numpy as np


def rows_times(x, W):
    """x[..., K] . W[C, K]^T -> [..., C], summed over k ascending in the arrays' own dtype, one product and one addition per
    term.  np.einsum / BLAS pick their summation order by the host's vector width, and a float32 error bound measured through them
    would differ from host to host; this order is the same everywhere."""
    acc = np.zeros(x.shape[:-1] + (W.shape[0],), dtype=x.dtype)
    for k in range(x.shape[-1]):
        acc += x[..., k:k + 1] * W[:, k]
    return acc


def conv1d(x, W, b):
    """nn.Conv1d with a kernel of width 1: x[B,Cin,N], W[Cout,Cin], b[Cout] -> [B,Cout,N]."""
    return np.ascontiguousarray(np.swapaxes(rows_times(np.ascontiguousarray(np.swapaxes(x, 1, 2)), W), 1, 2)) + b[None, :, None]


def relu(x):
    return np.maximum(x, 0)


def mlp2_max(x, W1, shift1, W2, b2, dtype=np.float64):
    """The contract of houv_mlp2_max: x[B,N,Cin]; shift1 [H] or [B,H] -> (pooled[B,Cout], y[B,N,Cout])."""
    x, W1, shift1, W2, b2 = (np.asarray(a, dtype=dtype) for a in (x, W1, shift1, W2, b2))
    h = relu(rows_times(x, W1) + (shift1[None, None, :] if shift1.ndim == 1 else shift1[:, None, :]))
    y = rows_times(h, W2) + b2
    assert y.dtype == dtype
    return y.max(1), y


def fold(coarse, feat, grid, W1, b1, W2, b2, W3, b3, dtype=np.float64):
    """pcn.py:108-125 as written: coarse[B,3,nc] channel-major, feat[B,1024], grid[2,scale], W1[512,1029] -> fine[B,3,nf]."""
    coarse, feat, grid, W1, b1, W2, b2, W3, b3 = (np.asarray(a, dtype=dtype) for a in (coarse, feat, grid, W1, b1, W2, b2, W3, b3))
    B, _, nc = coarse.shape
    scale = grid.shape[1]
    nf = nc * scale
    grid_feat = np.tile(grid[None], (B, 1, nc))                                              # [B,2,nf]
    point = np.repeat(np.swapaxes(coarse, 1, 2)[:, :, None, :], scale, axis=2).reshape(B, nf, 3)
    point_feat = np.swapaxes(point, 1, 2)                                                    # [B,3,nf]
    global_feat = np.repeat(feat[:, :, None], nf, axis=2)                                    # [B,1024,nf]
    cat = np.concatenate([grid_feat, point_feat, global_feat], 1)                            # [B,1029,nf]
    fine = conv1d(relu(conv1d(relu(conv1d(cat, W1, b1)), W2, b2)), W3, b3) + point_feat
    assert fine.dtype == dtype
    return fine


def fold_rows(coarse_rows, cvec, grid, Wgp, W2, b2, W3, b3, dtype=np.float64):
    """The contract of houv_pcn_fold in the reference's formulation: a 1029-channel convolution whose global part reproduces
    `cvec` (a one-hot feature through [I | 0] columns would not test the split; instead the 5 per-point channels are
    concatenated with cvec itself as extra channels under identity weights).  coarse_rows[B,nc,3] -> fine[B,nf,3]."""
    cvec = np.asarray(cvec, dtype=dtype)
    W1 = np.concatenate([np.asarray(Wgp, dtype=dtype), np.eye(512, dtype=dtype)], 1)         # [512, 5 + 512]
    out = fold(np.swapaxes(np.asarray(coarse_rows, dtype=dtype), 1, 2), cvec, grid, W1, np.zeros(512, dtype=dtype), W2, b2, W3,
               b3, dtype)
    return np.ascontiguousarray(np.swapaxes(out, 1, 2))


def gen_grid_up(up_ratio, grid_size=0.2, dtype=np.float32):
    """model_utils_completion.py:236-249; torch.linspace in float32 is start + i * step from the lower half and end - (n-1-i) * step
    from the upper: restated through float32 arithmetic the same way."""
    sqrted = int(math.sqrt(up_ratio)) + 1
    for i in range(sqrted, 0, -1):
        if up_ratio % i == 0:
            num_x, num_y = i, up_ratio // i
            break

    def linspace(n):
        if n == 1:
            return np.array([-grid_size], dtype=np.float32)
        step = np.float32((np.float32(grid_size) - np.float32(-grid_size)) / np.float32(n - 1))
        i = np.arange(n)
        lo = np.float32(-grid_size) + step * i.astype(np.float32)
        hi = np.float32(grid_size) - step * (n - 1 - i).astype(np.float32)
        return np.where(i < n // 2, lo, hi).astype(np.float32)
    x, y = np.meshgrid(linspace(num_x), linspace(num_y), indexing="ij")
    return np.ascontiguousarray(np.stack([x, y], -1).reshape(-1, 2).T).astype(dtype)


def encoder(state, x, dtype=np.float64):
    """pcn.py:20-29: x[B,3,N] -> [B,1024]."""
    w = lambda n: np.asarray(state[n], dtype=dtype).reshape(state[n].shape[0], -1)
    b = lambda n: np.asarray(state[n], dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    N = x.shape[2]
    x = relu(conv1d(x, w("encoder.conv1.weight"), b("encoder.conv1.bias")))
    x = conv1d(x, w("encoder.conv2.weight"), b("encoder.conv2.bias"))
    g = x.max(2)
    x = np.concatenate([x, np.repeat(g[:, :, None], N, axis=2)], 1)
    x = relu(conv1d(x, w("encoder.conv3.weight"), b("encoder.conv3.bias")))
    x = conv1d(x, w("encoder.conv4.weight"), b("encoder.conv4.bias"))
    return x.max(2)


def decoder(state, feat, num_coarse, scale, dtype=np.float64):
    """pcn.py:102-126: feat[B,1024] -> (coarse[B,3,nc], fine[B,3,nf])."""
    w = lambda n: np.asarray(state[n], dtype=dtype).reshape(state[n].shape[0], -1)
    b = lambda n: np.asarray(state[n], dtype=dtype)
    feat = np.asarray(feat, dtype=dtype)
    c = relu(rows_times(feat, w("decoder.fc1.weight")) + b("decoder.fc1.bias"))
    c = relu(rows_times(c, w("decoder.fc2.weight")) + b("decoder.fc2.bias"))
    coarse = (rows_times(c, w("decoder.fc3.weight")) + b("decoder.fc3.bias")).reshape(-1, 3, num_coarse)
    grid = gen_grid_up(2 ** int(math.log2(scale)), 0.05)
    fine = fold(coarse, feat, grid, w("decoder.conv1.weight"), b("decoder.conv1.bias"), w("decoder.conv2.weight"),
                b("decoder.conv2.bias"), w("decoder.conv3.weight"), b("decoder.conv3.bias"), dtype)
    return coarse, fine


def model(state, x, num_points, num_coarse, dtype=np.float64):
    """-> dict(feat[B,1024], out1[B,nc,3], out2[B,num_points,3]) as Model.forward returns them (rows of points)."""
    feat = encoder(state, x, dtype)
    coarse, fine = decoder(state, feat, num_coarse, num_points // num_coarse, dtype)
    return dict(feat=feat, out1=np.ascontiguousarray(np.swapaxes(coarse, 1, 2)), out2=np.ascontiguousarray(np.swapaxes(fine, 1, 2)))
