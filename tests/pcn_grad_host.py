"""NumPy backward of tests/pcn_host.py's PointNet block (the contract of houv_mlp2_max_backward, include/houv_hip.h; DESIGN.md
section 9.12) in the reference's MATERIALISING form: a dense [B,N,Cout] gradient of y, the maximum's backward as a one-hot of
`arg` added into it, every row of every cloud pushed through both products.  The dtype is a parameter, `arg` is injected, and
every product is summed over k ascending (pcn_host.rows_times), so a float32 error measured through it is the same on every
host."""
import numpy as np

import pcn_host as host


def hidden_pre(x, W1, shift1, dtype=np.float64):
    """The ReLU's input, [B,N,H]."""
    x, W1, shift1 = (np.asarray(a, dtype=dtype) for a in (x, W1, shift1))
    return host.rows_times(x, W1) + (shift1[None, None, :] if shift1.ndim == 1 else shift1[:, None, :])


def mlp2_max_backward(x, W1, shift1, W2, arg, gpooled, gy=None, dtype=np.float64):
    """x[B,N,Cin], arg[B,Cout] (an entry outside 0..N-1 passes nothing), gpooled[B,Cout], gy[B,N,Cout] or None ->
    dict(gW1[H,Cin], gshift1[B,H], gW2[Cout,H], gb2[Cout], gx[B,N,Cin])."""
    x, W1, W2, gpooled = (np.asarray(a, dtype=dtype) for a in (x, W1, W2, gpooled))
    B, N, Cin = x.shape
    H, Cout = W1.shape[0], W2.shape[0]
    pre = hidden_pre(x, W1, shift1, dtype)
    h = host.relu(pre)
    gz = np.zeros((B, N, Cout), dtype=dtype) if gy is None else np.array(gy, dtype=dtype)
    for b in range(B):
        for c in range(Cout):
            if 0 <= arg[b, c] < N:
                gz[b, arg[b, c], c] += gpooled[b, c]
    gzf, hf, xf = gz.reshape(B * N, Cout), h.reshape(B * N, H), x.reshape(B * N, Cin)
    ones = np.ones((1, B * N), dtype=dtype)
    gb2 = host.rows_times(np.ascontiguousarray(gzf.T), ones)[:, 0]
    gW2 = host.rows_times(np.ascontiguousarray(gzf.T), np.ascontiguousarray(hf.T))
    gh = host.rows_times(gz, np.ascontiguousarray(W2.T)) * (pre > 0)
    ghf = gh.reshape(B * N, H)
    gW1 = host.rows_times(np.ascontiguousarray(ghf.T), np.ascontiguousarray(xf.T))
    gshift1 = np.stack([host.rows_times(np.ascontiguousarray(gh[b].T), ones[:, :N])[:, 0] for b in range(B)])
    gx = host.rows_times(gh, np.ascontiguousarray(W1.T))
    out = dict(gW1=gW1, gshift1=gshift1, gW2=gW2, gb2=gb2, gx=gx)
    assert all(v.dtype == dtype for v in out.values())
    return out


def clear_of_kinks(x, W1, shift1):
    """True when every ReLU input of the block is at least delta away from zero in the float64 forward, delta = 4x the largest
    float32-vs-float64 difference of those inputs: the gradient's mask is then the same in both precisions and in any careful
    float32 evaluation.  No element is masked out: a case either qualifies whole or is not used."""
    p64, p32 = hidden_pre(x, W1, shift1, np.float64), hidden_pre(x, W1, shift1, np.float32)
    return float(np.abs(p64).min()) >= 4 * float(np.abs(p32 - p64).max())


def encoder_backward(w, x, gfeat, dtype=np.float64, backward=True):
    """PCN_encoder (pcn_host.encoder) and its backward, un-split: w maps conv1..conv4 .weight [out,in] / .bias, x[B,N,3] rows,
    gfeat[B,1024] -> (feat, dict of the eight parameter gradients, arg1, arg2, (y, z, pre1, pre2): both blocks' pre-pool
    activations and ReLU inputs, for choosing inputs away from the kinks).  conv3 sees cat(y, repeat(g1)): the gradient of
    its pooled half is summed over all N columns here, as the reference's autograd does."""
    c = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    x = np.asarray(x, dtype=dtype)
    B, N, _ = x.shape
    g1, y = host.mlp2_max(x, c["conv1.weight"], c["conv1.bias"], c["conv2.weight"], c["conv2.bias"], dtype)
    arg1 = y.argmax(1)
    cat = np.concatenate([y, np.repeat(g1[:, None, :], N, axis=1)], 2)                     # [B,N,512]
    feat, z = host.mlp2_max(cat, c["conv3.weight"], c["conv3.bias"], c["conv4.weight"], c["conv4.bias"], dtype)
    arg2 = z.argmax(1)
    kinks = (y, z, hidden_pre(x, c["conv1.weight"], c["conv1.bias"], dtype), hidden_pre(cat, c["conv3.weight"], c["conv3.bias"], dtype))
    if not backward:                                                                       # the forward's decisions only
        return feat, None, arg1, arg2, kinks
    r2 = mlp2_max_backward(cat, c["conv3.weight"], c["conv3.bias"], c["conv4.weight"], arg2, gfeat, None, dtype)
    gcat = r2["gx"]
    gg1 = np.zeros_like(g1)
    for n in range(N):
        gg1 += gcat[:, n, 256:]
    r1 = mlp2_max_backward(x, c["conv1.weight"], c["conv1.bias"], c["conv2.weight"], arg1, gg1, gcat[:, :, :256], dtype)
    ones = np.ones((1, B), dtype=dtype)
    bias = lambda g: host.rows_times(np.ascontiguousarray(g.T), ones)[:, 0]
    grads = {"conv1.weight": r1["gW1"], "conv1.bias": bias(r1["gshift1"]), "conv2.weight": r1["gW2"], "conv2.bias": r1["gb2"],
             "conv3.weight": r2["gW1"], "conv3.bias": bias(r2["gshift1"]), "conv4.weight": r2["gW2"], "conv4.bias": r2["gb2"]}
    return feat, grads, arg1, arg2, kinks


def ordered_times(x, W):
    """pcn_host.rows_times (x[..., K] . W[C, K]^T, one product and one addition per term, k ascending, in the arrays' dtype)
    without a fresh temporary per term: the same values bit for bit, about twice as fast on the long products below."""
    acc = np.zeros(x.shape[:-1] + (W.shape[0],), dtype=x.dtype)
    tmp = np.empty_like(acc)
    Wt = np.ascontiguousarray(W.T)
    xt = np.ascontiguousarray(np.moveaxis(x, -1, 0))[..., None]
    for k in range(x.shape[-1]):
        np.multiply(xt[k], Wt[k], out=tmp)
        acc += tmp
    return acc


def fold_cat_backward(coarse_rows, glob, grid, W1, b1, W2, b2, W3, b3, gfine, dtype=np.float64):
    """pcn.py:108-125 and its backward as the reference materialises them: the per-point feature cat[B,nf,5+F] = (grid cell,
    centre, `glob` repeated over the points) goes through conv1 = W1[512,5+F] + b1, conv2, conv3 (+ the centre), and the dense
    gradient of cat is reduced afterwards: gglob = sum over a cloud's points of gcat[..., 5:], gcoarse = the centre path plus
    gcat[..., 2:5] summed over a centre's cells.  -> dict(fine, gcoarse[B,nc,3], gglob[B,F], gW1, gb1, gW2, gb2, gW3, gb3,
    pre1, pre2)."""
    coarse_rows, glob, grid, W1, b1, W2, b2, W3, b3, gfine = (np.asarray(a, dtype=dtype) for a in
                                                              (coarse_rows, glob, grid, W1, b1, W2, b2, W3, b3, gfine))
    B, nc, _ = coarse_rows.shape
    scale = grid.shape[1]
    nf = nc * scale
    F = glob.shape[1]
    # float32: every product summed over k ascending (the error that bounds the kernel's must not depend on the host's BLAS);
    # float64 is the yardstick itself, 1e-16 whatever the order, and goes through matmul: the [512,512] x 3120-row products of the
    # largest case take 26 s otherwise
    times = (lambda x, W: x @ W.T) if dtype == np.float64 else ordered_times
    point = np.repeat(coarse_rows[:, :, None, :], scale, axis=2).reshape(B, nf, 3)
    cells = np.tile(grid.T[None], (B, nc, 1))                                              # [B,nf,2]
    cat = np.concatenate([cells, point, np.repeat(glob[:, None, :], nf, axis=1)], 2)       # [B,nf,5+F]
    pre1 = times(cat, W1) + b1
    h1 = host.relu(pre1)
    pre2 = times(h1, W2) + b2
    h2 = host.relu(pre2)
    fine = times(h2, W3) + b3 + point
    flat = lambda a: np.ascontiguousarray(a.reshape(B * nf, -1).T)                         # [C, B*nf]: rows become the k axis
    ones = np.ones((1, B * nf), dtype=dtype)
    gW3 = times(flat(gfine), flat(h2))
    gb3 = times(flat(gfine), ones)[:, 0]
    gh2 = times(gfine, np.ascontiguousarray(W3.T)) * (pre2 > 0)
    gW2 = times(flat(gh2), flat(h1))
    gb2 = times(flat(gh2), ones)[:, 0]
    gh1 = times(gh2, np.ascontiguousarray(W2.T)) * (pre1 > 0)
    gW1 = times(flat(gh1), flat(cat))                                                      # [512,5+F]
    gb1 = times(flat(gh1), ones)[:, 0]
    gcat = times(gh1, np.ascontiguousarray(W1.T))                                          # [B,nf,5+F]
    gglob = np.zeros((B, F), dtype=dtype)
    for f in range(nf):
        gglob += gcat[:, f, 5:]
    gpoint = (gfine + gcat[:, :, 2:5]).reshape(B, nc, scale, 3)
    gcoarse = np.zeros((B, nc, 3), dtype=dtype)
    for j in range(scale):
        gcoarse += gpoint[:, :, j]
    out = dict(fine=fine, gcoarse=gcoarse, gglob=gglob, gW1=gW1, gb1=gb1, gW2=gW2, gb2=gb2, gW3=gW3, gb3=gb3)
    assert all(v.dtype == dtype for v in out.values())
    out.update(pre1=pre1, pre2=pre2)
    return out


def fold_backward(coarse_rows, cvec, grid, Wgp, W2, b2, W3, b3, gfine, dtype=np.float64):
    """Backward of pcn_host.fold_rows (the contract of houv_pcn_fold_backward) in the materialising form, as fold_rows states the
    forward: cvec itself rides along as 512 extra channels under identity weights, W1 = [Wgp | I], no bias.
    -> dict(gcoarse[B,nc,3], gcvec[B,512], gWgp[512,5], gW2, gb2, gW3, gb3, pre1, pre2)."""
    W1 = np.concatenate([np.asarray(Wgp, dtype=dtype), np.eye(512, dtype=dtype)], 1)
    r = fold_cat_backward(coarse_rows, cvec, grid, W1, np.zeros(512, dtype=dtype), W2, b2, W3, b3, gfine, dtype)
    return dict(gcoarse=r["gcoarse"], gcvec=r["gglob"], gWgp=np.ascontiguousarray(r["gW1"][:, :5]), gW2=r["gW2"], gb2=r["gb2"],
                gW3=r["gW3"], gb3=r["gb3"], pre1=r["pre1"], pre2=r["pre2"])


def linear_backward(x, W, b, gy, relu, dtype):
    """y = relu?(x W^T + b) -> (y, pre, gx, gW, gb) under the gradient gy of y (a callable: it may depend on y)."""
    times = (lambda a, M: a @ M.T) if dtype == np.float64 else ordered_times
    pre = times(x, W) + b
    y = host.relu(pre) if relu else pre
    return y, pre, lambda g: (lambda gz: (times(gz, np.ascontiguousarray(W.T)), times(np.ascontiguousarray(gz.T), np.ascontiguousarray(x.T)),
                                          times(np.ascontiguousarray(gz.T), np.ones((1, x.shape[0]), dtype=dtype))[:, 0]))(g * (pre > 0) if relu else g)


def model_kinks(state, x, num_points, num_coarse, dtype=np.float64):
    """The forward of pcn_host.model with what decides its gradient's discontinuities: -> (relu: the inputs of the six ReLUs,
    pools: the two pre-pool activations [B,N,C]).  float64 goes through matmul (this is what a seed search calls)."""
    times = (lambda a, M: a @ M.T) if dtype == np.float64 else ordered_times
    w = lambda n: np.asarray(state[n], dtype=dtype).reshape(state[n].shape[0], -1)
    b = lambda n: np.asarray(state[n], dtype=dtype)
    rows = np.ascontiguousarray(np.swapaxes(np.asarray(x, dtype=dtype), 1, 2))
    B, N, _ = rows.shape
    e1 = times(rows, w("encoder.conv1.weight")) + b("encoder.conv1.bias")
    y = times(host.relu(e1), w("encoder.conv2.weight")) + b("encoder.conv2.bias")
    cat = np.concatenate([y, np.repeat(y.max(1)[:, None, :], N, axis=1)], 2)
    e2 = times(cat, w("encoder.conv3.weight")) + b("encoder.conv3.bias")
    z = times(host.relu(e2), w("encoder.conv4.weight")) + b("encoder.conv4.bias")
    feat = z.max(1)
    p1 = times(feat, w("decoder.fc1.weight")) + b("decoder.fc1.bias")
    p2 = times(host.relu(p1), w("decoder.fc2.weight")) + b("decoder.fc2.bias")
    c3 = times(host.relu(p2), w("decoder.fc3.weight")) + b("decoder.fc3.bias")
    coarse_rows = np.swapaxes(c3.reshape(B, 3, num_coarse), 1, 2)
    scale = num_points // num_coarse
    grid = np.asarray(host.gen_grid_up(2 ** int(np.log2(scale)), 0.05), dtype=dtype)
    point = np.repeat(coarse_rows, scale, axis=1)
    fcat = np.concatenate([np.tile(grid.T[None], (B, num_coarse, 1)), point, np.repeat(feat[:, None, :], num_points, axis=1)], 2)
    f1 = times(fcat, w("decoder.conv1.weight")) + b("decoder.conv1.bias")
    f2 = times(host.relu(f1), w("decoder.conv2.weight")) + b("decoder.conv2.bias")
    return (e1, e2, p1, p2, f1, f2), (y, z)


def clear_margins(k64, k32):
    """The issue's rule on two model_kinks results: every ReLU input at least delta from zero and every pool's runner-up at least
    delta below its maximum in float64, delta = 4x that quantity's float32-vs-float64 spread.  -> (ok, smallest margin / delta)."""
    worst = np.inf
    for a, b in zip(k64[0], k32[0]):
        worst = min(worst, float(np.abs(a).min()) / (4 * float(np.abs(a - b).max())))
    for a, b in zip(k64[1], k32[1]):
        top = np.sort(a, 1)
        worst = min(worst, float((top[:, -1] - top[:, -2]).min()) / (4 * float(np.abs(a - b).max()))) if a.shape[1] > 1 else worst
    return worst >= 1, worst


def model_backward(state, x, G1, G2, num_points, num_coarse, dtype=np.float64):
    """pcn_host.model and the gradients of L = <G1, out1> + <G2, out2> with respect to its 20 parameters, in the reference's
    formulation throughout (dense gradients, one-hot maxima, cat / repeat un-split).  x[B,3,N], G1[B,nc,3], G2[B,num_points,3].
    -> dict(out1, out2, feat, grads {state name: array of the parameter's shape}, relu (the ReLU inputs of all six ReLUs),
    pools ((y, z): the two pre-pool activations [B,N,C]))."""
    w = lambda n: np.asarray(state[n], dtype=dtype).reshape(state[n].shape[0], -1)
    b = lambda n: np.asarray(state[n], dtype=dtype)
    G1, G2 = np.asarray(G1, dtype=dtype), np.asarray(G2, dtype=dtype)
    rows = np.ascontiguousarray(np.swapaxes(np.asarray(x, dtype=dtype), 1, 2))
    enc = {k[len("encoder."):]: (w(k) if k.endswith("weight") else b(k)) for k in state if k.startswith("encoder.")}
    feat, _, arg1, arg2, (y, z, pre_e1, pre_e2) = encoder_backward(enc, rows, None, dtype, backward=False)
    B = feat.shape[0]
    scale = num_points // num_coarse
    c1, p1, back1 = linear_backward(feat, w("decoder.fc1.weight"), b("decoder.fc1.bias"), None, True, dtype)
    c2, p2, back2 = linear_backward(c1, w("decoder.fc2.weight"), b("decoder.fc2.bias"), None, True, dtype)
    c3, _, back3 = linear_backward(c2, w("decoder.fc3.weight"), b("decoder.fc3.bias"), None, False, dtype)
    coarse_rows = np.ascontiguousarray(np.swapaxes(c3.reshape(B, 3, num_coarse), 1, 2))
    grid = host.gen_grid_up(2 ** int(np.log2(scale)), 0.05)
    f = fold_cat_backward(coarse_rows, feat, grid, w("decoder.conv1.weight"), b("decoder.conv1.bias"), w("decoder.conv2.weight"),
                          b("decoder.conv2.bias"), w("decoder.conv3.weight"), b("decoder.conv3.bias"), G2, dtype)
    gc3 = np.ascontiguousarray(np.swapaxes(G1 + f["gcoarse"], 1, 2)).reshape(B, 3 * num_coarse)
    gc2, gW_fc3, gb_fc3 = back3(gc3)
    gc1, gW_fc2, gb_fc2 = back2(gc2)
    gfeat, gW_fc1, gb_fc1 = back1(gc1)
    _, ge, _, _, _ = encoder_backward(enc, rows, gfeat + f["gglob"], dtype)
    grads = {"encoder." + k: v for k, v in ge.items()}
    grads.update({"decoder.fc1.weight": gW_fc1, "decoder.fc1.bias": gb_fc1, "decoder.fc2.weight": gW_fc2, "decoder.fc2.bias": gb_fc2,
                  "decoder.fc3.weight": gW_fc3, "decoder.fc3.bias": gb_fc3, "decoder.conv1.weight": f["gW1"], "decoder.conv1.bias": f["gb1"],
                  "decoder.conv2.weight": f["gW2"], "decoder.conv2.bias": f["gb2"], "decoder.conv3.weight": f["gW3"], "decoder.conv3.bias": f["gb3"]})
    grads = {k: v.reshape(np.asarray(state[k]).shape) for k, v in grads.items()}
    assert all(v.dtype == dtype for v in grads.values()) and len(grads) == 20
    return dict(out1=coarse_rows, out2=f["fine"], feat=feat, grads=grads, relu=(pre_e1, pre_e2, p1, p2, f["pre1"], f["pre2"]), pools=(y, z))
