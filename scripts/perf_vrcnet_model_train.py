#!/usr/bin/env python3
"""VRCNet's "train" prefix, two measurements.

The loss node alone.  model_utils_completion.cd_loss (houv_chamfer_forward, then houv_cd_loss_backward's ordered sums) against
calc_cd (the same forward, torch's sqrt / mean backward and houv_chamfer_backward's float atomics) on the same device in the
same run: B = 48 clouds, a ground truth of 2048 points, M = 1024, 3072, 2048, 8192 output points -- random clouds, and the
BUNCHED case with every output within 1e-3 of the origin, where a few output rows are the nearest neighbour of hundreds of
ground-truth points each.  Forward + backward of L = <G, (cd_p, cd_t)>, allocator peak, and the two backward entry points alone.
The baseline of every row is calc_cd, never an earlier build of these kernels.

One whole "train" step at the shipped cfg's shapes (cfgs/vrcnet_mi355x.yaml: 2048 input points, num_coarse_raw 1024, 2048
output points, folding, the point label; seeded weights), at the first of --batch (default: the cfg's 24), 16, 8 that fits --
the largest batch that fits is not searched for: forward, backward, peak, and what the four losses cost on the step's own
clouds, with the node and with calc_cd in its place.

Median of RUNS timed runs after WARM warm-up runs, device events, one device; peak memory is torch's allocator peak over one
forward + backward, above what is allocated before it.  Every shape runs in a child process of its own under a time limit.

    python scripts/perf_vrcnet_model_train.py [--out profiles/perf_vrcnet_model_train.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B_LOSS, N_GT = 48, 2048
# (label, M, bunched)
JOBS = tuple((f"loss M={M:4d} {'bunched' if b else 'random '}", M, b) for M in (1024, 3072, 2048, 8192) for b in (False, True)) + (("step", 0, False),)
LIMIT = 300                                      # seconds per job


def loss_job(i):
    import torch
    from perf_vrcnet import RUNS, WARM, timed
    from perf_vrcnet_train import measure
    from houv_amd import _lib, ops
    from houv_amd.metrics import cd
    from houv_amd.model_utils_completion import calc_cd, cd_loss
    label, M, bunched = JOBS[i]
    dev = torch.device("cuda:0")
    if i == 0:
        print(f"build {_lib.build_id()}  median of {RUNS} after {WARM} warm-up runs, device events; this = cd_loss (ordered sums), "
              f"atomic = calc_cd;  B={B_LOSS}, ground truth {N_GT} points")
    gen = torch.Generator().manual_seed(33)
    gt = (torch.rand(B_LOSS, N_GT, 3, generator=gen) - 0.5).to(dev)
    out = ((torch.rand(B_LOSS, M, 3, generator=gen) - 0.5) * (2e-3 if bunched else 1.0)).to(dev).requires_grad_(True)
    G = (torch.rand(2, B_LOSS, generator=gen) + 0.5).to(dev)
    a = measure(lambda: torch.stack(cd_loss(out, gt)), [out], G)
    b = measure(lambda: torch.stack(calc_cd(out, gt)), [out], G)
    with torch.no_grad():
        d1, d2, i1, i2 = cd()(gt, out)
        longest = int(torch.stack([torch.bincount(r.long(), minlength=M) for r in i1]).max())
        o = out.detach()
        k_node = timed(lambda: ops.cd_loss_backward(o, gt, d1, d2, i1, i2, G[0], G[1]))
        g1, g2, z1, z2 = torch.rand_like(d1), torch.rand_like(d2), torch.zeros_like(gt), torch.zeros_like(o)
        k_atomic = timed(lambda: ops.chamfer_backward(gt, o, z1, z2, g1, g2, i1, i2))
    # forward and backward are not reported apart: at these sizes the event between them lands wherever the host's dispatch
    # happens to be, so only their sum and the kernels alone carry information
    print(f"{label}: forward + backward {a[0] + a[1]:7.3f} / {b[0] + b[1]:7.3f} ms ({(b[0] + b[1]) / (a[0] + a[1]):4.2f}x)   "
          f"peak {a[2]:6.1f} / {b[2]:6.1f} MiB   this / atomic;   longest list {longest:4d};   "
          f"houv_cd_loss_backward alone {k_node:.3f} ms, houv_chamfer_backward alone {k_atomic:.3f} ms")


def step_job(batch):
    import torch
    import vrcnet_host
    from perf_vrcnet import RUNS, WARM, timed
    from vrcnet_cases import vrcnet_weights as W
    import houv_amd.models.vrcnet as vrc
    from houv_amd.model_utils_completion import calc_cd, cd_loss
    dev = torch.device("cuda:0")
    c = vrcnet_host.cfg()
    state = {n: torch.tensor(v) for n, v in W.make_state(W.spec(c), W.SEED + 11).items()}
    trace = {}
    net = vrc.Model(W.args(c), trace=trace, trainable=True)
    net.load_state_dict(state, strict=True)
    net = net.to(dev).train()
    for B in dict.fromkeys((batch, 16, 8)):
        gen = torch.Generator().manual_seed(34)
        x = (torch.rand(B, 3, c.num_input, generator=gen) - 0.5).to(dev)
        gt = (torch.rand(B, 2048, 3, generator=gen) - 0.5).to(dev)
        eps = tuple(torch.randn(B, 128, generator=gen).to(dev) for _ in range(2))

        def step(loss_fn):
            vrc.cd_loss = loss_fn
            fw, bw = [], []
            for run in range(WARM + RUNS + 1):
                for p in net.parameters():
                    p.grad = None
                if run == WARM + RUNS:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                total = net(x, gt, prefix="train", alpha=0.5, eps=eps)[2]
                e[1].record()
                total.backward()
                e[2].record()
                torch.cuda.synchronize()
                if WARM <= run < WARM + RUNS:
                    fw.append(e[0].elapsed_time(e[1]))
                    bw.append(e[1].elapsed_time(e[2]))
            peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            import statistics
            return statistics.median(fw), statistics.median(bw), peak

        try:
            node = step(cd_loss)
        except torch.cuda.OutOfMemoryError:
            print(f"step B={B}: does not fit")
            torch.cuda.empty_cache()
            continue
        clouds = [trace[n].detach().clone().requires_grad_(True) for n in ("coarse_raw", "coarse_high", "coarse", "fine")]
        gt2 = torch.cat((gt, gt), 0)

        def four(loss_fn):
            for t in clouds:
                t.grad = None
            sum(loss_fn(t, gt2)[0].mean() for t in clouds).backward()

        t_node, t_atomic = timed(lambda: four(cd_loss)), timed(lambda: four(calc_cd))
        atomic = step(calc_cd)
        vrc.cd_loss = cd_loss
        print(f"step B={B} (doubled to {2 * B}; {c.num_input} input points, ground truth 2048, outputs {[t.shape[1] for t in clouds]}): "
              f"forward {node[0]:.2f} ms, backward {node[1]:.2f} ms, peak {node[2]:.0f} MiB with the node;  forward {atomic[0]:.2f} ms, "
              f"backward {atomic[1]:.2f} ms, peak {atomic[2]:.0f} MiB with calc_cd in its place")
        print(f"    the four losses, forward + backward: {t_node:.3f} ms with the node ({100 * t_node / (node[0] + node[1]):.2f} % of the "
              f"step), {t_atomic:.3f} ms with calc_cd ({100 * t_atomic / (atomic[0] + atomic[1]):.2f} % of the step)")
        return
    print("step: no batch fits")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=24, help="the first batch size the whole step tries")
    ap.add_argument("--job", type=int, default=None, help="run one job in this process (used by the parent)")
    args = ap.parse_args()
    if args.job is not None:
        return step_job(args.batch) if JOBS[args.job][0] == "step" else loss_job(args.job)
    lines = []                                   # the parent never touches the device: every job is a fresh child
    for i in range(len(JOBS)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--job", str(i), "--batch", str(args.batch)],
                               capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            lines.append(f"{JOBS[i][0]}: no result within {LIMIT} s")
            break
        if p.returncode != 0:                    # nothing more is started on the device after a failure
            lines.append(f"{JOBS[i][0]}: exit status {p.returncode}\n{p.stderr[-2000:]}")
            break
        lines.append(p.stdout.rstrip())
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
