"""AvUC loss + backward: the HIP kernels (bayesian_torch_amd.utils.avuc_loss) against the same loss written as vectorised torch ops on
the GPU in fp32 (the expression of tests/_avu_ref.evaluate) -- DESIGN.md 4.7.  The reference's own Python loop is not timed: it
synchronises the device several times per row and takes seconds per call.

Protocol: one process, one device.  Per (shape, T) both implementations are warmed up, then timed in alternation: REPS windows each, a
window being CALLS back-to-back calls (loss, then backward into the logits' .grad) between one pair of HIP events, ending in a
synchronise; reported: median, min and max of the per-call time over the windows, in microseconds.  "eager": the Python calls as a
training loop makes them (host enqueue included); "graph": the same step captured once in a torch.cuda.graph and replayed (what
mc.TrainGraph pays).  Shapes: [256, 10] and [256, 1000] logits, and 16 Monte Carlo samples of [256, 10] (types 0 and 1).

    python tools/time_avu.py [--reps 20] [--calls 50] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS = 1e-10
SHAPES = [("B256_C10", 1, 256, 10, 0), ("B256_C1000", 1, 256, 1000, 0), ("S16_B256_C10_type0", 16, 256, 10, 0), ("S16_B256_C10_type1", 16, 256, 10, 1)]


def torch_loss(z, y, ut, T, th, beta, x):
    """The loss in vectorised fp32 torch ops on z's device (thresholds in double, masks without gradient); no host read."""
    p = torch.softmax(z, -1)
    pbar = p.mean(0)
    c, pred = pbar.max(-1)
    H = lambda q: -(q * torch.log(q + EPS)).sum(-1)   # noqa: E731
    u = H(pbar) - H(p).mean(0) if ut else H(pbar)
    t = torch.tanh(u)
    ud = u.detach().double()
    if T == 1:
        thr = th.double()
    else:
        thr = ud.min() + x * (ud.max() - ud.min())
        thr = torch.cat([ud.min().reshape(1), thr[1:-1], ud.max().reshape(1)])
    cert = ud[None, :] <= thr[:, None]
    acc = (pred == y)[None, :]
    n_ac = torch.where(acc & cert, (c * (1 - t))[None, :], 0.0).sum(1)
    n_au = torch.where(acc & ~cert, (c * t)[None, :], 0.0).sum(1)
    n_ic = torch.where(~acc & cert, ((1 - c) * (1 - t))[None, :], 0.0).sum(1)
    n_iu = torch.where(~acc & ~cert, ((1 - c) * t)[None, :], 0.0).sum(1)
    avu = (n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu + EPS)
    v = avu[0] if T == 1 else torch.trapezoid(avu.double(), x).float()
    return -beta * torch.log(v + EPS)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def captured(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_avu.py measures on the GPU; none is available")
    from bayesian_torch_amd.utils.avuc_loss import AvULoss, AUAvULoss
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.linspace(0, 1, 21)).to(dev)
    for name, S, B, C, ut in SHAPES:
        torch.manual_seed(0)
        base = torch.randn(B, C) * 2
        y = torch.randint(0, C, (B,))
        y[::2] = base[::2].argmax(-1)
        z = (base[None] + (0.7 * torch.randn(S, B, C) if S > 1 else 0)).to(dev).requires_grad_()
        y = y.to(dev)
        probe = AUAvULoss()
        probe(z.detach(), y, type=ut)
        us = probe.last_stats["uncertainty"].sort().values
        th = (0.5 * (us[B // 2 - 1] + us[B // 2])).reshape(1)      # the T = 1 threshold: between the two middle uncertainties (on no row)
        for T in (1, 21):
            mod = AvULoss(beta=1.5) if T == 1 else AUAvULoss(beta=1.5)

            def hip():
                z.grad = None
                out = mod(z, y, th, type=ut) if T == 1 else mod(z, y, type=ut)[0]
                out.backward()

            def ops():
                z.grad = None
                torch_loss(z, y, ut, T, th, 1.5, x).backward()
            hip()
            g_hip = z.grad.clone()
            hip()
            same_bits = torch.equal(z.grad, g_hip)
            ops()
            diff = float((z.grad - g_hip).abs().max() / g_hip.abs().max())
            # grad_rel_diff is reported, not held: the tests hold the accuracy, on batches where no row lies within rounding of a threshold.
            # Here nothing keeps a row off the 21 thresholds, and the two implementations' u differ in the last bits: a row may change class.
            assert same_bits and diff == diff, (name, T, same_bits, diff)
            impls = {"hip eager": hip, "torch eager": ops, "hip graph": captured(hip), "torch graph": captured(ops)}
            times = {k: [] for k in impls}
            for k, fn in impls.items():
                for _ in range(args.warmup):
                    fn()
            for _ in range(args.reps):
                for k, fn in impls.items():
                    times[k].append(window(fn, args.calls))
            row = dict(shape=name, T=T, grad_rel_diff=diff, windows=args.reps, calls_per_window=args.calls)
            for k, v in times.items():
                row[k.replace(" ", "_") + "_us"] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
