"""LSTM layers: the "fused" path (one LSTM cell launch per step, KL once per forward) against the "torch" path (gate arithmetic in torch
ops, KL every step) -- DESIGN.md 4.6c.

Protocol (tools/conv3d_path_bench.py's): one process, one device; per (layer, S, mode, path) WARMUP calls, then N calls each timed with its
own pair of HIP events around the whole layer call; median, min and max in microseconds. Layers: LSTMReparameterization(128, 256) and
LSTMFlipout(128, 256) on x [64, 32, 128] (B = 64, T = 32). Modes: "infer" (no grad, x shared by S = 1 and by S = 16 MC samples) and
"train" (S = 1: forward, a sum loss and backward, gradients reset outside the timed region).

    python tools/lstm_path_bench.py [--n 200] [--warmup 20] [--paths fused,torch] [--cases infer1,infer16,train1] [--cell-stats KERNEL_STATS.csv]

A tree without the switch (the commit before it) runs its one path under the name "torch", at S = 1 only: it cannot batch samples.
Beside each row: the bytes the row's cell launches move, computed from the shapes (fp32: forward reads a, b [R, 4H] and c_prev, writes h
and c -- 11 R H words -- plus the 4 R H saved gates under grad; backward reads the gates, c_prev, c, grad_h, grad_c and writes dz, dc_prev
-- 13 R H words). ``--cell-stats``: a kernel-stats CSV of a SEPARATE ``rocprofv3 --kernel-trace --stats`` run of this script; the cell
kernels' average durations from it turn those bytes into GB/s, printed against the 8 TB/s HBM3E peak (6.3 TB/s is what a float4 copy
reaches). ``--trace``: a short run for such a profile (warm-up 2, n 5)."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_IN, HID, B, T = 128, 256, 64, 32
HBM_PEAK = 8.0e12


def cell_bytes(R, train):
    """(forward, backward) bytes of ONE cell launch over R rows."""
    return 4 * R * HID * (11 + (4 if train else 0)), (4 * R * HID * 13 if train else 0)


def cell_stats(path):
    """kernel-stats CSV of rocprofv3 -> {"fwd": average ns, "bwd": average ns} over the cell kernels' rows (weighted by calls)."""
    tot = {"fwd": [0.0, 0], "bwd": [0.0, 0]}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in tot:
                if "lstm_cell_%s_kernel" % k in name:
                    calls = int(row["Calls"])
                    tot[k][0] += float(row["AverageNs"]) * calls
                    tot[k][1] += calls
    return {k: (v[0] / v[1] if v[1] else None) for k, v in tot.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--paths", default="fused,torch")
    ap.add_argument("--cell-stats", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--cases", default="infer1,infer16,train1", help="which (mode, S) rows run: a profile wants one shape per run")
    args = ap.parse_args()
    if args.trace:
        args.n, args.warmup = 5, 2
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    set_path = getattr(L, "set_lstm_path", None)
    paths = [p for p in args.paths.split(",") if p == "torch" or set_path is not None]
    stats = cell_stats(args.cell_stats) if args.cell_stats else None
    torch.manual_seed(0)
    for cls in ("LSTMReparameterization", "LSTMFlipout"):
        layer = getattr(L, cls)(N_IN, HID).cuda()
        x = torch.randn(B, T, N_IN, device="cuda")
        for mode, S in (("infer", 1), ("infer", 16), ("train", 1)):
            if (S > 1 and set_path is None) or "%s%d" % (mode, S) not in args.cases.split(","):
                continue
            train = mode == "train"
            layer.train(train)
            for path in paths:
                if set_path is not None:
                    set_path(path)
                times = []
                for i in range(args.warmup + args.n):
                    for p in layer.parameters():
                        p.grad = None
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if train:
                        hs, (_, cs), kl = layer(x)
                        (hs.sum() + cs.sum() + kl).backward()
                    else:
                        with torch.no_grad(), mc.mc_samples(S, B):
                            hs = layer(x, return_kl=False)[0]
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        times.append(e0.elapsed_time(e1) * 1e3)
                    del hs
                fb, bb = cell_bytes(S * B, train)
                row = dict(layer=cls, mode=mode, S=S, path=path, median_us=round(statistics.median(times), 1), min_us=round(min(times), 1),
                           max_us=round(max(times), 1), n=len(times), cell_launches=T * (2 if train else 1) if path == "fused" else 0,
                           cell_fwd_bytes=fb, cell_bwd_bytes=bb)
                if stats and path == "fused":
                    for k, nbytes in (("fwd", fb), ("bwd", bb)):
                        if stats[k] and nbytes:      # (the stats file averages over every shape of its run: use one made with the same shapes)
                            row["cell_%s_avg_us" % k] = round(stats[k] / 1e3, 2)
                            row["cell_%s_GBps" % k] = round(nbytes / stats[k], 1)
                            row["cell_%s_of_hbm_peak" % k] = round(nbytes / stats[k] * 1e9 / HBM_PEAK, 4)
                print(json.dumps(row), flush=True)
    if set_path is not None:
        set_path("torch")


if __name__ == "__main__":
    main()
