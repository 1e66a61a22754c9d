"""ConvTranspose2d forward: the "native" path (input-dilated fetch inside the kernel) against the "upsample" path (zero-upsampled, padded
copy of x built with torch ops, then the Conv2d launch) -- DESIGN.md 4.6.

Protocol: one process, one device; per (layer, x layout, path) WARMUP calls, then N calls each timed with its own pair of HIP events
around the whole layer call (the torch ops of the materialising path included: they are part of what the path costs); median, min and
max in microseconds, and the peak bytes one call allocates (torch.cuda.max_memory_allocated delta). Layers: the U-Net upsampler
64 -> 32 k2 s2 and 64 -> 64 k4 s2 p1, both on [128, 64, 16, 16], S = 8 with shared and with stacked x.

    python tools/convt_path_bench.py [--n 200] [--warmup 20] [--paths native,upsample]

A tree without the switch (the commit before it) runs its one path under the name "upsample": that is the baseline."""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [("up 64->32 k2 s2", dict(in_channels=64, out_channels=32, kernel_size=2, stride=2)),
          ("64->64 k4 s2 p1", dict(in_channels=64, out_channels=64, kernel_size=4, stride=2, padding=1))]
XSHAPE, S = (128, 64, 16, 16), 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--paths", default="native,upsample")
    args = ap.parse_args()
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    set_path = getattr(L, "set_transpose_path", None)
    paths = [p for p in args.paths.split(",") if p == "upsample" or set_path is not None]
    torch.manual_seed(0)
    rows = []
    for lname, ctor in LAYERS:
        layer = L.ConvTranspose2dReparameterization(**ctor).cuda().eval()
        for layout in ("shared", "stacked"):
            x = torch.randn((XSHAPE[0] * (S if layout == "stacked" else 1),) + XSHAPE[1:], device="cuda")
            for path in paths:
                if set_path is not None:
                    set_path(path)
                times, peak = [], 0
                with torch.no_grad():
                    for i in range(args.warmup + args.n):
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        with mc.mc_samples(S, XSHAPE[0]):
                            out = layer(x, return_kl=False)
                        e1.record()
                        torch.cuda.synchronize()
                        if i >= args.warmup:
                            times.append(e0.elapsed_time(e1) * 1e3)
                            peak = max(peak, torch.cuda.max_memory_allocated() - base)
                        del out
                rows.append(dict(layer=lname, x=layout, path=path, kernel=layer._last["kernel"], x_path=layer._last.get("x_path", "upsample"),
                                 median_us=round(statistics.median(times), 1), min_us=round(min(times), 1), max_us=round(max(times), 1),
                                 peak_alloc_bytes=int(peak), n=len(times)))
                print(json.dumps(rows[-1]), flush=True)
    if set_path is not None:
        set_path("upsample")


if __name__ == "__main__":
    main()
