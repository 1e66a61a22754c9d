"""Conv3d forward: the "native" path (depth-window fetch inside the kernel) against the "unfold" path (depth-unfolded copy of x built with
torch ops, then the Conv2d launch) -- DESIGN.md 4.6b.

Protocol (tools/convt_path_bench.py's): one process, one device; per (layer, x layout, path) WARMUP calls, then N calls each timed with
its own pair of HIP events around the whole layer call (the torch ops of the unfolding path and the output's re-arrangement included:
they are part of what a path costs); median, min and max in microseconds, and the peak bytes one call allocates
(torch.cuda.max_memory_allocated delta). Layers: two 3x3x3 video-block layers 32 -> 32 on [16, 32, 8, 28, 28] (depth stride 1 and 2) and
the one-channel stem 1 -> 32 k(3,7,7) s(1,2,2) on [16, 1, 8, 56, 56], whose unfolded launch is the stem kernel's and whose window launch
is the fp32 general kernel's; S = 8 with shared and with stacked x.

    python tools/conv3d_path_bench.py [--n 200] [--warmup 20] [--paths native,unfold]

A tree without the switch (the commit before it) runs its one path under the name "unfold": that is the baseline."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_PRI = dict(prior_mean=0.0, prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0)
LAYERS = [("32->32 k3 p1", dict(in_channels=32, out_channels=32, kernel_size=3, padding=1, **_PRI), (16, 32, 8, 28, 28)),
          ("32->32 k3 s(2,1,1) p1", dict(in_channels=32, out_channels=32, kernel_size=3, stride=(2, 1, 1), padding=1, **_PRI), (16, 32, 8, 28, 28)),
          ("stem 1->32 k(3,7,7) s(1,2,2)", dict(in_channels=1, out_channels=32, kernel_size=(3, 7, 7), stride=(1, 2, 2), padding=(1, 3, 3), **_PRI),
           (16, 1, 8, 56, 56))]
S = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--paths", default="native,unfold")
    args = ap.parse_args()
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    set_path = getattr(L, "set_conv3d_path", None)
    paths = [p for p in args.paths.split(",") if p == "unfold" or set_path is not None]
    torch.manual_seed(0)
    rows = []
    for lname, ctor, xshape in LAYERS:
        layer = L.Conv3dReparameterization(**ctor).cuda().eval()
        for layout in ("shared", "stacked"):
            x = torch.randn((xshape[0] * (S if layout == "stacked" else 1),) + xshape[1:], device="cuda")
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
                        with mc.mc_samples(S, xshape[0]):
                            out = layer(x, return_kl=False)
                        e1.record()
                        torch.cuda.synchronize()
                        if i >= args.warmup:
                            times.append(e0.elapsed_time(e1) * 1e3)
                            peak = max(peak, torch.cuda.max_memory_allocated() - base)
                        del out
                rows.append(dict(layer=lname, x=layout, path=path, kernel=layer._last["kernel"], x_path=layer._last.get("x_path", "unfold"),
                                 median_us=round(statistics.median(times), 1), min_us=round(min(times), 1), max_us=round(max(times), 1),
                                 peak_alloc_bytes=int(peak), n=len(times)))
                print(json.dumps(rows[-1]), flush=True)
    if set_path is not None:
        set_path("unfold")


if __name__ == "__main__":
    main()
