"""The hierarchical KL kernels (bt_kl_hier, bt_kl_hier_bwd) against the same formula composed of torch ops on the device, as the
reference's kl_loss() composes it -- DESIGN.md 4.6e.

Sizes: one 512 x 512 x 3 x 3 layer (2,359,296 elements), and a whole ResNet-18's weight tensors (21 segments, 11.7 M elements) in one
launch against the torch composition run layer by layer (what get_kl_loss of the reference does).

Protocol: one process, one device; WARMUP calls of each side, then the sides ALTERNATE window by window; a window is INNER back-to-back
calls between one pair of HIP events, ended by a synchronise; per-call time = window / INNER; median, min, max over N windows, in
microseconds. Bytes: the forward reads 28 B/element; the backward reads 28 and writes 16. The two sides' results are compared once at
the timed size.

Kernel times proper (the windows above include the host's per-call work, which at these sizes is of the kernels' order): a run of its
own under ``rocprofv3 --kernel-trace --stats`` with one ``--sizes`` per process.

    python tools/hier_kl_bench.py [--n 20] [--warmup 3] [--inner 10] [--sizes layer|resnet|both]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RESNET18 = [(64, 3, 7, 7)] + [(64, 64, 3, 3)] * 4 + [(128, 64, 3, 3), (128, 128, 3, 3), (128, 64, 1, 1)] + [(128, 128, 3, 3)] * 2 \
    + [(256, 128, 3, 3), (256, 256, 3, 3), (256, 128, 1, 1)] + [(256, 256, 3, 3)] * 2 + [(512, 256, 3, 3), (512, 512, 3, 3), (512, 256, 1, 1)] \
    + [(512, 512, 3, 3)] * 2 + [(1000, 512)]


def torch_kl(mu, rho, pm, la, lb, a0, b0):
    """kl_loss() of the reference's weightwise classes, op for op in torch."""
    s2 = torch.log1p(torch.exp(rho)) ** 2
    a, b = torch.exp(la), torch.exp(lb)
    e_log = torch.log(b) - torch.digamma(a)
    e_inv = a / b
    A = 0.5 * (e_log - torch.log(s2) + e_inv * (s2 + (mu - pm) ** 2) - 1)
    B = (a - a0) * torch.digamma(a) - torch.lgamma(a) + torch.lgamma(a0) + a0 * (torch.log(b) - torch.log(b0)) + (b0 - b) * e_inv
    return torch.sum(A + B)


def segment(shape, gen):
    r = lambda: torch.randn(shape, device="cuda", generator=gen)
    u = lambda: torch.rand(shape, device="cuda", generator=gen)
    return (0.1 * r(), -3 + 0.1 * r(), 0.1 * r(), 0.5 * r(), 0.5 * r(), 0.5 + 2 * u(), 0.5 + 2 * u())


def windows(sides, n, warmup, inner):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    ts = {k: [] for k in sides}
    for _ in range(n):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                r = fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / inner)
            del r
    return {k: dict(median_us=round(statistics.median(t), 2), min_us=round(min(t), 2), max_us=round(max(t), 2), n=len(t)) for k, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", choices=("layer", "resnet", "both"), default="both", help="one size per process under a kernel trace: its --stats average per kernel")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hier_kl_bench needs a GPU: a CPU run measures nothing")
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    gen = torch.Generator(device="cuda").manual_seed(0)
    g = torch.ones((), device="cuda")
    sizes = [("layer", "one layer 512x512x3x3", [(512, 512, 3, 3)]), ("resnet", "ResNet-18, 21 segments", RESNET18)]
    for name, shapes in [(n, s) for key, n, s in sizes if args.sizes in (key, "both")]:
        segs = [segment(s, gen) for s in shapes]
        n_el = sum(s[0].numel() for s in segs)
        leaves = [tuple(t.clone().requires_grad_(i in (0, 1, 3, 4)) for i, t in enumerate(s)) for s in segs]

        def torch_fwd():
            with torch.no_grad():
                kl = torch_kl(*segs[0])
                for s in segs[1:]:
                    kl = kl + torch_kl(*s)
            return kl

        def torch_fwd_bwd():
            kl = torch_kl(*leaves[0])
            for s in leaves[1:]:
                kl = kl + torch_kl(*s)
            return torch.autograd.grad(kl, [s[i] for s in leaves for i in (0, 1, 3, 4)])

        hip_fwd = lambda: _lib.kl_hier(segs, layer_ids=list(range(len(segs))), owner="hier_kl_bench")
        hip_bwd = lambda: F.kl_hier_backward(segs, g)
        hip_fwd_bwd = lambda: (hip_fwd(), hip_bwd())
        a, b = float(hip_fwd()), float(torch_fwd())
        gh, gt = hip_bwd(), torch_fwd_bwd()
        gerr = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip([t for sg in gh for t in sg], gt))
        print(json.dumps(dict(check=name, elements=n_el, kl_hip=a, kl_torch=b, rel=abs(a - b) / abs(b), grad_max_err_over_max=gerr)), flush=True)
        del gh, gt
        t = windows({"hip forward": hip_fwd, "torch forward": torch_fwd}, args.n, args.warmup, args.inner)
        t.update(windows({"hip backward": hip_bwd, "hip forward+backward": hip_fwd_bwd, "torch forward+backward": torch_fwd_bwd}, args.n, args.warmup, args.inner))
        for k, v in t.items():
            nbytes = {"hip forward": 28, "hip backward": 44, "hip forward+backward": 72}.get(k)
            extra = {} if nbytes is None else dict(GBps=round(nbytes * n_el / v["median_us"] / 1e3, 1))
            print(json.dumps(dict(what=k, size=name, elements=n_el, **v, **extra)), flush=True)
        print(json.dumps(dict(what="ratio", size=name, forward=round(t["torch forward"]["median_us"] / t["hip forward"]["median_us"], 2),
                              forward_backward=round(t["torch forward+backward"]["median_us"] / t["hip forward+backward"]["median_us"], 2))), flush=True)


if __name__ == "__main__":
    main()
