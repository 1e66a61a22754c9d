"""Conv2dReparameterization_Multivariate: ``mc_forward`` on the kernels (in-kernel low-rank source, mean pre-pass, KL kernels) against the
same call forced onto the materialising torch path (``layer.force_path = "materialised"``) -- DESIGN.md 4.6d.

Model (tests/test_gpu_lowrank.py's, at a size a user would run): multivariate conv 3 -> 16, k3 p1, rank 432 (the full-rank stem) - ReLU -
multivariate conv 16 -> 16, k3 s2 p1, rank 1 - ReLU - global average pool - LinearReparameterization(16, 10); x [128, 3, 32, 32], S = 32.

Protocol: one process, one device; WARMUP calls of each path, then the two paths ALTERNATE call by call, each call timed with its own pair
of HIP events around the whole ``mc_forward`` and a synchronise; median, min, max in microseconds. Then the fused path's stages, each timed
the same way on the same shapes: the stem's mean pre-pass, its forward launch, its KL (sweep + factorisation at r = 432), and the second
layer's forward launch and KL. The outputs of the two paths are compared once at the timed size (same draws: same coordinates).

    python tools/lowrank_path_bench.py [--n 30] [--warmup 5] [--B 128] [--S 32] [--hw 32]

``--train`` runs the training leg instead: forward + ``(out * g).sum() + kl`` + backward of the same model at S = 1 and at S, under
``set_lowrank_train_path("fused")`` (the inference launches and the HIP backward of csrc/bt_lowrank_bwd.hip) against ``"materialised"`` (the
torch composition under autograd), alternating call by call after WARMUP calls of each, the same timing; the gradients of the two paths are
compared once per S (same coordinates: same draws); then the fused backward's stages at S.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, n, warmup):
    ts = []
    for i in range(warmup + n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1) * 1e3)
        del r
    return dict(median_us=round(statistics.median(ts), 1), min_us=round(min(ts), 1), max_us=round(max(ts), 1), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--hw", type=int, default=32)
    ap.add_argument("--train", action="store_true", help="the training leg: fused against materialised training steps")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lowrank_path_bench needs a GPU: a CPU run measures nothing")
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd import mc, rng
    from bayesian_torch_amd.layers import LinearReparameterization
    from bayesian_torch_amd.layers.variational_layers.conv_variational import Conv2dReparameterization_Multivariate as M

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = M(3, 16, 3, padding=1, rank=432)
            self.conv2 = M(16, 16, 3, stride=2, padding=1, rank=1)
            self.fc = LinearReparameterization(16, 10)

        def forward(self, x):
            x = torch.relu(self.conv1(x, return_kl=False))
            x = torch.relu(self.conv2(x, return_kl=False))
            return self.fc(x.mean((2, 3)), return_kl=False)

    rng.set_mode("philox")
    torch.manual_seed(0)
    net = Net()
    rng.assign_layer_ids(net)
    net = net.cuda().eval()
    B, S = args.B, args.S
    x = torch.randn(B, 3, args.hw, args.hw, device="cuda")
    convs = (net.conv1, net.conv2)

    if args.train:
        return train_leg(args, net, x, convs, F, mc, rng)

    def run(path):
        for c in convs:
            c.force_path = path
        return mc.mc_forward(net, x, S)

    # same draws on both paths: the outputs agree at the timed size
    c0 = rng.peek_call()
    a, ka = run(None)
    rng.set_call(c0)
    b, kb = run("materialised")
    err = float((a - b).abs().max()) / float(b.abs().max())
    print(json.dumps(dict(check="fused vs materialised at the timed size", max_err_over_max=err, kl_fused=float(ka), kl_materialised=float(kb),
                          paths=[c._last["path"] for c in convs])), flush=True)
    del a, b
    for p in (None, "materialised"):
        for _ in range(args.warmup):
            run(p)
    ts = {None: [], "materialised": []}
    for i in range(args.n):
        for p in (None, "materialised"):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = run(p)
            e1.record()
            torch.cuda.synchronize()
            ts[p].append(e0.elapsed_time(e1) * 1e3)
            del r
    for p, name in ((None, "fused"), ("materialised", "materialised")):
        t = ts[p]
        print(json.dumps(dict(what="mc_forward", path=name, B=B, S=S, hw=args.hw, median_us=round(statistics.median(t), 1), min_us=round(min(t), 1),
                              max_us=round(max(t), 1), n=len(t))), flush=True)
    for c in convs:
        c.force_path = None
    # the fused path's stages
    c1, c2 = convs
    d = float(c1.D_param[0])
    conv1, conv2 = c1._conv_desc(), c2._conv_desc()
    with torch.no_grad():
        mean = F.lowrank_mean(c1.mu_kernel, c1.L_param, S)
        h = torch.relu(F.lowrank_conv2d(x, mean, None, d, c1._wshape(), conv1, S=S))
        stages = [
            ("stem mean pre-pass (r=432, n=432)", lambda: F.lowrank_mean(c1.mu_kernel, c1.L_param, S)),
            ("stem forward launch (R=0)", lambda: F.lowrank_conv2d(x, mean, None, d, c1._wshape(), conv1, S=S)),
            ("stem KL: sweep + factorisation (r=432)", lambda: F.kl_lowrank(c1.mu_kernel, c1.L_param, d, c1.prior_mean, c1.prior_cov_D)),
            ("layer 2 forward launch (R=1, in-kernel)", lambda: F.lowrank_conv2d(h, c2.mu_kernel, c2.L_param, d, c2._wshape(), conv2, S=S, shared_x=False)),
            ("layer 2 KL (r=1, n=2304)", lambda: F.kl_lowrank(c2.mu_kernel, c2.L_param, d, c2.prior_mean, c2.prior_cov_D)),
        ]
        for name, fn in stages:
            print(json.dumps(dict(what="stage", stage=name, **timed(fn, args.n, args.warmup))), flush=True)


def train_leg(args, net, x, convs, F, mc, rng):
    import bayesian_torch_amd.layers as BL
    c1, c2 = convs
    B = args.B
    params = [p for p in net.parameters()]

    def step(path, S, g):
        BL.set_lowrank_train_path(path)
        for p in params:
            p.grad = None
        with mc.mc_samples(S, B):
            h, k1 = c1(x)
            h, k2 = c2(torch.relu(h))
            out, k3 = net.fc(torch.relu(h).mean((2, 3)))
        ((out * g).sum() + k1 + k2 + k3).backward()
        return out

    for S in sorted({1, args.S}):
        g = torch.randn(S * B, 10, device="cuda")
        c0 = rng.peek_call()
        grads, ran = {}, {}
        for path in ("fused", "materialised"):
            rng.set_call(c0)
            step(path, S, g)
            grads[path] = [p.grad.clone() for p in params]
            ran[path] = [c._last["backward"] for c in convs]
        err = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(grads["fused"], grads["materialised"]))
        print(json.dumps(dict(check="fused vs materialised gradients", S=S, max_err_over_max=err, backward=ran)), flush=True)
        del grads
        for path in ("fused", "materialised"):
            for _ in range(args.warmup):
                step(path, S, g)
        ts = {"fused": [], "materialised": []}
        for i in range(args.n):
            for path in ("fused", "materialised"):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = step(path, S, g)
                e1.record()
                torch.cuda.synchronize()
                ts[path].append(e0.elapsed_time(e1) * 1e3)
                del r
        for path, t in ts.items():
            print(json.dumps(dict(what="training step", path=path, B=B, S=S, hw=args.hw, median_us=round(statistics.median(t), 1), min_us=round(min(t), 1),
                                  max_us=round(max(t), 1), n=len(t))), flush=True)
    BL.set_lowrank_train_path("materialised")
    # the fused backward's stages at S
    S = args.S
    d = float(c1.D_param[0])
    conv1, conv2 = c1._conv_desc(), c2._conv_desc()
    one = torch.ones(1, device="cuda")
    with torch.no_grad():
        mean = F.lowrank_mean(c1.mu_kernel, c1.L_param, S)
        h = torch.relu(F.lowrank_conv2d(x, mean, None, d, c1._wshape(), conv1, S=S))
        h2 = F.lowrank_conv2d(h, c2.mu_kernel, c2.L_param, d, c2._wshape(), conv2, S=S, shared_x=False)
        g1, g2 = torch.randn_like(h), torch.randn_like(h2)
        dw1 = F.lowrank_backward(x, g1, mean, None, d, c1._wshape(), conv1, S=S, need_x=False)[1]
        dw2 = F.lowrank_backward(h, g2, c2.mu_kernel, c2.L_param, d, c2._wshape(), conv2, S=S, shared_x=False)[1]
        stages = [
            ("stem weight gradient, per sample (x is a leaf: no data gradient)", lambda: F.lowrank_backward(x, g1, mean, None, d, c1._wshape(), conv1, S=S, need_x=False)),
            ("stem finishing pass (r=432, n=432)", lambda: F.lowrank_wgrad_finish(dw1, 432)),
            ("stem KL gradient (r=432): sweep, factor, inverses, gradient", lambda: F.kl_lowrank_backward(c1.mu_kernel, c1.L_param, d, c1.prior_mean, c1.prior_cov_D, one)),
            ("layer 2 data + weight gradient (R=1, in-kernel)", lambda: F.lowrank_backward(h, g2, c2.mu_kernel, c2.L_param, d, c2._wshape(), conv2, S=S, shared_x=False)),
            ("layer 2 data gradient alone", lambda: F.lowrank_backward(h, g2, c2.mu_kernel, c2.L_param, d, c2._wshape(), conv2, S=S, shared_x=False, need_w=False)),
            ("layer 2 finishing pass (r=1, n=2304)", lambda: F.lowrank_wgrad_finish(dw2, 1)),
            ("layer 2 KL gradient (r=1, n=2304)", lambda: F.kl_lowrank_backward(c2.mu_kernel, c2.L_param, d, c2.prior_mean, c2.prior_cov_D, one)),
        ]
        for name, fn in stages:
            print(json.dumps(dict(what="stage", stage=name, S=S, **timed(fn, args.n, args.warmup))), flush=True)


if __name__ == "__main__":
    main()
