"""INT8 quantised ResNet18 against the float Bayesian ResNet18 it was converted from: ``mc_forward`` rates in one process -- DESIGN.md 4.6f.

Models (bench.py's cfg3: the harness ResNet18 via dnn_to_bnn, CIFAR 3x32x32, batch 128, S = 32, eval mode, seeded parameters):
  float         the converted model as dnn_to_bnn leaves it, on its default path (split-precision bf16x3 kernels; BatchNorm / ReLU / add
                are torch modules);
  float_fused   the same model after harness.fuse_inference (BatchNorm, ReLU and the residual add in the conv kernels' output stage):
                the benchmark's flagship form, reported for scale;
  int8          a copy converted by bnn_to_qbnn(fuse_conv_bn=True): every conv and the Linear run on the int8 MFMA forward
                (bt_q8_conv2d_fwd / bt_q8_linear_fwd), BatchNorm folded into the int8 images, ReLU / add / max-pool as torch modules,
                activations fp32 between layers.

Protocol: WARMUP calls of each model, then the models ALTERNATE over windows of at least ``--window`` seconds (whole mc_forward calls, a
synchronise at each end of a window), ``--repeats`` windows each; a rate is images x samples per second of one window. Printed: per
model the median, min and max rate over the windows, then the kernel every Bayesian layer of the int8 and the float model ran, and each
int8 layer's own time (HIP events around its launch, median of ``--n``) beside the float layer's.

``--calibrate N``: a third copy is calibrated first -- ``quantization.prepare(fuse_conv_bn=True)``, N calls of ``mc_forward`` on fresh
random batches (every layer observes all S samples' draws, its input and its output on the device), ``quantization.convert`` -- and
reported as ``int8_calibrated`` beside the default-branch ``int8``; per layer the prepared float layer's time (forward + the observer
launches in the layer's own forward; the folded BatchNorm's output is observed behind it, outside these events) beside the float
layer's, and the layer's calibrated ``quant_dict``. Calibration is not on the inference path: it runs N times per model, ever.

``--flipout``: the Flipout ResNet18 (bench.py's cfg4: the same network via dnn_to_bnn(type="Flipout"), same seeded parameters) joins the
alternation as ``float_flipout``, and its copy converted by bnn_to_qbnn(fuse_conv_bn=True, flipout=True) as ``int8_flipout``: every conv
and the Linear on the two-contraction int8 forward (bt_q8_flip_conv2d_fwd / bt_q8_flip_linear_fwd, default pairs). Per layer: the
int8 Flipout layer's time beside the float Flipout layer's and the INT8 Reparameterization layer's -- DESIGN.md 4.6h.

``--flipout --calibrate N``: a copy of the Flipout model is calibrated as well -- ``quantization.prepare(fuse_conv_bn=True, flipout=True)``,
N calls of ``mc_forward``, ``quantization.convert(fuse_conv_bn=True, flipout=True)`` -- and joins the alternation as
``int8_flipout_calibrated`` beside the default-pair ``int8_flipout`` and ``float_flipout``; per layer the float Flipout layer's time, the
prepared layer's (forward + the four observer launches) and their difference, the observers alone -- DESIGN.md 4.6i.

``--u8``: a copy of every converted model gets ``harness.resnet.u8_inference`` -- quint8 carriers from the stem to the classifier
(quantization/qact.py: the convs read and write the u8 channel-blocked image, ReLU / max-pool / add_relu run on it, fc dequantises) --
and joins the alternation as ``<model>_u8``; per layer the u8 layer's time beside the fp32-between-layers int8 layer's -- DESIGN.md 4.6k.

    python tools/bench_q8.py [--B 128] [--S 32] [--window 1.0] [--repeats 5] [--warmup 3] [--n 10] [--calibrate N] [--flipout] [--u8]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization",
         "moped_enable": False, "moped_delta": 0.5}


def window(fn, seconds):
    """Whole calls of fn for at least ``seconds`` -> (calls, elapsed seconds)."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        if n % 2 == 0 or n == 1:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    torch.cuda.synchronize()
    return n, time.perf_counter() - t0


def layer_times(net, x, S, n):
    """Per Bayesian layer: (name, kernel, median microseconds of the layer's own forward) from HIP events in forward hooks."""
    from bayesian_torch_amd import mc
    layers = [(nm, m) for nm, m in net.named_modules() if hasattr(m, "_last") and hasattr(m, "_layer_id")]
    ev = {nm: [] for nm, _ in layers}
    hooks = []
    for nm, m in layers:
        def pre(mod, inp, nm=nm):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev[nm].append([e, None])

        def post(mod, inp, out, nm=nm):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev[nm][-1][1] = e
        hooks += [m.register_forward_pre_hook(pre), m.register_forward_hook(post)]
    for _ in range(n):
        mc.mc_forward(net, x, S)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    return [(nm, m._last["kernel"], round(statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev[nm]), 1)) for nm, m in layers]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--calibrate", type=int, default=0, metavar="N", help="also calibrate a copy on N batches and report it beside the default-branch model")
    ap.add_argument("--flipout", action="store_true", help="also run the Flipout ResNet18, float and converted to the INT8 Flipout layers")
    ap.add_argument("--u8", action="store_true", help="also run every converted model with u8 activations between its layers (harness.resnet.u8_inference)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_q8 needs a GPU: a CPU run measures nothing")
    from bayesian_torch_amd import mc, rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn

    rng.set_mode("philox")
    torch.manual_seed(0)
    net = H.resnet18(10, 64)
    dnn_to_bnn(net, PRIOR)
    with torch.no_grad():
        H.fill_bayes_params(net, 1)
    net = net.cuda().eval()
    q = copy.deepcopy(net)
    bnn_to_qbnn(q, fuse_conv_bn=True)
    fused = H.fuse_inference(copy.deepcopy(net))
    models = {"float": net, "float_fused": fused, "int8": q}
    if args.flipout:
        torch.manual_seed(0)
        fnet = H.resnet18(10, 64)
        dnn_to_bnn(fnet, dict(PRIOR, type="Flipout"))
        with torch.no_grad():
            H.fill_bayes_params(fnet, 1)
        fnet = fnet.cuda().eval()
        fq = copy.deepcopy(fnet)
        bnn_to_qbnn(fq, fuse_conv_bn=True, flipout=True)
        models["float_flipout"], models["int8_flipout"] = fnet, fq
    B, S = args.B, args.S
    x = torch.randn(B, 3, 32, 32, device="cuda")
    if args.calibrate > 0:
        from bayesian_torch_amd import quantization
        cal = quantization.prepare(copy.deepcopy(net), fuse_conv_bn=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calibrate):
            mc.mc_forward(cal, torch.randn(B, 3, 32, 32, device="cuda"), S, with_kl=False)
        torch.cuda.synchronize()
        print(json.dumps(dict(what="calibration", batches=args.calibrate, B=B, S=S, seconds=round(time.perf_counter() - t0, 3))), flush=True)
        for (nm, kf, uf), (_, _, up) in zip(layer_times(net, x, S, args.n), layer_times(cal, x, S, args.n)):
            m = dict(cal.named_modules())[nm]
            print(json.dumps(dict(what="observer", layer=nm, float_us=uf, prepared_us=up, observer_us=round(up - uf, 1), observer_kernels=m._last.get("observer_kernels"))), flush=True)
        quantization.convert(cal, fuse_conv_bn=True)
        for nm, m in cal.named_modules():
            if getattr(m, "quant_dict", None) is not None:
                print(json.dumps(dict(what="quant_dict", layer=nm, pairs=[(round(d["scale"], 6), d["zero_point"]) for d in m.quant_dict])), flush=True)
        models["int8_calibrated"] = cal
        if args.flipout:
            fcal = quantization.prepare(copy.deepcopy(fnet), fuse_conv_bn=True, flipout=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calibrate):
                mc.mc_forward(fcal, torch.randn(B, 3, 32, 32, device="cuda"), S, with_kl=False)
            torch.cuda.synchronize()
            print(json.dumps(dict(what="calibration_flipout", batches=args.calibrate, B=B, S=S, seconds=round(time.perf_counter() - t0, 3))), flush=True)
            for (nm, kf, uf), (_, _, up) in zip(layer_times(fnet, x, S, args.n), layer_times(fcal, x, S, args.n)):
                m = dict(fcal.named_modules())[nm]
                print(json.dumps(dict(what="observer_flipout", layer=nm, float_flipout_us=uf, prepared_us=up, observer_us=round(up - uf, 1),
                                      observer_kernels=m._last.get("observer_kernels"))), flush=True)
            quantization.convert(fcal, fuse_conv_bn=True, flipout=True)
            for nm, m in fcal.named_modules():
                if getattr(m, "quant_dict", None) is not None:
                    print(json.dumps(dict(what="quant_dict_flipout", layer=nm, pairs=[(round(d["scale"], 6), d["zero_point"]) for d in m.quant_dict])), flush=True)
            models["int8_flipout_calibrated"] = fcal
    if args.u8:
        for k in [k for k in models if k.startswith("int8")]:
            models[k + "_u8"] = H.u8_inference(copy.deepcopy(models[k]))
    run = {k: (lambda m=m: mc.mc_forward(m, x, S, with_kl=False)) for k, m in models.items()}
    with torch.no_grad():
        for k in models:
            for _ in range(args.warmup):
                run[k]()
        rates = {k: [] for k in models}
        for _ in range(args.repeats):
            for k in models:
                n, dt = window(run[k], args.window)
                rates[k].append(n * B * S / dt)
        for k, r in rates.items():
            print(json.dumps(dict(what="mc_forward", model=k, B=B, S=S, unit="image-samples/s", median=round(statistics.median(r)), min=round(min(r)), max=round(max(r)),
                                  windows=len(r), window_s=args.window)), flush=True)
        print(json.dumps(dict(what="ratio", int8_over_float=round(statistics.median(rates["int8"]) / statistics.median(rates["float"]), 3),
                              int8_over_float_fused=round(statistics.median(rates["int8"]) / statistics.median(rates["float_fused"]), 3))), flush=True)
        if "int8_calibrated" in rates:
            print(json.dumps(dict(what="ratio", int8_calibrated_over_int8=round(statistics.median(rates["int8_calibrated"]) / statistics.median(rates["int8"]), 3))), flush=True)
        if args.flipout:
            med = lambda k: statistics.median(rates[k])
            print(json.dumps(dict(what="ratio", int8_flipout_over_float_flipout=round(med("int8_flipout") / med("float_flipout"), 3),
                                  int8_flipout_over_int8=round(med("int8_flipout") / med("int8"), 3))), flush=True)
            if "int8_flipout_calibrated" in rates:
                print(json.dumps(dict(what="ratio", int8_flipout_calibrated_over_int8_flipout=round(med("int8_flipout_calibrated") / med("int8_flipout"), 3),
                                      int8_flipout_calibrated_over_float_flipout=round(med("int8_flipout_calibrated") / med("float_flipout"), 3))), flush=True)
            for (nm, kq, uq), (_, kf, uf), (_, _, ur) in zip(layer_times(fq, x, S, args.n), layer_times(fnet, x, S, args.n), layer_times(q, x, S, args.n)):
                print(json.dumps(dict(what="layer_flipout", layer=nm, int8_flipout_us=uq, float_flipout_us=uf, int8_reparam_us=ur, int8_flipout_kernel=kq,
                                      float_flipout_kernel=kf)), flush=True)
        for k in [k for k in rates if k.endswith("_u8")]:
            base = k[:-3]
            print(json.dumps(dict(what="ratio", **{f"{k}_over_{base}": round(statistics.median(rates[k]) / statistics.median(rates[base]), 3)},
                                  base_spread=round(max(rates[base]) - min(rates[base])), median_difference=round(statistics.median(rates[k]) - statistics.median(rates[base])))),
                  flush=True)
            for (nm, ku, uu), (_, kq, uq) in zip(layer_times(models[k], x, S, args.n), layer_times(models[base], x, S, args.n)):
                print(json.dumps(dict(what="layer_u8", model=k, layer=nm, u8_us=uu, fp32_between_us=uq, u8_kernel=ku, fp32_between_kernel=kq)), flush=True)
        tq, tf = layer_times(q, x, S, args.n), layer_times(net, x, S, args.n)
        for (nm, kq, uq), (nf, kf, uf) in zip(tq, tf):
            print(json.dumps(dict(what="layer", layer=nm, int8_us=uq, float_us=uf, int8_kernel=kq, float_kernel=kf)), flush=True)


if __name__ == "__main__":
    main()
