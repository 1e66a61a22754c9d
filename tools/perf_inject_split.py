#!/usr/bin/env python3
"""Supplied draws on the split-precision kernels (rng.set_inject_path): model-level cost of the two paths, and a kernel trace.

Full-width Bayesian ResNet18 (unfused, as in the golden test), CIFAR b128, S = 8, every layer's draw injected (the on-chip draw of a
first run, materialised).  On the GPU box:
    python tools/perf_inject_split.py             device events, windows >= 0.5 s, three alternating rounds of: on-chip; inject_draw on
                                                  the path "general" / "split"; the bt_pack_eps passes alone; rng mode "torch" on
                                                  either path; torch's generator alone -> OUT/inject_split_model.json (--out OUT; default: the temporary directory)
    rocprofv3 --kernel-trace --stats --output-format csv -d out/trace -o inj -- python tools/perf_inject_split.py --trace
                                                  six on-chip forwards, then six replays on the path "split", in one trace: the inj
                                                  instantiations beside their on-chip twins in inj_kernel_stats.csv
    --flipout (with either form)                  the Flipout model: the draw holds both sign tensors, the path "split" packs them with
                                                  bt_pack_signs and launches the flip,...,inj kernels; the "pack only" column is
                                                  bt_pack_eps + the two bt_pack_signs per layer -> OUT/inject_split_flipout_model.json"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bayesian_torch_amd import rng, _lib
from bayesian_torch_amd.harness import resnet as H
from bayesian_torch_amd.mc import mc_forward
from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "moped_enable": False, "moped_delta": 0.5, "type": "Reparameterization"}
S, B = 8, 128
FLIP = "--flipout" in sys.argv[1:]


def model():
    torch.manual_seed(1)
    net = H.resnet18(10, 64)
    dnn_to_bnn(net, dict(PRIOR, type="Flipout" if FLIP else "Reparameterization"))
    H.fill_bayes_params(net, 1)
    net = net.cuda().eval()
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    return net, x, [m for _, m in H.bayes_layers(net)]


def trace():
    net, x, layers = model()
    rng.manual_seed(5)
    for _ in range(6):
        mc_forward(net, x, S)
    draws = [m.materialize_last_draw() for m in layers]
    for m, d in zip(layers, draws):
        m.inject_draw = d
    rng.set_inject_path("split")
    for _ in range(6):
        mc_forward(net, x, S)
    torch.cuda.synchronize()


def measure():
    def timeit(fn, min_s=0.5):
        fn(); torch.cuda.synchronize()
        n = 2
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record(); torch.cuda.synchronize()
            t = e0.elapsed_time(e1) / 1e3
            if t >= min_s:
                return t / n * 1e6
            n = max(2 * n, int(n * min_s / max(t, 1e-6) * 1.2) + 1)


    net, x, layers = model()
    rng.manual_seed(5)
    ref, _ = mc_forward(net, x, S)
    onchip = [m._last["kernel"] for m in layers]
    draws = [m.materialize_last_draw() for m in layers]
    res = {"S": S, "B": B, "device": torch.cuda.get_device_name(0), "onchip_kernels": onchip, "rounds": []}


    def fwd():
        mc_forward(net, x, S)


    def set_inject(on):
        for m, d in zip(layers, draws):
            m.inject_draw = d if on else None


    def pack_only():
        L = _lib.lib()
        for m, d in zip(layers, draws):
            w = d["eps_w"]
            Co, Ci = w.shape[1], w.shape[2]
            T = w[0, 0, 0].numel()
            buf = m._eps_pack.get("buf")
            if buf is None:      # (a layer whose launch was declined packs nothing)
                continue
            L.bt_pack_eps(w.data_ptr(), S, Co, Ci, T, buf.data_ptr(), _lib.stream_ptr(w.device))
            if FLIP:
                cnt = m._eps_pack["sign_count"]
                for i, key in enumerate(("sign_in", "sign_out")):
                    t = d[key]
                    L.bt_pack_signs(t.data_ptr(), S, t.numel() // S, m._eps_pack[key + "_buf"].data_ptr(), cnt.data_ptr() + 4 * i, _lib.stream_ptr(t.device))


    def torch_draws_only():
        for m in layers:
            w = m._w("mu")
            torch.empty((S,) + tuple(w.shape), device=w.device).normal_()
            if m.mu_bias is not None:
                torch.empty((S, w.shape[0]), device=w.device).normal_()
            if FLIP:
                for shp in (m._last["x_shape"], m._last["out_shape"]):
                    torch.empty((S,) + tuple(shp), device=w.device).uniform_(-1, 1).sign_()


    # correctness at the timed size
    set_inject(True)
    rng.set_inject_path("split")
    out_s, _ = mc_forward(net, x, S)
    res["split_kernels"] = [m._last["kernel"] for m in layers]
    res["split_equals_onchip_bits"] = bool(torch.equal(out_s, ref))
    res["split_max_abs_diff_vs_onchip"] = float((out_s - ref).abs().max())
    if FLIP:
        res["sign_counts"] = [[int(v) for v in m._eps_pack["sign_count"].cpu()] if "sign_count" in m._eps_pack else None for m in layers]
    rng.set_inject_path("general")
    out_g, _ = mc_forward(net, x, S)
    res["general_kernels"] = [m._last["kernel"] for m in layers]
    res["general_max_abs_diff_vs_onchip"] = float((out_g - ref).abs().max())
    res["logit_scale"] = float(ref.abs().max())

    for r in range(3):
        row = {}
        set_inject(False); rng.set_mode("philox")
        row["onchip_us"] = timeit(fwd)
        set_inject(True)
        rng.set_inject_path("general"); row["inject_general_us"] = timeit(fwd)
        rng.set_inject_path("split"); row["inject_split_us"] = timeit(fwd)
        row["pack_eps_only_us"] = timeit(pack_only)
        row["inject_split_excl_pack_us"] = row["inject_split_us"] - row["pack_eps_only_us"]
        set_inject(False); rng.set_mode("torch")
        rng.set_inject_path("general"); row["torch_mode_general_us"] = timeit(fwd)
        rng.set_inject_path("split"); row["torch_mode_split_us"] = timeit(fwd)
        row["torch_generator_only_us"] = timeit(torch_draws_only)
        rng.set_mode("philox"); rng.set_inject_path("general")
        res["rounds"].append(row)
        print(json.dumps(row), flush=True)
    argv = sys.argv[1:]
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else tempfile.gettempdir()
    os.makedirs(out_dir, exist_ok=True)
    name = "inject_split_flipout_model.json" if FLIP else "inject_split_model.json"
    json.dump(res, open(os.path.join(out_dir, name), "w"), indent=1)
    print("bits equal:", res["split_equals_onchip_bits"], "->", os.path.join(out_dir, name))


if __name__ == "__main__":
    trace() if "--trace" in sys.argv[1:] else measure()
