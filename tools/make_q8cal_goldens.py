#!/usr/bin/env python3
"""Generate tests/golden/q8cal_*.npz by RUNNING the reference's post-training calibration flow on the CPU: ``prepare()`` of a float
``Conv2dReparameterization`` / ``LinearReparameterization`` (seven QuantStubs with MinMaxObservers), ``torch.quantization.prepare``,
three calibration batches, ``torch.quantization.convert`` and the ``quant_dict`` selection of ``models/bnn_to_qbnn.py:105-111`` /
``:132-138``.

Runs only in the build container, like tools/make_q8_goldens.py: the reference is imported (``termcolor`` stubbed) at generation time,
nothing of it is copied. Recorded per fixture: the float parameters, the three inputs, the draws of the three forwards (read back from
``eps_kernel`` / ``eps_weight`` and ``eps_bias``), every observer's (min, max) in the order sigma, mu, eps, mul, add, in, out, the
(scale, zero point) each stub was converted to, and the five-entry ``quant_dict`` (eps, mul, add, in, out).

The ``quant_dict`` is the one the reference's own ``qbnn_conv_layer`` / ``qbnn_linear_layer`` leaves on the converted layer.

Usage:  python tools/make_q8cal_goldens.py
"""
import os
import sys
import types
import warnings

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")
_tc = types.ModuleType("termcolor")
_tc.colored = lambda s, *a, **k: s
sys.modules["termcolor"] = _tc

import numpy as np
import torch
import torch.nn as nn

import bayesian_torch.layers as RL                       # the reference
from bayesian_torch.models import bnn_to_qbnn as RQ      # the reference

OUT = os.path.join(REPO, "tests", "golden")
torch.set_num_threads(4)
warnings.simplefilter("ignore")

# tag -> (kind, ctor kwargs, input shape, input scale and shift)
CASES = {
    "conv_c5x7k3p1": ("conv", dict(in_channels=5, out_channels=7, kernel_size=3, padding=1, bias=True), (2, 5, 9, 9), (1.5, 0.4)),
    "linear_567x4": ("linear", dict(in_features=567, out_features=4), (5, 567), (1.2, -0.3)),
}
BATCHES = 3


def npy(t):
    return t.detach().cpu().numpy().copy()


def run(tag, kind, kw, xshape, xdist, seed):
    torch.manual_seed(seed)
    d = RL.Conv2dReparameterization(**kw) if kind == "conv" else RL.LinearReparameterization(**kw)
    wn = "kernel" if kind == "conv" else "weight"
    with torch.no_grad():
        getattr(d, "rho_" + wn).normal_(-3.0, 0.3)
        d.rho_bias.normal_(-3.0, 0.3)
        d.mu_bias.normal_(0.0, 0.3)
    rec = dict(mu_w=npy(getattr(d, "mu_" + wn)), rho_w=npy(getattr(d, "rho_" + wn)), mu_b=npy(d.mu_bias), rho_b=npy(d.rho_bias))
    d.prepare()
    d.dnn_to_bnn_flag = True
    model = nn.Sequential(d).eval()
    model.qconfig = torch.quantization.get_default_qconfig("fbgemm")
    model = torch.quantization.prepare(model)      # (a copy: the observers hang on ITS stubs)
    d = model[0]
    xs, ews, ebs, outs = [], [], [], []
    with torch.no_grad():
        for _ in range(BATCHES):
            x = torch.randn(xshape) * xdist[0] + xdist[1]
            outs.append(npy(model(x)))
            xs.append(npy(x)), ews.append(npy(getattr(d, "eps_" + wn))), ebs.append(npy(d.eps_bias))
    rec["x"], rec["eps_w"], rec["eps_b"] = np.stack(xs), np.stack(ews), np.stack(ebs)
    stubs = list(d.qint_quant) + list(d.quint_quant)            # sigma, mu, eps, mul, add, in, out
    rec["minmax"] = np.array([[float(s.activation_post_process.min_val), float(s.activation_post_process.max_val)] for s in stubs], dtype=np.float32)
    rec["out_minmax_of_outputs"] = np.array([min(o.min() for o in outs), max(o.max() for o in outs)], dtype=np.float32)
    model = torch.quantization.convert(model)
    d = model[0]
    stubs = list(d.qint_quant) + list(d.quint_quant)
    rec["scales"] = np.array([float(s.scale.float()) for s in stubs], dtype=np.float32)
    rec["zero_points"] = np.array([int(s.zero_point) for s in stubs], dtype=np.int32)
    q = RQ.qbnn_conv_layer(d) if kind == "conv" else RQ.qbnn_linear_layer(d)      # the reference's converter: its quant_dict selection
    quant_dict = list(q.quant_dict)
    assert len(quant_dict) == 5
    rec["dict_scales"] = np.array([float(e["scale"]) for e in quant_dict], dtype=np.float32)
    rec["dict_zero_points"] = np.array([int(e["zero_point"]) for e in quant_dict], dtype=np.int32)
    path = os.path.join(OUT, f"q8cal_{tag}.npz")
    np.savez_compressed(path, **rec)
    print(f"{tag}: quant_dict {[(round(float(s), 6), int(z)) for s, z in zip(rec['dict_scales'], rec['dict_zero_points'])]}, {os.path.getsize(path)} bytes")
    print("   minmax", rec["minmax"].tolist())


if __name__ == "__main__":
    for i, (tag, case) in enumerate(CASES.items()):
        run(tag, *case, seed=300 + i)
