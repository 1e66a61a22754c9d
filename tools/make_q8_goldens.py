#!/usr/bin/env python3
"""Generate tests/golden/q8_*.npz by RUNNING the reference's QuantizedLinearReparameterization and QuantizedConv2dReparameterization
(layers/variational_layers/quantize_linear_variational.py, quantize_conv_variational.py; read-only at /root/reference) on the CPU.

Runs only in the build container, like tools/make_goldens.py: the reference is imported (``termcolor`` stubbed), a seeded float layer
is converted through the reference's own ``qbnn_linear_layer`` / ``qbnn_conv_layer`` / ``batch_norm_folding``
(models/bnn_to_qbnn.py), its forward is run, and recorded are: the float parameters (and the BatchNorm's), the int8 images and their
scales, the fp32 bias tensors, the eps the layer drew (read back from ``eps_kernel`` / ``eps_weight`` and ``eps_bias``), the input,
the five (scale, zero point) pairs and the u8 image of the output. Nothing of the reference is copied.

As written, the reference's conv ``quantize()`` fails on ``delattr(self, "qint_quant")`` when ``prepare()`` never ran: this tool sets
the three attributes that ``prepare()`` would have made (``qint_quant``, ``quint_quant``, ``dequant``) to None on the float layer first.
Both forward branches are covered: the default one (``quant_dict`` None) and a hand-written ``quant_dict`` with input zero points 0
and 57. The quantised engine is fbgemm: oneDNN's dilated quantised convolution (which the default "x86" engine picks) corrupts the
heap in this torch build.

Usage:  python tools/make_q8_goldens.py
"""
import os
import sys
import types

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
torch.backends.quantized.engine = "fbgemm"


def qd(eps, mul, add, inp, out):
    return [dict(scale=s, zero_point=z) for s, z in (eps, mul, add, inp, out)]


# tag -> (kind, ctor kwargs, input shape, fold a BatchNorm, quant_dict or None, what it covers)
CASES = {
    "conv_c5x7k3p1": ("conv", dict(in_channels=5, out_channels=7, kernel_size=3, padding=1, bias=True), (2, 5, 9, 9), False, None,
                      "default branch, sampled bias, channels below one 16-block"),
    "conv_c19x10k3s2p1_z0": ("conv", dict(in_channels=19, out_channels=10, kernel_size=3, stride=2, padding=1, bias=False), (2, 19, 11, 11), False,
                             qd((0.0291, 0), (0.0011, 0), (0.0031, 0), (0.0437, 0), (0.05, 31)), "quant_dict, input zero point 0, no bias, two 16-blocks"),
    "conv_c6x5k3d2p2_z57": ("conv", dict(in_channels=6, out_channels=5, kernel_size=3, padding=2, dilation=2, bias=True), (2, 6, 10, 10), False,
                            qd((0.0291, 0), (0.0011, 0), (0.0031, 0), (0.0713, 57), (0.04, 140)), "quant_dict, input zero point 57, dilation 2"),
    "conv_c8x12k3p1_bn": ("conv", dict(in_channels=8, out_channels=12, kernel_size=3, padding=1, bias=False), (2, 8, 8, 8), True, None,
                          "default branch, BatchNorm folded into a layer without bias (sigma_b None)"),
    "conv_c8x12k3p1_bnb_z57": ("conv", dict(in_channels=8, out_channels=12, kernel_size=3, padding=1, bias=True), (2, 8, 8, 8), True,
                               qd((0.0291, 0), (0.0013, 0), (0.0052, 0), (0.0713, 57), (0.06, 120)), "quant_dict, BatchNorm folded into a biased layer"),
    "linear_70x9": ("linear", dict(in_features=70, out_features=9), (5, 70), False, None, "default branch (scale 0.2)"),
    "linear_33x10_z0": ("linear", dict(in_features=33, out_features=10), (4, 33), False,
                        qd((0.0291, 0), (0.0011, 0), (0.0031, 0), (0.0437, 0), (0.05, 31)), "quant_dict, input zero point 0"),
}


def npy(t):
    return t.detach().cpu().numpy().copy()


def run(tag, kind, kw, xshape, fold, quant_dict, what, seed):
    torch.manual_seed(seed)
    rec = {}
    if kind == "conv":
        d = RL.Conv2dReparameterization(**kw)
        wn = "kernel"
    else:
        d = RL.LinearReparameterization(**kw)
        wn = "weight"
    with torch.no_grad():
        getattr(d, "rho_" + wn).normal_(-3.0, 0.3)
        if getattr(d, "rho_bias", None) is not None:
            d.rho_bias.normal_(-3.0, 0.3)
            d.mu_bias.normal_(0.0, 0.3)
    rec["mu_w"], rec["rho_w"] = npy(getattr(d, "mu_" + wn)), npy(getattr(d, "rho_" + wn))
    has_b = getattr(d, "mu_bias", None) is not None
    if has_b:
        rec["mu_b"], rec["rho_b"] = npy(d.mu_bias), npy(d.rho_bias)
    d.qint_quant = d.quint_quant = d.dequant = None       # what prepare() would have made: the conv quantize() deletes them
    if fold:
        bn = nn.BatchNorm2d(kw["out_channels"])
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5), bn.bias.normal_(0.0, 0.2), bn.running_mean.normal_(0.0, 0.3), bn.running_var.uniform_(0.5, 2.0)
        bn.eval()
        rec["bn_weight"], rec["bn_bias"], rec["bn_mean"], rec["bn_var"], rec["bn_eps"] = npy(bn.weight), npy(bn.bias), npy(bn.running_mean), npy(bn.running_var), np.float64(bn.eps)
        q = RQ.batch_norm_folding(d, bn)
    else:
        q = RQ.qbnn_conv_layer(d) if kind == "conv" else RQ.qbnn_linear_layer(d)
    rec["q_mu"], rec["q_sigma"] = npy(q.quantized_mu_weight.int_repr()), npy(q.quantized_sigma_weight.int_repr())
    rec["s_mu"], rec["s_sigma"] = np.float64(q.quantized_mu_weight.q_scale()), np.float64(q.quantized_sigma_weight.q_scale())
    qmb, qsb = getattr(q, "quantized_mu_bias", None), getattr(q, "quantized_sigma_bias", None)
    if qmb is not None:
        rec["q_mu_b"] = npy(qmb)
    if qsb is not None:
        rec["q_sigma_b"] = npy(qsb)
    q.quant_dict = quant_dict
    x = torch.randn(xshape) * 1.5
    rec["x"] = npy(x)
    default_scale = 0.1 if kind == "conv" else 0.2
    with torch.no_grad():      # (inference; the Linear layer's bias branch re-registers a dequantised Parameter, which only works without a graph)
        out = q(x, return_kl=False)
    s_mu, s_sigma = float(rec["s_mu"]), float(rec["s_sigma"])
    if quant_dict is None:
        s_mul = s_sigma * (6 / 255)
        pairs = [(6 / 255, 0), (s_mul, 0), (max(s_mul, s_mu), 0), (default_scale, 128), (default_scale, 128)]
    else:
        pairs = [(float(e["scale"]), int(e["zero_point"])) for e in quant_dict]
    rec["pair_scales"] = np.array([p[0] for p in pairs], dtype=np.float64)
    rec["pair_zeros"] = np.array([p[1] for p in pairs], dtype=np.int32)
    rec["eps_w"] = npy(getattr(q, "eps_" + wn))
    if qmb is not None and qsb is not None:
        rec["eps_b"] = npy(q.eps_bias)
    if out.is_quantized:
        rec["out_q"] = npy(out.int_repr())
        rec["out"] = npy(out.dequantize())
    else:            # Linear dequantises: the u8 image back from out = float(oq - z) * s_out
        rec["out"] = npy(out)
        rec["out_q"] = npy(torch.round(out.double() / pairs[4][0]) + pairs[4][1]).astype(np.uint8)
    rec["what"] = np.array(what)
    path = os.path.join(OUT, f"q8_{tag}.npz")
    np.savez_compressed(path, **rec)
    u = np.unique(rec["out_q"])
    print(f"{tag}: out {rec['out_q'].shape}, {len(u)} distinct levels [{u.min()}, {u.max()}], {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for i, (tag, case) in enumerate(CASES.items()):
        run(tag, *case, seed=100 + i)
