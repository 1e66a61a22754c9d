#!/usr/bin/env python3
"""Generate tests/golden/q8cal_flip_*.npz by RUNNING the reference's post-training calibration flow of its Flipout layers on the CPU:
``prepare()`` of a float ``Conv2dFlipout`` / ``LinearFlipout`` (four qint8 and eight quint8 QuantStubs with MinMaxObservers),
``torch.quantization.prepare``, three calibration batches, ``torch.quantization.convert``. The flow runs as the reference writes it.

Runs only where the reference is installed, like tools/make_q8cal_goldens.py: it is imported (``termcolor`` stubbed) at generation time
from the directory given as the first argument (or ``BT_REFERENCE_ROOT``); nothing of it is copied. Recorded per fixture: the float
parameters, the three inputs, the draws of the three forwards (eps read back from ``eps_kernel`` / ``eps_weight`` and ``eps_bias``, the
two sign tensors caught by forward pre-hooks on ``quint_quant[2]`` and ``quint_quant[3]``), the twelve observers' (min, max) as
``minmax13`` in ``functional.CALIB_FLIP_ROWS``' order (row "add", which the reference does not observe, stays (+inf, -inf)), the twelve
(scale, zero point) likewise, and the ten-entry selection in ``functional.Q8_FLIP_PAIRS``' order.

The seed of a fixture is the first one from its base for which no recorded quint8 zero point of a row that is computed within a
tolerance (mean, pert, pert_signed, out) sits near a rounding tie: min / scale at least 1e-3 away from a half-integer, so that a one-ulp
difference in a scale cannot move a zero point. The rows reproduced exactly (in, xp, sign_in, sign_out) give the recorded scale bit
for bit; the sign rows' argument, -1 / (2 / 255) = -127.5, is a tie by construction.

Usage:  python tools/make_q8cal_flip_goldens.py REFERENCE_ROOT
"""
import os
import sys
import types
import warnings

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BT_REFERENCE_ROOT")
if not REFERENCE or not os.path.isdir(REFERENCE):
    sys.exit("usage: make_q8cal_flip_goldens.py REFERENCE_ROOT (the directory that holds the reference's bayesian_torch package)")
sys.path.insert(0, REFERENCE)
_tc = types.ModuleType("termcolor")
_tc.colored = lambda s, *a, **k: s
sys.modules["termcolor"] = _tc

import numpy as np
import torch
import torch.nn as nn

import bayesian_torch.layers as RL                       # the reference

OUT = os.path.join(REPO, "tests", "golden")
torch.set_num_threads(4)
warnings.simplefilter("ignore")

# tag -> (kind, ctor kwargs, input shape, input scale and shift)
CASES = {
    "conv_c5x7k3p1": ("conv", dict(in_channels=5, out_channels=7, kernel_size=3, padding=1, bias=True), (2, 5, 9, 9), (1.5, 0.4)),
    "linear_567x4": ("linear", dict(in_features=567, out_features=4), (5, 567), (1.2, -0.3)),
}
BATCHES = 3
ROWS = ("sigma", "mu", "eps", "delta", "add", "in", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")
PAIRS = ("eps", "delta", "in", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")
TIE_MARGIN = 1e-3


def npy(t):
    return t.detach().cpu().numpy().copy()


def run(kind, kw, xshape, xdist, seed):
    torch.manual_seed(seed)
    d = RL.Conv2dFlipout(**kw) if kind == "conv" else RL.LinearFlipout(**kw)
    wn = "kernel" if kind == "conv" else "weight"
    with torch.no_grad():
        getattr(d, "rho_" + wn).normal_(-3.0, 0.3)
        d.rho_bias.normal_(-3.0, 0.3)
        d.mu_bias.normal_(0.0, 0.3)
    rec = dict(mu_w=npy(getattr(d, "mu_" + wn)), rho_w=npy(getattr(d, "rho_" + wn)), mu_b=npy(d.mu_bias), rho_b=npy(d.rho_bias), seed=np.array(seed))
    d.prepare()
    d.dnn_to_bnn_flag = True
    model = nn.Sequential(d).eval()
    model.qconfig = torch.quantization.get_default_qconfig("fbgemm")
    model = torch.quantization.prepare(model)      # (a copy: the observers hang on ITS stubs)
    d = model[0]
    signs = {2: [], 3: []}
    hooks = [d.quint_quant[i].register_forward_pre_hook(lambda m, args, i=i: signs[i].append(npy(args[0]))) for i in (2, 3)]
    xs, ews, ebs = [], [], []
    with torch.no_grad():
        for _ in range(BATCHES):
            x = torch.randn(xshape) * xdist[0] + xdist[1]
            model(x)
            xs.append(npy(x)), ews.append(npy(getattr(d, "eps_" + wn))), ebs.append(npy(d.eps_bias))
    for h in hooks:
        h.remove()
    rec["x"], rec["eps_w"], rec["eps_b"] = np.stack(xs), np.stack(ews), np.stack(ebs)
    rec["sign_in"], rec["sign_out"] = np.stack(signs[2]), np.stack(signs[3])
    assert bool((np.abs(rec["sign_in"]) == 1.0).all()) and bool((np.abs(rec["sign_out"]) == 1.0).all())
    at = lambda stubs, get: [get(s) for s in stubs[:4]] + [None] + [get(s) for s in stubs[4:]]      # twelve stubs -> thirteen rows
    stubs = list(d.qint_quant) + list(d.quint_quant)            # sigma, mu, eps, delta; in, mean, sign_in, sign_out, xp, pert, pert_signed, out
    mm = at(stubs, lambda s: [float(s.activation_post_process.min_val), float(s.activation_post_process.max_val)])
    rec["minmax13"] = np.array([[np.inf, -np.inf] if v is None else v for v in mm], dtype=np.float32)
    model = torch.quantization.convert(model)
    d = model[0]
    stubs = list(d.qint_quant) + list(d.quint_quant)
    rec["scales13"] = np.array([0.0 if v is None else v for v in at(stubs, lambda s: float(s.scale.float()))], dtype=np.float32)
    rec["zero_points13"] = np.array([0 if v is None else v for v in at(stubs, lambda s: int(s.zero_point))], dtype=np.int32)
    take = [ROWS.index(n) for n in PAIRS]
    rec["dict_scales"], rec["dict_zero_points"] = rec["scales13"][take], rec["zero_points13"][take]
    # distance of every affine zero point's argument from a rounding tie, for the rows a device computes within a tolerance (in, xp and
    # the two sign rows are reproduced exactly, scale included; the sign rows' -1 / (2 / 255) = -127.5 IS a tie, decided alike everywhere)
    margin = 1.0
    for n in ("mean", "pert", "pert_signed", "out"):
        i = ROWS.index(n)
        q = min(float(rec["minmax13"][i, 0]), 0.0) / float(rec["scales13"][i])
        margin = min(margin, abs(abs(q - np.floor(q)) - 0.5))
    return rec, margin


if __name__ == "__main__":
    for i, (tag, case) in enumerate(CASES.items()):
        seed = 400 + 100 * i
        while True:
            rec, margin = run(*case, seed=seed)
            if margin >= TIE_MARGIN:
                break
            seed += 1
        assert margin >= TIE_MARGIN
        path = os.path.join(OUT, f"q8cal_flip_{tag}.npz")
        np.savez_compressed(path, **rec)
        print(f"{tag}: seed {seed}, tie margin {margin:.4f}, {os.path.getsize(path)} bytes")
        print("   quant_dict", [(round(float(s), 6), int(z)) for s, z in zip(rec["dict_scales"], rec["dict_zero_points"])])
        print("   minmax13", rec["minmax13"].tolist())
