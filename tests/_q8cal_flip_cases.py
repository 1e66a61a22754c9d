"""What the Flipout calibration tests share (tests/test_q8_flip_calib_host.py, tests/test_gpu_q8_flip_calib.py): the fixtures of
tools/make_q8cal_flip_goldens.py, the thirteen statistics computed on the host from tests/_q8_flip_model.py's ``float_flipout`` (double),
the tolerances of DESIGN.md section 4.6i, and the small conv - BatchNorm - ReLU - Linear Flipout model of the folding tests.

Tolerances: mu, eps, in, sign_in, sign_out, xp exact; sigma, delta within 8 fp32 ulps of the row's largest magnitude (section 4.6g's
rule for rows through the device softplus); mean, pert, pert_signed, out within 1e-4 of the row's largest magnitude (the forward's)."""
import os

import numpy as np
import torch
import torch.nn as nn

import _q8_flip_model as FM
import _q8cal_cases as K
from conftest import GOLD

FIXTURES = ("conv_c5x7k3p1", "linear_567x4")
ROWS = ("sigma", "mu", "eps", "delta", "add", "in", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")
PAIR_ROWS = tuple(ROWS.index(n) for n in FM.PAIRS)          # the quant_dict's ten rows, in its order
EXACT = ("mu", "eps", "in", "sign_in", "sign_out", "xp")
ULPS8 = ("sigma", "delta")
REL = ("mean", "pert", "pert_signed", "out")
REL_TOL = 1e-4
INF = float("inf")


def load(tag):
    g = np.load(os.path.join(GOLD, f"q8cal_flip_{tag}.npz"))
    return {k: torch.from_numpy(g[k]) for k in g.files}


def sgn(t):
    return torch.where(t < 0, -1.0, 1.0)


def host_stats(x, mu, rho, eps_w, sign_in, sign_out, mu_b=None, rho_b=None, eps_b=None, conv=None, coef=None, shift=None, shared_x=True):
    """The thirteen (min, max) pairs on the host. x [B, ...] shared or [S * B, ...]; eps_w [S, *w], eps_b [S, Co], sign_in [S, B, ...],
    sign_out [S, B, Co, ...]. coef / shift [Co]: the folded BatchNorm (mean = (.) * coef + shift, pert = (.) * coef; the weight rows
    those of mu * coef, sigma * coef). -> (fp32 [13, 2], {row name: largest magnitude of the row's tensor})."""
    S = eps_w.shape[0]
    f = lambda t: None if t is None else t.detach().cpu().float()
    x, mu, rho, eps_w, mu_b, rho_b, eps_b, coef, shift = map(f, (x, mu, rho, eps_w, mu_b, rho_b, eps_b, coef, shift))
    sign_in, sign_out = sgn(f(sign_in)), sgn(f(sign_out))
    B = x.shape[0] // (1 if shared_x else S)
    sigma = K.softplus_host(rho)
    sigma_b = None if rho_b is None else K.softplus_host(rho_b)
    wrows = K.host_weight_rows(mu, rho, eps_w, coef)
    tens = {k: [] for k in ROWS}
    tens["sigma"], tens["mu"], tens["eps"], tens["delta"], tens["add"] = ([wrows[k]] for k in ("sigma", "mu", "eps", "mul", "add"))
    cshape = (1, -1) + (1,) * (sign_out.dim() - 3)
    for s in range(S):
        xs = x if shared_x else x[s * B:(s + 1) * B]
        _, t = FM.float_flipout(xs, mu, sigma, eps_w[s], sign_in[s], sign_out[s], mu_b, sigma_b, None if eps_b is None else eps_b[s], conv)
        mean, pert = t["mean"], t["pert"]
        if coef is not None:
            mean = mean * coef.double().view(cshape) + shift.double().view(cshape)
            pert = pert * coef.double().view(cshape)
        ps = pert * sign_out[s].double()
        for k, v in (("in", xs), ("mean", mean), ("sign_in", sign_in[s]), ("sign_out", sign_out[s]), ("xp", t["xp"]), ("pert", pert), ("pert_signed", ps),
                     ("out", mean + ps)):
            tens[k].append(v)
    mm = torch.tensor([[min(float(v.min()) for v in tens[k]), max(float(v.max()) for v in tens[k])] for k in ROWS], dtype=torch.float64)
    mags = {k: max(float(v.abs().max()) for v in tens[k]) for k in ROWS}
    return mm, mags


def check_rows(stats, want, mags, label, rows=ROWS, skip=("add",), exact=EXACT):
    """stats: the device's [13, 2] on the CPU; want / mags: host_stats' (or recorded ranges and their magnitudes). Prints every
    deviation measured, returns {row: deviation in its own unit (ulps, or relative to the magnitude)}. ``exact``: the rows held
    exactly (a layer fed by fp32 device arithmetic the host repeats in double holds its input rows to the relative bound instead)."""
    seen = {}
    for name in rows:
        if name in skip:
            continue
        i = ROWS.index(name)
        have, ref = stats[i].double(), want[i].double()
        dev = float((have - ref).abs().max())
        if name in exact:
            assert dev == 0.0, (label, name, have.tolist(), ref.tolist())
            seen[name] = 0.0
        elif name in ULPS8:
            u = dev / (K.ulps(mags[name]) / 8)
            print(f"{label}: {name} deviates by {u:.2f} ulps of {mags[name]:.4g} (bound 8)")
            assert dev <= K.ulps(mags[name]), (label, name, have.tolist(), ref.tolist(), u)
            seen[name] = u
        else:
            rel = dev / mags[name]
            print(f"{label}: {name} deviates by {rel:.3e} of {mags[name]:.4g} (bound {REL_TOL:g})")
            assert rel <= REL_TOL, (label, name, have.tolist(), ref.tolist(), rel)
            seen[name] = rel
    return seen


def dict_of(mm):
    """[13, 2] statistics -> the ten-entry quant_dict (FM.PAIRS' order) through observer_qparams."""
    from bayesian_torch_amd.quantization import observer_qparams
    out = []
    for name, row in zip(FM.PAIRS, PAIR_ROWS):
        s, z = observer_qparams(mm[row, 0].float(), mm[row, 1].float(), torch.qint8 if name in ("eps", "delta") else torch.quint8)
        out.append(dict(scale=float(s), zero_point=int(z)))
    return out


class FoldNet(nn.Module):
    """conv(5 -> 7, 3 x 3, pad 1) - BatchNorm2d - ReLU - Flatten - Linear(7 * 6 * 6 -> 4), Flipout: ``conv1`` / ``bn1`` is a pair of the folding rules."""

    def __init__(self, L):
        super().__init__()
        self.conv1 = L.Conv2dFlipout(5, 7, 3, padding=1, bias=True)
        self.bn1 = nn.BatchNorm2d(7)
        self.relu = nn.ReLU()
        self.flatten = nn.Flatten()
        self.fc = L.LinearFlipout(7 * 6 * 6, 4)

    def forward(self, x):
        return self.fc(self.flatten(self.relu(self.bn1(self.conv1(x)))))


FOLD_SEED = 7
FOLD_BATCHES = 3


def fold_net(seed=FOLD_SEED):
    """The seeded float Flipout model (CPU, eval, BatchNorm with non-trivial running statistics), its calibration inputs [3][4, 5, 6, 6]
    and the draws of the three calibration forwards: per batch {layer: dict(eps_w [1, *w], eps_b [1, Co], sign_in [1, B, ...], sign_out)}."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = FoldNet(L)
    r = lambda *s: torch.randn(*s, generator=g)
    sg = lambda *s: sgn(torch.randn(*s, generator=g))
    with torch.no_grad():
        net.conv1.mu_kernel.copy_(r(7, 5, 3, 3) * 0.15), net.conv1.rho_kernel.copy_(-3.0 + 0.3 * r(7, 5, 3, 3))
        net.conv1.mu_bias.copy_(r(7) * 0.2), net.conv1.rho_bias.copy_(-3.0 + 0.3 * r(7))
        net.fc.mu_weight.copy_(r(4, 252) * 0.1), net.fc.rho_weight.copy_(-3.0 + 0.3 * r(4, 252))
        net.fc.mu_bias.copy_(r(4) * 0.2), net.fc.rho_bias.copy_(-3.0 + 0.3 * r(4))
        net.bn1.weight.copy_(0.5 + torch.rand(7, generator=g)), net.bn1.bias.copy_(r(7) * 0.2)
        net.bn1.running_mean.copy_(r(7) * 0.3), net.bn1.running_var.copy_(0.5 + 1.5 * torch.rand(7, generator=g))
    net.conv1.dnn_to_bnn_flag = net.fc.dnn_to_bnn_flag = True
    rng.assign_layer_ids(net)
    xs = [r(4, 5, 6, 6) * 1.3 + 0.2 for _ in range(FOLD_BATCHES)]
    draws = [dict(conv1=dict(eps_w=r(1, 7, 5, 3, 3), eps_b=r(1, 7), sign_in=sg(1, 4, 5, 6, 6), sign_out=sg(1, 4, 7, 6, 6)),
                  fc=dict(eps_w=r(1, 4, 252), eps_b=r(1, 4), sign_in=sg(1, 4, 252), sign_out=sg(1, 4, 4))) for _ in range(FOLD_BATCHES)]
    return net.eval(), xs, draws


CONV1 = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1)


def bn_affine(bn):
    """(coef, shift) of the BatchNorm as quantize() folds it: coef = weight / sqrt(var + eps), shift = bias - coef * running_mean."""
    coef = K.bn_coef(bn)
    return coef, bn.bias.detach() - coef * bn.running_mean


def float_forward(net, x, d):
    """The float model for one batch and its draws, in double on the CPU -> (BatchNorm output, logits)."""
    sp = K.softplus_host
    c, f = net.conv1, net.fc
    dc, df = d["conv1"], d["fc"]
    y, _ = FM.float_flipout(x, c.mu_kernel, sp(c.rho_kernel), dc["eps_w"][0], dc["sign_in"][0], dc["sign_out"][0], c.mu_bias, sp(c.rho_bias), dc["eps_b"][0], CONV1)
    coef, shift = bn_affine(net.bn1)
    z = y * coef.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    h = torch.relu(z).flatten(1).float()
    out, _ = FM.float_flipout(h, f.mu_weight, sp(f.rho_weight), df["eps_w"][0], df["sign_in"][0], df["sign_out"][0], f.mu_bias, sp(f.rho_bias), df["eps_b"][0], None)
    return z, out


def fold_host_stats(net, xs, draws):
    """The thirteen pairs of either layer of the FOLDED model after the calibration batches, merged over the batches -> {name: ([13, 2], mags)}."""
    out = {}
    with torch.no_grad():
        coef, shift = bn_affine(net.bn1)
        for name in ("conv1", "fc"):
            mm, mags = None, {}
            for x, d in zip(xs, draws):
                if name == "conv1":
                    c = net.conv1
                    m1, g1 = host_stats(x, c.mu_kernel, c.rho_kernel, d[name]["eps_w"], d[name]["sign_in"], d[name]["sign_out"], c.mu_bias, c.rho_bias,
                                        d[name]["eps_b"], CONV1, coef, shift)
                else:
                    f = net.fc
                    h = torch.relu(float_forward(net, x, d)[0]).flatten(1).float()
                    m1, g1 = host_stats(h, f.mu_weight, f.rho_weight, d[name]["eps_w"], d[name]["sign_in"], d[name]["sign_out"], f.mu_bias, f.rho_bias,
                                        d[name]["eps_b"], None)
                mm = m1 if mm is None else torch.stack([torch.minimum(mm[:, 0], m1[:, 0]), torch.maximum(mm[:, 1], m1[:, 1])], 1)
                mags = {k: max(v, mags.get(k, 0.0)) for k, v in g1.items()}
            out[name] = (mm, mags)
    return out
