"""What the q8 Flipout host and GPU tests share: the layer cases (geometry x pairs x bias form), each with its input, S draws of four
tensors and the model's answer (tests/_q8_flip_model.py), computed once on the CPU and never modified."""
import functools
import math
import zlib

import torch

import _q8_edges as E
import _q8_flip_model as FM

S_MU, S_SIGMA = 0.003, 0.0009                                  # the scales of the random int8 images

C3 = lambda s, p, d: dict(stride=(s, s), padding=(p, p), dilation=(d, d), groups=1)
# name -> (weight shape, x shape, conv or None)
GEOMS = {
    "conv_c37x70k3p1_9x7": ((70, 37, 3, 3), (3, 37, 9, 7), C3(1, 1, 1)),       # 189 pixels, 70 channels: both tile edges; 27 units: a partial last stage
    "conv_c5x6k3s2d2p2_8x5": ((6, 5, 3, 3), (2, 5, 8, 5), C3(2, 2, 2)),
    "conv_c20x6k3p1_1x1": ((6, 20, 3, 3), (5, 20, 1, 1), C3(1, 1, 1)),         # eight of nine taps read padding only
    "linear_70x10_b3": ((10, 70), (3, 70), None),
}


def _edge_geom(name):
    (KH, KW, H, W, *_), Ci, Co, B, _ = E.GEOMS[name]
    return (Co, Ci, KH, KW), (B, Ci, H, W), E.geom_conv(name)


# The walk's hard geometries, which the Reparameterization kernel sees in tests/test_gpu_q8_edges.py (tests/_q8_edges.py, F): both
# chains run on one walk (csrc/bt_q8_common.h), so both are held to them.
EDGE_GEOMS = ("k3x5_2x7_uneven", "k4x4_2x1_s2p3", "k5x5_2x2_p2", "k2x8_3x2_p1x7", "k3x3_1x5")
GEOMS.update({name: _edge_geom(name) for name in EDGE_GEOMS})


def pruned(c):
    """Whether the kernel prunes the taps of case c: both activations' zero points 128, at most 16 taps, a tap that reads padding only."""
    wshape, xshape, conv = GEOMS[c["name"]]
    return conv is not None and c["pairs"][FM.XP][1] == 128 and E.walked_taps(conv, wshape, xshape, c["pairs"][FM.IN][1])[1]


def pairs_of(kind, K):
    """The ten pairs of a case. 'default': the default branch's. 'dict': a calibrated-style set with every zero point != 128 whose
    intermediates span their ranges. 'dict_xp120': 'default' but for z_xp = 120 (taps must not be pruned). 'clamps': 'dict' with the
    four result scales cut so that o1, p, p' and oq reach both clamp ends, and with sign scales whose reciprocals are exact ties
    (0.4 -> 2.5, 2 / 3 -> 1.5). 'ties': 'default' with the signs, x' and p' at scale 0.2 -- the signs quantise to 128 +- 5 and both umul
    multipliers are 0.1, so every odd operand is a tie, which the fp32 multiplier f32(0.1) * f32(0.2) * (1 / f32(0.2)) and the double
    quotient's f32(0.1) decide differently."""
    r = math.sqrt(K)
    if kind == "default":
        return FM.scales_default(S_SIGMA)
    if kind == "dict_xp120":
        p = FM.scales_default(S_SIGMA)
        p[FM.XP] = (0.1, 120)
        return p
    if kind == "ties":
        p = FM.scales_default(S_SIGMA)
        for i in (FM.SIGN_IN, FM.SIGN_OUT, FM.XP, FM.PERT_SIGNED):
            p[i] = (0.2, 128)
        return p
    if kind == "dict":
        return [(0.0291, 0), (0.0031, 0), (0.05, 120), (0.008 * r, 117), (0.01, 100), (0.02, 77), (0.05, 131), (0.0045 * r, 140), (0.0045 * r, 119), (0.011 * r, 121)]
    if kind == "clamps":
        return [(0.0291, 0), (0.0031, 0), (0.05, 120), (0.002 * r, 117), (0.4, 100), (2 / 3, 77), (0.04, 131), (0.0012 * r, 140), (0.0006 * r, 119), (0.002 * r, 121)]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case(name, kind="dict", bias="full", S=1, x_std=1.5):
    wshape, xshape, conv = GEOMS[name]
    g = torch.Generator().manual_seed(zlib.crc32(repr((name, kind, bias, S, x_std)).encode()))
    q_mu = torch.randint(-128, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
    q_sigma = torch.randint(0, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
    K = math.prod(wshape[1:])
    pairs = pairs_of(kind, K)
    x = torch.randn((S,) + xshape, generator=g) * x_std          # per-sample inputs; x[0] is the shared one
    Co = wshape[0]
    s_b = pairs[FM.MEAN][0]
    mu_b = torch.randn(Co, generator=g) * (3.0 * s_b) if bias != "none" else None
    sigma_b = torch.rand(Co, generator=g) * (2.0 * pairs[FM.PERT][0]) if bias == "full" else None
    eps_w = torch.randn((S,) + wshape, generator=g)
    eps_b = torch.randn((S, Co), generator=g) if bias == "full" else None
    sign_in = torch.randint(0, 2, (S,) + xshape, generator=g).float() * 2 - 1
    ref0 = FM.forward(x[0], q_mu, q_sigma, S_MU, S_SIGMA, pairs, eps_w[0], sign_in[0], torch.ones(1), mu_b, sigma_b, None if eps_b is None else eps_b[0], conv)
    oshape = tuple(ref0[0].shape)
    sign_out = torch.randint(0, 2, (S,) + oshape, generator=g).float() * 2 - 1
    c = dict(name=name, q_mu=q_mu, q_sigma=q_sigma, x=x, pairs=pairs, mu_b=mu_b, sigma_b=sigma_b, eps_w=eps_w, eps_b=eps_b, sign_in=sign_in, sign_out=sign_out,
             conv=conv, wshape=wshape, S=S)
    return c


def model(c, shared_x=True, mul=FM.umul, add=FM.uadd):
    """The model's answer for every sample of a case -> (u8 [S * B, ...], fp32, the list of per-sample intermediates)."""
    key = (id(c), shared_x, mul, add)
    if key not in _MODEL:
        ref = [FM.forward(c["x"][0 if shared_x else s], c["q_mu"], c["q_sigma"], S_MU, S_SIGMA, c["pairs"], c["eps_w"][s], c["sign_in"][s], c["sign_out"][s], c["mu_b"],
                          c["sigma_b"], None if c["eps_b"] is None else c["eps_b"][s], c["conv"], mul=mul, add=add) for s in range(c["S"])]
        _MODEL[key] = (torch.cat([r[0] for r in ref], 0), torch.cat([r[1] for r in ref], 0), [r[2] for r in ref], c)      # (c: keeps id(c) alive)
    return _MODEL[key][:3]


_MODEL = {}

# (name, kind, bias, x_std): the layer cases the host test holds to torch's operator chain and the GPU test runs
LAYER_CASES = [
    ("conv_c37x70k3p1_9x7", "dict", "full", 1.5),
    ("conv_c37x70k3p1_9x7", "default", "mu_only", 8.0),        # |x| past 12.8: xq = 0 under a negative sign makes x' = 256 -> 255
    ("conv_c37x70k3p1_9x7", "clamps", "none", 1.5),
    ("conv_c5x6k3s2d2p2_8x5", "dict", "full", 1.5),
    ("conv_c5x6k3s2d2p2_8x5", "clamps", "mu_only", 1.5),
    ("conv_c5x6k3s2d2p2_8x5", "ties", "full", 4.0),
    ("conv_c20x6k3p1_1x1", "default", "full", 8.0),
    ("conv_c20x6k3p1_1x1", "dict_xp120", "full", 8.0),
    ("linear_70x10_b3", "dict", "full", 1.5),
    ("linear_70x10_b3", "default", "none", 8.0),
    ("linear_70x10_b3", "clamps", "mu_only", 1.5),
]

# (name, kind, bias, x_std) on the edge geometries, supplied draws, S = 1: pruned taps and, with the 'dict' pairs, padding corrected
# through both row sums; 25 taps (no pruning) with the default pairs: padding a true zero in both contractions; a pixel tile that
# crosses images, so that both sign offsets cross an image boundary inside one workgroup. x_std 1.5 spreads x over +-15 levels of the
# default in-scale 0.1 (and +-30 of the dict's 0.05): neither activation saturates, and K >= 160 spreads o1 and p over tens of levels.
EDGE_CASES = [
    ("k3x5_2x7_uneven", "default", "full", 1.5),
    ("k3x5_2x7_uneven", "dict", "full", 1.5),
    ("k5x5_2x2_p2", "default", "full", 1.5),
    ("k2x8_3x2_p1x7", "dict", "full", 1.5),
]
# (name, kind, bias, x_std) run with S = 2: on-chip draws on 16 taps of which eight are walked; guard bands around the results and signs
ON_CHIP_EDGE = ("k4x4_2x1_s2p3", "default", "full", 1.5)
GUARD_EDGE = ("k3x3_1x5", "default", "full", 1.5)
