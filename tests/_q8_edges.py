"""The edge cases of the INT8 forward that tests/test_q8_edges_host.py (CPU) and tests/test_gpu_q8_edges.py (GPU) share: exact rounding
ties at each of the five roundings, both ends of each clamp, uneven geometry (KH != KW, sh != sw, ph != pw, dh != dw) and tap pruning.
Every case is built once (functools.lru_cache) with the model's answer (tests/_q8_model.py), on the CPU.

``run`` is the model again, step by step, with one step replaced by a subtly wrong variant (``MUTANTS``): the host test holds the
unmutated ``run`` to ``M.forward`` and counts, per case, the outputs each variant changes -- a case is worth something against a wrong
kernel only if a wrong model changes its answer. The convolution of ``run`` is a loop over the taps the kernel walks, in the kernel's
index arithmetic (csrc/bt_q8.hip), so that an axis swap or a wrong tap set can be expressed at all."""
import functools
import math
import zlib

import torch

import _q8_cases as QC
import _q8_model as M

ZPAIRS = [(128, 121), (0, 3), (57, 250)]          # (z_in, z_out) of the requantisation cases: both output clamps are reached
Z_INS = (128, 0, 57)


@functools.lru_cache(maxsize=None)
def scale_sets():
    return QC.scale_sets()


# ---------------------------------------------------------------------------- the model, step by step, with one step replaced
ROUNDINGS = ("e", "p", "w", "xq", "oq")
MUTANTS = (tuple("away_" + r for r in ROUNDINGS) + ("fused_w", "unfused_oq", "bias_after_m", "m_double", "div_eps", "div_add", "div_in", "div_out") + tuple("wide_" + r for r in ROUNDINGS)
           + ("decode_kh", "swap_stride", "swap_padding", "swap_dilation", "pad_xq0", "prune_shift"))
GEOMETRY_MUTANTS = ("decode_kh", "swap_stride", "swap_padding", "swap_dilation", "pad_xq0", "prune_shift")


def _away(t):
    """Round half away from zero (roundf), exact: in double."""
    d = t.double()
    return (torch.sign(d) * torch.floor(d.abs() + 0.5)).float()


def _quant(pre, lo, hi, site, mut, offset=0):
    """clamp(round(pre) + offset, lo, hi) as int32. Mutants: round half away at this site; the clamp one wider at either end, after
    which the cast to the 8-bit type wraps."""
    r = (_away(pre) if mut == "away_" + site else torch.round(pre)) + offset
    if mut == "wide_" + site:
        r = torch.clamp(r, lo - 1, hi + 1).to(torch.int32)
        return (r - lo) % (hi - lo + 1) + lo
    return torch.clamp(r, lo, hi).to(torch.int32)


def _scaled(t, s, div):
    return t / M.f32(s) if div else t * M.rcp32(s)


def conv_out(conv, wshape, xshape):
    (sh, sw), (ph, pw), (dh, dw) = conv["stride"], conv["padding"], conv["dilation"]
    return ((xshape[2] + 2 * ph - dh * (wshape[2] - 1) - 1) // sh + 1, (xshape[3] + 2 * pw - dw * (wshape[3] - 1) - 1) // sw + 1)


def live_taps(conv, wshape, xshape):
    """The host's rule (bt_q8.hip, q8_forward): a tap is live when its row meets the image for some output row AND its column does for
    some output column -> the live taps, ascending."""
    (sh, sw), (ph, pw), (dh, dw) = conv["stride"], conv["padding"], conv["dilation"]
    KH, KW, H, W = wshape[2], wshape[3], xshape[2], xshape[3]
    Ho, Wo = conv_out(conv, wshape, xshape)
    rows = [any(0 <= oh * sh - ph + ky * dh < H for oh in range(Ho)) for ky in range(KH)]
    cols = [any(0 <= ow * sw - pw + kx * dw < W for ow in range(Wo)) for kx in range(KW)]
    return [ky * KW + kx for ky in range(KH) for kx in range(KW) if rows[ky] and cols[kx]]


def walked_taps(conv, wshape, xshape, z_in):
    """-> (the taps the kernel walks, whether they were pruned): pruning needs z_in == 128, at most 16 taps and a dead tap."""
    taps = wshape[2] * wshape[3]
    live = live_taps(conv, wshape, xshape)
    if z_in == 128 and taps <= 16 and 0 < len(live) < taps:
        return live, True
    return list(range(taps)), False


def _acc(xq, z_in, w, conv, mut):
    """sum_k (xq - z_in) * w as int32 (exact in float64). Conv: tap by tap over the walked taps, each tap's input row and column from
    the kernel's ih = oh * sh - ph + ky * dh; a position outside the image contributes 0 (the mutant pad_xq0: xq = 0, so -z_in)."""
    xs = (xq - z_in).to(torch.float64)
    wd = w.to(torch.float64)
    if conv is None:
        return (xs @ wd.t()).to(torch.int32)
    Co, Ci, KH, KW = w.shape
    B, _, H, W = xs.shape
    Ho, Wo = conv_out(conv, w.shape, xs.shape)
    (sh, sw), (ph, pw), (dh, dw) = conv["stride"], conv["padding"], conv["dilation"]
    if mut == "swap_stride":
        sh, sw = sw, sh
    if mut == "swap_padding":
        ph, pw = pw, ph
    if mut == "swap_dilation":
        dh, dw = dw, dh
    walked, pruned = walked_taps(conv, w.shape, xs.shape, z_in)
    if mut == "prune_shift" and pruned:
        walked = [(t + 1) % (KH * KW) for t in walked]
    pad = float(-z_in) if mut == "pad_xq0" else 0.0
    acc = torch.zeros((B, Co, Ho, Wo), dtype=torch.float64)
    for t in walked:
        wy, wx = divmod(t, KW)                                   # the weight of tap t is where the pack put it, whatever the mutant
        ky, kx = divmod(t, KH) if mut == "decode_kh" else (wy, wx)
        ih, iw = torch.arange(Ho) * sh - ph + ky * dh, torch.arange(Wo) * sw - pw + kx * dw
        inside = ((ih >= 0) & (ih < H)).view(-1, 1) & ((iw >= 0) & (iw < W)).view(1, -1)
        patch = xs[:, :, ih.clamp(0, H - 1)][:, :, :, iw.clamp(0, W - 1)]
        patch = torch.where(inside, patch, torch.full((), pad, dtype=torch.float64))
        acc += torch.einsum("bchw,oc->bohw", patch, wd[:, :, wy, wx])
    return acc.to(torch.int32)


def run(c, s, mut=None):
    """Sample s of case c by the model's steps (module docstring of _q8_model), ``mut`` replacing one -> dict of the int32 images e, p,
    w, xq, acc, oq, the fp32 out, and ``pre``: the fp32 value each rounding was fed."""
    pairs = c["pairs"]
    s_eps, s_mul, s_add = pairs[0][0], pairs[1][0], pairs[2][0]
    (s_in, z_in), (s_out, z_out) = pairs[3], pairs[4]
    qm, qs = c["q_mu"].to(torch.int32), c["q_sigma"].to(torch.int32)
    pre = {}
    pre["e"] = _scaled(c["eps_w"][s].float(), s_eps, mut == "div_eps")
    e = _quant(pre["e"], -128, 127, "e", mut)
    pre["p"] = (qs * e).to(torch.float32) * M.f32(float(c["s_sigma"]) * float(s_eps) / float(s_mul))
    p = _quant(pre["p"], -128, 127, "p", mut)
    if mut == "fused_w":
        t = (p.double() * M.f32(s_mul).double() + qm.double() * M.f32(c["s_mu"]).double()).float()
    else:
        t = p.float() * M.f32(s_mul) + qm.float() * M.f32(c["s_mu"])
    pre["w"] = _scaled(t, s_add, mut == "div_add")
    w = _quant(pre["w"], -128, 127, "w", mut)
    x = c["x"] if c.get("shared_x", True) else c["x"].chunk(c["S"], 0)[s]
    pre["xq"] = _scaled(x.float(), s_in, mut == "div_in")
    xq = _quant(pre["xq"], 0, 255, "xq", mut, offset=z_in)
    acc = _acc(xq, z_in, w, c["conv"], mut)
    a, m = M.out_scales(s_in, s_add, s_out)
    if mut == "m_double":                     # the multiplier from the double scales, rounded once
        m = M.f32(float(s_in) * float(s_add) / float(s_out))
    b = M.bias_of(c["mu_b"], c["sigma_b"], None if c["eps_b"] is None else c["eps_b"][s])
    t = acc.float()
    if b is not None:
        bv = b.view((1, -1) + (1,) * (acc.dim() - 2))
        if mut == "div_out":                  # bias / a, which no fma takes in
            t = t + bv / a
        elif mut == "unfused_oq":             # two roundings
            t = t + bv * (torch.tensor(1.0) / a)
        elif mut == "bias_after_m":           # the bias at the output scale, behind the multiplier
            t = t * m + bv * M.rcp32(s_out)
        else:
            t = M.fma32(bv, torch.tensor(1.0) / a, t)
    pre["oq"] = t if mut == "bias_after_m" and b is not None else t * m
    t = pre["oq"]
    oq = _quant(t, 0, 255, "oq", mut, offset=z_out)
    return dict(e=e, p=p, w=w, xq=xq, acc=acc, oq=oq, out=(oq - z_out).float() * M.f32(s_out), pre=pre)


def run_oq(c, mut=None):
    """The u8 image of all of c's samples, as int32, stacked like the kernel's output."""
    return torch.cat([run(c, s, mut)["oq"] for s in range(c["S"])], 0)


def stats(c):
    """Per rounding, over all samples: exact ties fed to it (fraction exactly 0.5 in fp32), hits of either clamp end, distinct values."""
    out = {}
    for r in ROUNDINGS:
        lo, hi = (-128, 127) if r in ("e", "p", "w") else (0, 255)
        ties = n_lo = n_hi = 0
        seen = set()
        for s in range(c["S"]):
            st = run(c, s)
            pre = st["pre"][r]
            ties += int((pre - torch.floor(pre) == 0.5).sum())
            n_lo, n_hi = n_lo + int((st[r] == lo).sum()), n_hi + int((st[r] == hi).sum())
            seen |= set(torch.unique(st[r]).tolist())
        out[r] = dict(ties=ties, lo=n_lo, hi=n_hi, levels=len(seen))
    return out


def _finish(c):
    """Add the model's answer (M.forward per sample) to a case."""
    c.setdefault("S", 1), c.setdefault("shared_x", True)
    for k in ("mu_b", "sigma_b", "eps_b"):
        c.setdefault(k, None)
    xs = [c["x"]] * c["S"] if c["shared_x"] else list(c["x"].chunk(c["S"], 0))
    ref = [M.forward(xs[s], c["q_mu"], c["q_sigma"], c["s_mu"], c["s_sigma"], c["pairs"], c["eps_w"][s], c["mu_b"], c["sigma_b"],
                     None if c["eps_b"] is None else c["eps_b"][s], c["conv"]) for s in range(c["S"])]
    c["oq"], c["out"] = torch.cat([r[0] for r in ref], 0), torch.cat([r[1] for r in ref], 0)
    c["wshape"] = tuple(c["q_mu"].shape)
    return c


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------- C. the weight chain, read out through an identity input
CHAIN_N = 256
CHAIN_PATTERNS = (0, 1, 2)


def is_tie_set(name):
    return name in QC.TIE_SETS


@functools.lru_cache(maxsize=None)
def chain_case(set_name, pat):
    """Linear 256 <- 256 on x = eye(256) with input pair (1, 128) and output pair (s_add, 128): the output multiplier is exactly 1 and
    oq - 128 = w[co, k] transposed. q_mu[co, k] = co - 128 (every value); q_sigma: two patterns in 0..127, one over -128..127; eps a
    ramp over k that passes both clamp ends of e -- at the tie sets on exact half steps of s_eps. S = 2, the second sample's ramp
    shifted by a row-dependent offset."""
    s_mu, s_sigma, s_eps, s_mul, s_add = scale_sets()[set_name]
    n = CHAIN_N
    co, k = torch.arange(n).view(-1, 1), torch.arange(n).view(1, -1)
    q_mu = (co - 128).expand(n, n).to(torch.int8)
    if pat < 2:
        q_sigma = ((5 * co + 3 * k + 41 * pat) % 128).to(torch.int8)
    else:
        q_sigma = ((5 * co + 3 * k + 82) % 256 - 128).to(torch.int8)
    ks = torch.stack([k.expand(n, n), (k + 7 * co + 13) % n]).to(torch.float64) - 128
    if is_tie_set(set_name):      # on the half steps: every e a tie -- and so every e even; pattern 1's second sample is a quarter step off: odd e too
        eps = ((ks + torch.tensor([0.5, 0.25 if pat == 1 else 0.5], dtype=torch.float64).view(2, 1, 1)) * float(s_eps)).to(torch.float32)
    else:
        eps = (ks * 1.03 * float(s_eps)).to(torch.float32)
    pairs = [(s_eps, 0), (s_mul, 0), (s_add, 0), (1.0, 128), (s_add, 128)]
    return _finish(dict(q_mu=q_mu.contiguous(), q_sigma=q_sigma.contiguous(), x=torch.eye(n), pairs=pairs, eps_w=eps, conv=None, s_mu=s_mu, s_sigma=s_sigma, S=2))


# ---------------------------------------------------------------------------- D. the input quantiser, read out through an identity weight
INQ_KINDS = {"dyadic": QC.DYADIC_S_IN, "decimal": QC.GPU_S_IN}


@functools.lru_cache(maxsize=None)
def inq_case(kind, z):
    """Linear 96 <- 96 with q_mu = eye, q_sigma = 0 and s_mu = s_add = 2^-6 (w = q_mu), output pair (s_in * 2^-6, z): oq = xq. x is
    [140, 96] of half steps (n + 0.5) * s_in, n over -320..320 (past both clamp ends at every z); every third row is moved off the ties."""
    s_in, s = INQ_KINDS[kind], 2.0 ** -6
    B, n = 140, 96
    idx = torch.arange(B * n)
    steps = ((idx * 37) % 641 - 320).to(torch.float64)
    x = ((steps + 0.5) * s_in).to(torch.float32).view(B, n).clone()
    x[2::3] *= 1.003
    q_mu = torch.eye(n).to(torch.int8)
    pairs = [QC.GPU_PAIRS3[0], QC.GPU_PAIRS3[1], (s, 0), (s_in, z), (s_in * s, z)]
    eps = torch.randn((1, n, n), generator=_gen("inq", kind, z))
    return _finish(dict(q_mu=q_mu, q_sigma=torch.zeros_like(q_mu), x=x, pairs=pairs, eps_w=eps, conv=None, s_mu=s, s_sigma=QC.GPU_S_SIGMA))


# ---------------------------------------------------------------------------- E. requantisation ties and clamps
REQ_SHAPES = {"linear": ((70, 112), (140, 112), None),        # two row tiles, seven units, two pixel tiles
              "conv": ((9, 20, 3, 2), (3, 20, 6, 7), dict(stride=(2, 1), padding=(1, 0), dilation=(1, 2), groups=1)),
              "conv_undilated": ((9, 20, 3, 2), (3, 20, 6, 7), dict(stride=(2, 1), padding=(1, 0), dilation=(1, 1), groups=1))}      # (for oneDNN, host only)
REQ_S_IN, REQ_S_ADD, REQ_S_OUT = 2.0 ** -4, 2.0 ** -7, 2.0 ** -10      # the output multiplier is exactly 0.5
REQ_S_ADD_DEC = 0.006                                                  # 'half_decimal': s_out = 0.006 / 8, the multiplier still exactly 0.5


REQ_TIE_BIASES = ("none", "half", "half_decimal")


@functools.lru_cache(maxsize=None)
def requant_case(shape, zi, bias):
    """bias 'none' / 'half': sigma = 0 and s_mu = s_add, so w = q_mu in -9..9; x integer steps of s_in in -6..6; the multiplier 0.5
    makes every odd accumulator an exact tie, and a bias of half-integer multiples of s_out ('half') every even one.
    bias 'half_decimal': the same with the decimal s_add = s_mu = 0.006 and s_out = s_add / 8: b * (1 / a) is an odd integer or a fraction of an
    ulp beside it, channel by channel, which only the ONE rounding of fma(b, 1 / a, float(acc)) keeps; b / a is not the same value.
    bias 'full': random int8 images and fp32 data at the GPU cases' decimal scales with mu_b + sigma_b * eps_b: off the ties."""
    wshape, xshape, conv = REQ_SHAPES[shape]
    z_in, z_out = ZPAIRS[zi]
    g = _gen("requant", shape, zi, bias)
    Co = wshape[0]
    if bias == "full":
        K, z_out = math.prod(wshape[1:]), 121
        s_out = 0.02 * math.sqrt(K)
        c = dict(q_mu=torch.randint(-128, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8),
                 q_sigma=torch.randint(0, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8), x=torch.randn(xshape, generator=g) * 1.5,
                 pairs=QC.GPU_PAIRS3 + [(QC.GPU_S_IN, z_in), (s_out, z_out)], s_mu=QC.GPU_S_MU, s_sigma=QC.GPU_S_SIGMA,
                 mu_b=torch.randn(Co, generator=g) * (3.0 * s_out), sigma_b=torch.rand(Co, generator=g) * (2.0 * s_out), eps_b=torch.randn((1, Co), generator=g))
    else:
        s_add, s_out = (REQ_S_ADD, REQ_S_OUT) if bias != "half_decimal" else (REQ_S_ADD_DEC, REQ_S_ADD_DEC * 2.0 ** -3)
        q_mu = torch.randint(-9, 10, wshape, generator=g, dtype=torch.int32).to(torch.int8)
        c = dict(q_mu=q_mu, q_sigma=torch.zeros_like(q_mu), x=torch.randint(-6, 7, xshape, generator=g).float() * REQ_S_IN,
                 pairs=[QC.GPU_PAIRS3[0], QC.GPU_PAIRS3[1], (s_add, 0), (REQ_S_IN, z_in), (s_out, z_out)], s_mu=s_add, s_sigma=QC.GPU_S_SIGMA)
        if bias == "half":
            c["mu_b"] = (torch.randint(-8, 8, (Co,), generator=g).float() + 0.5) * REQ_S_OUT
        if bias == "half_decimal":
            c["mu_b"] = ((torch.randint(-64, 64, (Co,), generator=g).double() + 0.5) * s_out).float()
    c["eps_w"] = torch.randn((1,) + wshape, generator=g)
    c["conv"] = conv
    return _finish(c)


# ---------------------------------------------------------------------------- E'. near ties of the output stage at non-dyadic multipliers
# (s_in, s_add, the multiplier aimed at, weight step): m = f32(s_in) * f32(s_add) / f32(s_out) in fp32 operations is not exactly the
# multiplier aimed at, and (for these scales) not the double quotient rounded once either; weight step * multiplier is an integer
NEAR = [(0.0437, 0.0031, 0.75, 4), (0.05, 0.0029, 1.5, 2), (0.0713, 0.0053, 0.3, 10)]


@functools.lru_cache(maxsize=None)
def near_case(i, as_conv=False):
    """Linear 256 <- 1 on 64 rows holding the input levels 0..63 (z_in = 0), or the same as a 1x1 conv on 1x1 maps; w = q_mu (sigma = 0,
    s_mu = s_add) in +-1..3 weight steps, so that acc * m is an integer but for the error of m, and a bias that puts (acc + b / a) * m
    on a half step but for its own rounding to fp32: every output that is not clamped sits ON or an ulp or two BESIDE a tie, where
    the one rounding of the fma, the reciprocal of a, and the last bit of m each decide it."""
    s_in, s_add, mt, step = NEAR[i]
    s_out = s_in * s_add / mt
    a, m = M.out_scales(s_in, s_add, s_out)
    g = _gen("near", i)
    co = torch.arange(256)
    q_mu = (torch.tensor([-3, -2, -1, 1, 2, 3])[co % 6] * step).to(torch.int8).view(256, 1)
    half = torch.randint(-20, 20, (256,), generator=g).double() + 0.5
    x = (torch.arange(64).double() * s_in).float().view(64, 1)
    c = dict(q_mu=q_mu, q_sigma=torch.zeros_like(q_mu), x=x, pairs=[QC.GPU_PAIRS3[0], QC.GPU_PAIRS3[1], (s_add, 0), (s_in, 0), (s_out, 128)], s_mu=s_add,
             s_sigma=QC.GPU_S_SIGMA, mu_b=(half / float(m) * float(a)).float(), eps_w=torch.randn((1, 256, 1), generator=g), conv=None)
    if as_conv:
        c.update(q_mu=q_mu.view(256, 1, 1, 1), q_sigma=torch.zeros(256, 1, 1, 1, dtype=torch.int8), x=x.view(64, 1, 1, 1), eps_w=c["eps_w"].view(1, 256, 1, 1, 1),
                 conv=dict(stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1))
    return _finish(c)


# ---------------------------------------------------------------------------- F. uneven geometry and tap pruning
# name -> ((KH, KW, H, W, sh, sw, ph, pw, dh, dw), Ci, Co, B, the live taps by the host's rule)
GEOMS = {
    "k3x3_1x5": ((3, 3, 1, 5, 1, 1, 1, 1, 1, 1), 20, 9, 30, [3, 4, 5]),                       # three live taps, CB = 2: VU = 6, no multiple of the stage
    "k4x4_2x1_s2p3": ((4, 4, 2, 1, 2, 2, 3, 3, 1, 1), 20, 9, 3, list(range(1, 16, 2))),      # 16 taps, the limit of the live-tap word
    "k5x5_2x2_p2": ((5, 5, 2, 2, 1, 1, 2, 2, 1, 1), 20, 9, 3, [6, 7, 8, 11, 12, 13, 16, 17, 18]),      # 25 taps: pruning is off, padding must be a true zero
    "k3x5_2x7_uneven": ((3, 5, 2, 7, 2, 1, 1, 4, 1, 2), 20, 70, 20, list(range(5, 15))),     # ten live taps, two channel tiles, two pixel tiles
    "k2x8_3x2_p1x7": ((2, 8, 3, 2, 1, 1, 1, 7, 1, 1), 16, 9, 5, list(range(16))),            # all 16 live; Ho = 4, Wo = 9: a pixel tile crosses images
    "k3x2_9x7_uneven": ((3, 2, 9, 7, 2, 1, 1, 0, 1, 2), 20, 9, 7, list(range(6))),           # unpruned, every pair uneven
}


def geom_conv(name):
    KH, KW, H, W, sh, sw, ph, pw, dh, dw = GEOMS[name][0]
    return dict(stride=(sh, sw), padding=(ph, pw), dilation=(dh, dw), groups=1)


@functools.lru_cache(maxsize=None)
def geom_case(name, z_in, S=1, stacked=False):
    """Random int8 images, fp32 data and a full bias at the GPU cases' scales on geometry ``name``; stacked: one x per sample."""
    (KH, KW, H, W, *_), Ci, Co, B, _ = GEOMS[name]
    g = _gen("geom", name, z_in, S, stacked)
    wshape = (Co, Ci, KH, KW)
    s_out = 0.02 * math.sqrt(len(GEOMS[name][4]) * Ci)
    return _finish(dict(q_mu=torch.randint(-128, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8),
                        q_sigma=torch.randint(0, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8),
                        x=torch.randn(((S if stacked else 1) * B, Ci, H, W), generator=g) * 1.5, pairs=QC.GPU_PAIRS3 + [(QC.GPU_S_IN, z_in), (s_out, 121)],
                        s_mu=QC.GPU_S_MU, s_sigma=QC.GPU_S_SIGMA, mu_b=torch.randn(Co, generator=g) * (3.0 * s_out), sigma_b=torch.rand(Co, generator=g) * (2.0 * s_out),
                        eps_w=torch.randn((S,) + wshape, generator=g), eps_b=torch.randn((S, Co), generator=g), conv=geom_conv(name), S=S, shared_x=not stacked))


# ---------------------------------------------------------------------------- every case the GPU file runs, by family
def all_cases():
    """-> {id: (builder, arguments)} of every case of C to F."""
    out = {}
    for name in sorted(scale_sets()):
        for pat in CHAIN_PATTERNS:
            out[f"chain[{name}]-pat{pat}"] = (chain_case, (name, pat))
    for kind in INQ_KINDS:
        for z in Z_INS:
            out[f"inq-{kind}-z{z}"] = (inq_case, (kind, z))
    for shape in ("linear", "conv"):
        for zi in range(len(ZPAIRS)):
            for bias in REQ_TIE_BIASES:
                out[f"requant-{shape}-z{ZPAIRS[zi][0]}-{bias}"] = (requant_case, (shape, zi, bias))
        out[f"requant-{shape}-z57-full"] = (requant_case, (shape, 2, "full"))
    for i in range(len(NEAR)):
        out[f"near-{i}-linear"] = (near_case, (i, False))
        out[f"near-{i}-conv1x1"] = (near_case, (i, True))
    for name in GEOMS:
        for z in Z_INS:
            out[f"geom-{name}-z{z}"] = (geom_case, (name, z))
    out["geom-k3x2_9x7_uneven-z57-S2-stacked"] = (geom_case, ("k3x2_9x7_uneven", 57, 2, True))
    return out
