"""The arithmetic of the INT8 quantised Bayesian layers in plain torch: the oracle of the q8 tests.

Every multiplication and addition below is ONE fp32 rounding, never fused -- except the ONE ``fma`` of the output stage, which is
fbgemm's; ``rne`` is round-to-nearest-even (torch.round); ``1 / s`` is the fp32 reciprocal of the fp32 scale. A scale arrives as a
Python float (a double, what ``q_scale()`` returns in the reference). In the weight chain the quotient of scales is taken in double
and rounded to fp32 once (torch's quantized.mul); in the output stage the scales are rounded to fp32 FIRST and every operation on them
is an fp32 one (fbgemm's conv and linear). tests/test_q8_model_host.py holds every step to torch's CPU quantised operators with exact
equality, the output stage on exact and near ties where the two readings of either choice differ.

    e   = clamp(rne(eps * (1 / s_eps)), -128, 127)
    p   = clamp(rne(float(q_sigma * e) * float(s_sigma * s_eps / s_mul)), -128, 127)
    w   = clamp(rne((float(p) * s_mul + float(q_mu) * s_mu) * (1 / s_add)), -128, 127)
    xq  = clamp(rne(x * (1 / s_in)) + z_in, 0, 255)
    acc = sum_k (xq - z_in) * w          int32, exact; padding contributes 0
    b   = mu_b + sigma_b * eps_b
    a   = f32(s_in) * f32(s_add)         (fp32), m = a / f32(s_out) (fp32)
    oq  = clamp(rne(fma(b, 1 / a, float(acc)) * m) + z_out, 0, 255)         fma: b * (1 / a) + float(acc) rounded ONCE
    out = float(oq - z_out) * s_out
"""
import torch
import torch.nn.functional as TF


def f32(v):
    """A Python float rounded to fp32, as a 0-dim fp32 tensor."""
    return torch.tensor(float(v), dtype=torch.float64).to(torch.float32)


def rcp32(s):
    return torch.tensor(1.0, dtype=torch.float32) / f32(s)


def scale_of(t, default_scale=0.1):
    """get_scale_and_zero_point + get_quantized_tensor's zero-scale rule -> Python float (the fp32 scale's value)."""
    s = torch.clamp(t.detach().abs().max(), 0, 100) * 2 / 255
    s = float(s)
    return default_scale if s == 0 else s


def quantize_sym(t, s):
    """Per-tensor symmetric int8 image of t at scale s (torch.quantize_per_tensor, qint8, zero point 0) -> int8 tensor."""
    return torch.clamp(torch.round(t.float() * rcp32(s).to(t.device)), -128, 127).to(torch.int8)


def quant_eps(eps, s_eps):
    return quantize_sym(eps, s_eps)


def qmul(q_sigma, e, s_sigma, s_eps, s_mul):
    m = f32(float(s_sigma) * float(s_eps) / float(s_mul)).to(e.device)
    prod = (q_sigma.to(torch.int32) * e.to(torch.int32)).to(torch.float32)
    return torch.clamp(torch.round(prod * m), -128, 127).to(torch.int8)


def qadd(p, q_mu, s_mul, s_mu, s_add):
    dev = p.device
    t = p.to(torch.float32) * f32(s_mul).to(dev) + q_mu.to(torch.float32) * f32(s_mu).to(dev)
    return torch.clamp(torch.round(t * rcp32(s_add).to(dev)), -128, 127).to(torch.int8)


def quant_in(x, s_in, z_in):
    return torch.clamp(torch.round(x.float() * rcp32(s_in).to(x.device)) + z_in, 0, 255).to(torch.uint8)


def sampled_weight(q_mu, q_sigma, eps, s_mu, s_sigma, s_eps, s_mul, s_add):
    """-> int8 w of eps's shape ([..., *q_mu.shape])."""
    e = quant_eps(eps, s_eps)
    return qadd(qmul(q_sigma, e, s_sigma, s_eps, s_mul), q_mu, s_mul, s_mu, s_add)


def scales_default(s_mu, s_sigma, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128):
    """The five (scale, zero point) pairs of the default branch (quant_dict is None, enable_int8_compute)."""
    s_mul = float(s_sigma) * float(normal_scale)
    s_add = max(s_mul, float(s_mu))
    return [(float(normal_scale), 0), (s_mul, 0), (s_add, 0), (float(default_scale), int(default_zero_point)), (float(default_scale), int(default_zero_point))]


def scales_from_dict(quant_dict):
    return [(float(d["scale"]), int(d["zero_point"])) for d in quant_dict]


def bias_of(mu_b, sigma_b, eps_b):
    if mu_b is None:
        return None
    if sigma_b is None:
        return mu_b.float()
    return mu_b.float() + sigma_b.float() * eps_b.float()


def out_scales(s_in, s_add, s_out):
    """-> (a, m) of the output stage as 0-dim fp32 tensors: a = f32(s_in) * f32(s_add) and m = a / f32(s_out), both fp32 operations."""
    a = f32(s_in) * f32(s_add)
    return a, a / f32(s_out)


def fma32(x, y, z):
    """fmaf(x, y, z) on fp32 tensors, in double: the product of two fp32 values is exact there, and its sum with z is rounded to 53 bits
    before the one rounding to fp32 -- which differs from a true fmaf only where that 53-bit value falls exactly on the midpoint of two
    fp32 values and the exact sum does not (some 2^-29 of all operands; torch has no fp32 fma on the CPU to take instead)."""
    return (x.double() * y.double() + z.double()).to(torch.float32)


def requant(acc, b, pairs):
    """int32 acc [N, Co, ...] and fp32 b [Co] (or None) -> the u8 output image."""
    (s_in, _), (s_out, z_out), s_add = pairs[3], pairs[4], pairs[2][0]
    dev = acc.device
    a, m = out_scales(s_in, s_add, s_out)
    t = acc.to(torch.float32)
    if b is not None:
        t = fma32(b.to(dev).view((1, -1) + (1,) * (acc.dim() - 2)), (torch.tensor(1.0) / a).to(dev), t)
    return torch.clamp(torch.round(t * m.to(dev)) + z_out, 0, 255).to(torch.uint8)


def dequant(oq, pairs):
    s_out, z_out = pairs[4]
    return (oq.to(torch.int32) - z_out).to(torch.float32) * f32(s_out).to(oq.device)


def int_conv(xq, z_in, w, conv):
    """sum_k (xq - z_in) * w, exact: float64 conv of integers (|acc| < 2^31 << 2^53) -> int32. conv None: Linear."""
    xs = (xq.to(torch.int32) - z_in).to(torch.float64)
    wd = w.to(torch.float64)
    if conv is None:
        acc = xs @ wd.t()
    else:
        acc = TF.conv2d(xs, wd, None, conv["stride"], conv["padding"], conv["dilation"], 1)
    return acc.to(torch.int32)


def forward(x, q_mu, q_sigma, s_mu, s_sigma, pairs, eps_w, mu_b=None, sigma_b=None, eps_b=None, conv=None):
    """One sample: x fp32 [B, Ci, H, W] or [B, In]; eps_w of q_mu's shape; -> (u8 image, dequantised fp32)."""
    w = sampled_weight(q_mu, q_sigma, eps_w, s_mu, s_sigma, pairs[0][0], pairs[1][0], pairs[2][0])
    xq = quant_in(x, *pairs[3])
    acc = int_conv(xq, pairs[3][1], w, conv)
    oq = requant(acc, bias_of(mu_b, sigma_b, eps_b), pairs)
    return oq, dequant(oq, pairs)
