"""The arithmetic of the INT8 quantised Flipout layers in plain torch: the oracle of the q8 Flipout tests.

It continues tests/_q8_model.py (whose ``quant_eps``, ``qmul``, ``quant_in``, ``int_conv``, ``requant``, ``dequant`` and ``fma32`` it
reuses) with the two operators on quint8 tensors the Flipout chain adds; tests/test_q8_flip_model_host.py holds both to torch's CPU
operators on every pair of u8 values, and the whole chain to the literal operator chain. Ten (scale, zero point) pairs, ``PAIRS``'
order; every operation ONE fp32 rounding:

    e    = clamp(rne(eps * (1 / s_eps)), -128, 127)
    d    = qmul(q_sigma, e; s_sigma, s_eps -> s_delta)                          (qint8 x qint8: the quotient of scales in double)
    xq   = clamp(rne(x * (1 / s_in)) + z_in, 0, 255)
    acc1 = sum_k (xq - z_in) * q_mu;   o1 = requant(acc1, mu_b; a = f32(s_in) * f32(s_mu)) -> (s_mean, z_mean)
    qsi  = clamp(rne(sign_in * (1 / s_si)) + z_si, 0, 255),  qso likewise
    x'   = umul(xq, qsi -> xp)
    acc2 = sum_k (x' - z_xp) * d;      p  = requant(acc2, sigma_b * eps_b; a = f32(s_xp) * f32(s_delta)) -> (s_pert, z_pert)
    p'   = umul(p, qso -> pert_signed)
    oq   = uadd(o1, p' -> out);        out = float(oq - z_out) * s_out
    umul(a, b -> o) = clamp(rne(float((a - z_a) * (b - z_b)) * M) + z_o, 0, 255),  M = f32(s_a) * f32(s_b) * (1 / f32(s_o)), left to right
    uadd(a, b -> o) = clamp(rne((fma(float(a), s_a, -(float(z_a) * s_a)) + fma(float(b), s_b, -(float(z_b) * s_b))) * (1 / s_o)) + z_o, 0, 255)

``umul_double_quotient`` and ``uadd_unfused`` are the two readings torch does NOT take (the multiplier of the qint8 ``qmul``; the
dequantisation as (a - z) * s): kept so that the tests can show that they give other bytes.
"""
import torch

import _q8_model as M
from _q8_model import f32, rcp32

PAIRS = ("eps", "delta", "in", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")
EPS, DELTA, IN, MEAN, SIGN_IN, SIGN_OUT, XP, PERT, PERT_SIGNED, OUT = range(10)


def scales_default(s_sigma, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128):
    """The ten pairs of the default branch (quant_dict is None)."""
    dflt = (float(default_scale), int(default_zero_point))
    return [(float(normal_scale), 0), (float(s_sigma) * float(normal_scale), 0)] + [dflt] * 8


def scales_from_dict(quant_dict):
    return [(float(d["scale"]), int(d["zero_point"])) for d in quant_dict]


def quant_sign(sign, s, z):
    """quantize_per_tensor of a +-1 tensor to quint8 -> uint8."""
    return M.quant_in(sign, s, z)


def _to_u8(t, z_o):
    return torch.clamp(torch.round(t) + z_o, 0, 255).to(torch.uint8)


def umul(a, pa, b, pb, po):
    """quantized.mul of two quint8 images a, b (uint8 tensors) with pairs pa, pb -> the image at pair po."""
    (s_a, z_a), (s_b, z_b), (s_o, z_o) = pa, pb, po
    m = f32(s_a) * f32(s_b) * rcp32(s_o)
    prod = ((a.to(torch.int32) - z_a) * (b.to(torch.int32) - z_b)).to(torch.float32)
    return _to_u8(prod * m.to(a.device), z_o)


def umul_double_quotient(a, pa, b, pb, po):
    """NOT torch's: the multiplier as the qint8 qmul takes it, float(s_a * s_b / s_o) from doubles."""
    (s_a, z_a), (s_b, z_b), (s_o, z_o) = pa, pb, po
    m = f32(float(s_a) * float(s_b) / float(s_o))
    prod = ((a.to(torch.int32) - z_a) * (b.to(torch.int32) - z_b)).to(torch.float32)
    return _to_u8(prod * m.to(a.device), z_o)


def _deq_fused(a, s, z):
    sf = f32(s)
    return M.fma32(a.to(torch.float32), sf.expand(a.shape), (-(torch.tensor(float(z), dtype=torch.float32) * sf)).expand(a.shape))


def uadd(a, pa, b, pb, po):
    """quantized.add of two quint8 images."""
    (s_a, z_a), (s_b, z_b), (s_o, z_o) = pa, pb, po
    t = (_deq_fused(a, s_a, z_a) + _deq_fused(b, s_b, z_b)) * rcp32(s_o)
    return _to_u8(t, z_o)


def uadd_unfused(a, pa, b, pb, po):
    """NOT torch's: either operand dequantised as float(a - z) * s."""
    (s_a, z_a), (s_b, z_b), (s_o, z_o) = pa, pb, po
    da = (a.to(torch.int32) - z_a).to(torch.float32) * f32(s_a)
    db = (b.to(torch.int32) - z_b).to(torch.float32) * f32(s_b)
    return _to_u8((da + db) * rcp32(s_o), z_o)


def _requant(acc, b, s_act, s_w, po):
    """tests/_q8_model.py's output stage with a = f32(s_act) * f32(s_w) and the result's pair po."""
    return M.requant(acc, b, [None, None, (s_w, 0), (s_act, 0), po])


def forward(x, q_mu, q_sigma, s_mu, s_sigma, pairs, eps_w, sign_in, sign_out, mu_b=None, sigma_b=None, eps_b=None, conv=None, mul=umul, add=uadd):
    """One sample: x fp32 [B, Ci, H, W] or [B, In]; eps_w of q_mu's shape; sign_in of x's shape, sign_out of the output's (+-1; a
    negative value means -1, anything else +1) -> (u8 image, dequantised fp32, dict(o1, xp, p, ps) of the intermediate u8 images).
    ``mul`` / ``add``: the operator forms (the rejected ones for the tests that tell them apart)."""
    sgn = lambda t: torch.where(t < 0, -1.0, 1.0)
    e = M.quant_eps(eps_w, pairs[EPS][0])
    d = M.qmul(q_sigma, e, s_sigma, pairs[EPS][0], pairs[DELTA][0])
    xq = M.quant_in(x, *pairs[IN])
    o1 = _requant(M.int_conv(xq, pairs[IN][1], q_mu, conv), None if mu_b is None else mu_b.float(), pairs[IN][0], s_mu, pairs[MEAN])
    qsi = quant_sign(sgn(sign_in), *pairs[SIGN_IN])
    qso = quant_sign(sgn(sign_out), *pairs[SIGN_OUT])
    xp = mul(xq, pairs[IN], qsi, pairs[SIGN_IN], pairs[XP])
    bp = None if (mu_b is None or sigma_b is None) else sigma_b.float() * eps_b.float()
    p = _requant(M.int_conv(xp, pairs[XP][1], d, conv), bp, pairs[XP][0], pairs[DELTA][0], pairs[PERT])
    ps = mul(p, pairs[PERT], qso, pairs[SIGN_OUT], pairs[PERT_SIGNED])
    oq = add(o1, pairs[MEAN], ps, pairs[PERT_SIGNED], pairs[OUT])
    out = (oq.to(torch.int32) - pairs[OUT][1]).to(torch.float32) * f32(pairs[OUT][0])
    return oq, out, dict(o1=o1, xp=xp, p=p, ps=ps, d=d, xq=xq)


def float_flipout(x, mu, sigma, eps_w, sign_in, sign_out, mu_b=None, sigma_b=None, eps_b=None, conv=None):
    """The float Flipout formula on the same draws, in double: conv(x, mu) + mu_b + (conv(x * s_in, sigma * eps) + sigma_b * eps_b) * s_out
    -> (out, dict of the intermediates whose ranges a quant_dict is built from)."""
    import torch.nn.functional as TF
    dd = lambda t: None if t is None else t.double()
    op = (lambda a, w, b: TF.linear(a, w, b)) if conv is None else (lambda a, w, b: TF.conv2d(a, w, b, conv["stride"], conv["padding"], conv["dilation"], 1))
    mean = op(x.double(), mu.double(), dd(mu_b))
    delta = sigma.double() * eps_w.double()
    xp = x.double() * sign_in.double()
    bp = None if (mu_b is None or sigma_b is None) else sigma_b.double() * eps_b.double()
    pert = op(xp, delta, bp)
    ps = pert * sign_out.double()
    out = mean + ps
    return out, dict(eps=eps_w, delta=delta, inp=x, mean=mean, sign_in=sign_in, sign_out=sign_out, xp=xp, pert=pert, pert_signed=ps, out=out)
