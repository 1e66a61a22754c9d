"""The arithmetic of u8 activations between the INT8 layers in plain torch: the oracle of the q8 u8 tests.

It continues tests/_q8_model.py (M) and tests/_q8_flip_model.py (FM). tests/test_q8_u8_model_host.py holds every function here to
torch's CPU quantised operators with exact equality. Levels are uint8 tensors in NATURAL order; a pair is (scale, zero point).

    layer from a quint8 input   the layer's chain (M.forward / FM.forward) with xq GIVEN and the carrier's pair in place of `in`:
                                ``deq`` of the levels requantises to the same levels at the same pair, so the chain is fed deq(xq)
    add(a, b -> o)              FM.uadd
    add_relu(a, b -> o)         max(add, z_o)      (the fp32 sum clamped at 0 before it is requantised gives the same level)
    relu(q)                     max(q, z)
    max_pool2d                  the maximum of the levels over the window's positions inside the image
    avg_pool (global)           clamp(rne(float(sum - z * n) * float(1 / n) + z), 0, 255)      NOT rne(acc / n) + z: ties with odd z, even n
                                (the operator a CONTIGUOUS NCHW quint8 tensor gets, the reference QResNet's; torch's channels-last and
                                qnnpack kernels round first and add z afterwards)
    blocked layout              [N][ceil(C / 16)][H][W][16], bytes of channels >= C hold z
"""
import torch
import torch.nn.functional as TF

import _q8_flip_model as FM
import _q8_model as M
from _q8_model import f32


def deq(levels, pair):
    """(q - z) * s in fp32: what dequantize() gives; quantising it at the same pair returns the levels."""
    s, z = pair
    return (levels.to(torch.int32) - z).to(torch.float32) * f32(s).to(levels.device)


def with_in(pairs, pair, index=3):
    pairs = list(pairs)
    pairs[index] = (float(pair[0]), int(pair[1]))
    return pairs


def reparam_from_u8(xq, pair, q_mu, q_sigma, s_mu, s_sigma, pairs, eps_w, mu_b=None, sigma_b=None, eps_b=None, conv=None):
    """One sample of the Reparameterization layer fed a quint8 input of its own pair -> the u8 output image."""
    pr = with_in(pairs, pair, 3)
    w = M.sampled_weight(q_mu, q_sigma, eps_w, s_mu, s_sigma, pr[0][0], pr[1][0], pr[2][0])
    acc = M.int_conv(xq, pr[3][1], w, conv)
    return M.requant(acc, M.bias_of(mu_b, sigma_b, eps_b), pr)


def flip_from_u8(xq, pair, q_mu, q_sigma, s_mu, s_sigma, pairs, eps_w, sign_in, sign_out, mu_b=None, sigma_b=None, eps_b=None, conv=None):
    """One sample of the Flipout layer fed a quint8 input of its own pair -> the u8 output image."""
    pr = with_in(pairs, pair, FM.IN)
    oq, _, mid = FM.forward(deq(xq, pair), q_mu, q_sigma, s_mu, s_sigma, pr, eps_w, sign_in, sign_out, mu_b, sigma_b, eps_b, conv)
    assert torch.equal(mid["xq"], xq)
    return oq


def add(a, pa, b, pb, po):
    return FM.uadd(a, pa, b, pb, po)


def add_relu(a, pa, b, pb, po):
    return torch.clamp(add(a, pa, b, pb, po), min=int(po[1]))


def add_relu_clamped_sum(a, pa, b, pb, po):
    """The other writing of add_relu: the fp32 sum clamped at 0, then requantised."""
    (s_a, z_a), (s_b, z_b), (s_o, z_o) = pa, pb, po
    t = torch.clamp(FM._deq_fused(a, s_a, z_a) + FM._deq_fused(b, s_b, z_b), min=0.0) * M.rcp32(s_o)
    return FM._to_u8(t, z_o)


def relu(q, z):
    return torch.clamp(q, min=int(z))


def max_pool2d(q, kernel, stride, padding):
    return TF.max_pool2d(q.to(torch.float32), kernel, stride, padding).to(torch.uint8)      # (padding is -inf there: ignored)


def avg_pool(q, z):
    """Global average pool of levels [N, C, H, W] -> [N, C, 1, 1]."""
    n = q.shape[2] * q.shape[3]
    acc = (q.to(torch.int32).sum((2, 3), keepdim=True) - z * n).to(torch.float32)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    return torch.clamp(torch.round(acc * inv + float(z)), 0, 255).to(torch.uint8)


def avg_pool_rne_first(q, z):
    """NOT torch's: rne(acc / n) + z."""
    n = q.shape[2] * q.shape[3]
    acc = (q.to(torch.int32).sum((2, 3), keepdim=True) - z * n).to(torch.float32)
    return torch.clamp(torch.round(acc / n) + z, 0, 255).to(torch.uint8)


def block(levels, z):
    """Natural [N, C, H, W] or [N, F] -> the blocked image [N, CB, H, W, 16] / [N, CB * 16]."""
    if levels.dim() == 2:
        N, Fe = levels.shape
        out = torch.full((N, (Fe + 15) // 16 * 16), z, dtype=torch.uint8)
        out[:, :Fe] = levels
        return out
    N, C, H, W = levels.shape
    CB = (C + 15) // 16
    out = torch.full((N, CB, H, W, 16), z, dtype=torch.uint8)
    for c in range(C):
        out[:, c // 16, :, :, c % 16] = levels[:, c]
    return out


def unblock(img, shape):
    if len(shape) == 2:
        return img[:, :shape[1]].clone()
    N, C, H, W = shape
    return torch.stack([img[:, c // 16, :, :, c % 16] for c in range(C)], 1)


def tie_planes(h, w, z):
    """Planes [K, 3, h, w] whose sum - z * n is n * k + n / 2 (an exact tie of the mean) for every k the u8 range allows (n even).
    Three channels: a contiguous [K, 1, h, w] tensor is ALSO channels-last contiguous, and torch then takes its channels-last kernel,
    which rounds such a tie the other way (rne(acc * (1 / n)) + z) -- the operator the model follows is the one a contiguous NCHW
    quint8 tensor gets, which is what the reference's QResNet feeds it."""
    n = h * w
    assert n % 2 == 0
    ks = [k for k in range(-z, 255 - z)]
    planes = torch.empty(len(ks), 3, n, dtype=torch.int32)
    for i, k in enumerate(ks):
        planes[i, :, :n // 2] = z + k
        planes[i, :, n // 2:] = z + k + 1
        planes[i, 1] = planes[i, 1].flip(0)
    return planes.to(torch.uint8).view(len(ks), 3, h, w)
