"""CPU: the model of u8 activations between the INT8 layers (tests/_q8_u8_model.py) against torch's own CPU quantised operators --
a conv fed a quint8 tensor, quantized.add / add_relu over all u8 pairs, relu, max_pool2d and the global average pool (exact ties
included) -- with exact equality everywhere. No kernels are launched."""
import pytest
import torch
import torch.nn.functional as TF

import _q8_model as M
import _q8_u8_model as U

ADD_SETS = {"equal scales": ((0.1, 128), (0.1, 128), (0.1, 0)),
            "qresnet default": ((0.05, 100), (0.073, 57), (0.073, 0)),
            "odd output zero point": ((0.031, 0), (0.02, 255), (0.045, 121)),
            "dyadic ties": ((2.0 ** -4, 128), (2.0 ** -5, 64), (2.0 ** -4, 3)),
            "narrow output": ((0.21, 7), (0.4, 250), (0.05, 31))}


def _qt(levels, pair):
    return torch._make_per_tensor_quantized_tensor(levels, float(pair[0]), int(pair[1]))


def _all_u8_pairs():
    a = torch.arange(256, dtype=torch.int32)
    return a.repeat_interleave(256).to(torch.uint8).view(256, 256), a.repeat(256).to(torch.uint8).view(256, 256)


@pytest.mark.parametrize("name", sorted(ADD_SETS))
def test_add_and_add_relu_over_all_u8_pairs(name):
    pa, pb, po = ADD_SETS[name]
    a, b = _all_u8_pairs()
    ref = torch.ops.quantized.add(_qt(a, pa), _qt(b, pb), po[0], po[1]).int_repr()
    assert torch.equal(U.add(a, pa, b, pb, po), ref)
    ref_r = torch.ops.quantized.add_relu(_qt(a, pa), _qt(b, pb), po[0], po[1]).int_repr()
    got_r = U.add_relu(a, pa, b, pb, po)
    assert torch.equal(got_r, ref_r), int((got_r != ref_r).sum())
    assert torch.equal(U.add_relu_clamped_sum(a, pa, b, pb, po), ref_r)      # the two writings agree on every pair
    assert len(torch.unique(ref)) > 8 and (po[1] == 0 or not torch.equal(ref, ref_r))


@pytest.mark.parametrize("z", [0, 100, 255])
def test_relu_over_all_levels(z):
    q = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(1, 1, 16, 16)
    ref = torch.relu(_qt(q, (0.07, z))).int_repr()
    assert torch.equal(U.relu(q, z), ref)
    ref = TF.relu(_qt(q.clone(), (0.07, z)), inplace=True).int_repr()
    assert torch.equal(U.relu(q, z), ref)


@pytest.mark.parametrize("shape,kernel,stride,padding", [((2, 5, 9, 7), 3, 2, 1), ((2, 3, 4, 4), 2, 2, 0)])
def test_max_pool2d(shape, kernel, stride, padding):
    g = torch.Generator().manual_seed(11)
    q = torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)
    q[0, 0] = 0          # a plane of the lowest level: padding must not win
    for z in (0, 131):
        ref = TF.max_pool2d(_qt(q, (0.05, z)), kernel, stride, padding).int_repr()
        assert torch.equal(U.max_pool2d(q, kernel, stride, padding), ref)


@pytest.mark.parametrize("z", [0, 1, 57, 128, 255])
@pytest.mark.parametrize("hw", [(2, 2), (4, 4), (3, 5), (7, 7)])
def test_global_average_pool(hw, z):
    h, w = hw
    g = torch.Generator().manual_seed(100 * h + w)
    q = torch.randint(0, 256, (64, 7, h, w), generator=g, dtype=torch.int32).to(torch.uint8)
    near = torch.clamp(torch.randint(-3, 4, (64, 7, h, w), generator=g, dtype=torch.int32) + z, 0, 255).to(torch.uint8)      # small |sum - z n|: both signs
    cases = [q, near]
    if (h * w) % 2 == 0:
        cases.append(U.tie_planes(h, w, z))
    for t in cases:
        ref = TF.adaptive_avg_pool2d(_qt(t, (0.043, z)), 1).int_repr()
        got = U.avg_pool(t, z)
        assert torch.equal(got, ref), (hw, z, int((got != ref).sum()))
        assert torch.equal(TF.avg_pool2d(_qt(t, (0.043, z)), (h, w)).int_repr(), ref)      # the global nn.AvgPool2d is the same operator


def test_average_pool_ties_tell_the_two_forms_apart():
    """rne(acc / n) + z is NOT torch's: on exact ties with an odd zero point and an even n it rounds the other way."""
    t = U.tie_planes(2, 2, 57)
    ref = TF.adaptive_avg_pool2d(_qt(t, (0.043, 57)), 1).int_repr()
    assert torch.equal(U.avg_pool(t, 57), ref) and not torch.equal(U.avg_pool_rne_first(t, 57), ref)


def test_dequantise_then_requantise_returns_the_levels():
    q = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    for pair in [(0.1, 128), (0.0437, 0), (0.0713, 57), (1e-3, 255), (37.5, 3)]:
        x = U.deq(q, pair)
        assert torch.equal(x, _qt(q, pair).dequantize())
        assert torch.equal(M.quant_in(x, *pair), q)


CONVS = [((12, 5, 3, 3), (3, 5, 9, 9), dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1))),
         ((9, 19, 3, 3), (2, 19, 11, 10), dict(stride=(2, 2), padding=(1, 1), dilation=(1, 1))),
         ((10, 70), (37, 70), None)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("inp", [(0.1, 128), (0.0437, 0), (0.0713, 57)])
def test_conv_from_a_quint8_input(inp, bias):
    """The layer's model fed levels at the carrier's pair == torch's quantised conv2d / linear fed that quint8 tensor; the sampled
    weight comes from the existing weight-chain model. The layer's own `in` pair (here (0.5, 9)) is not read."""
    s_mu, s_sigma = 0.0023, 0.0007
    for i, (wshape, xshape, conv) in enumerate(CONVS):
        g = torch.Generator().manual_seed(40 + i)
        q_mu = torch.randint(-128, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
        q_sigma = torch.randint(0, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
        eps = torch.randn(wshape, generator=g)
        xq = torch.randint(0, 256, xshape, generator=g, dtype=torch.int32).to(torch.uint8)
        K = q_mu[0].numel()
        pairs = [(6 / 255, 0), (0.0004, 0), (0.0029, 0), (0.5, 9), (0.012 * K ** 0.5, 31)]
        mu_b = torch.randn(wshape[0], generator=g) * 2.0 if bias else None
        w = M.sampled_weight(q_mu, q_sigma, eps, s_mu, s_sigma, pairs[0][0], pairs[1][0], pairs[2][0])
        wq = torch._make_per_tensor_quantized_tensor(w, pairs[2][0], 0)
        if conv is None:
            ref = torch.nn.quantized.functional.linear(_qt(xq, inp), wq, mu_b, scale=pairs[4][0], zero_point=pairs[4][1]).int_repr()
        else:
            ref = torch.nn.quantized.functional.conv2d(_qt(xq, inp), wq, mu_b, conv["stride"], conv["padding"], conv["dilation"], 1, scale=pairs[4][0],
                                                       zero_point=pairs[4][1]).int_repr()
        got = U.reparam_from_u8(xq, inp, q_mu, q_sigma, s_mu, s_sigma, pairs, eps, mu_b, None, None, conv)
        assert 0 < int((ref > 0).sum()) and int((ref < 255).sum()) > ref.numel() // 4      # the case is not saturated away
        assert torch.equal(got, ref), (wshape, int((got != ref).sum()), ref.numel())
        # ... and equals the existing fp32-input model fed the dequantised levels at the same pair
        assert torch.equal(M.forward(U.deq(xq, inp), q_mu, q_sigma, s_mu, s_sigma, U.with_in(pairs, inp), eps, mu_b, None, None, conv)[0], ref)


@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (1, 16, 2, 2), (3, 20, 3, 1), (2, 70, 2, 3), (4, 20), (2, 32)])
def test_blocked_layout_of_the_model_round_trips(shape):
    g = torch.Generator().manual_seed(7)
    q = torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)
    img = U.block(q, 91)
    assert torch.equal(U.unblock(img, shape), q)
    C = shape[1]
    pad = img.reshape(shape[0], -1, 16) if len(shape) == 2 else img
    if C % 16:
        assert bool((pad[..., -1, C % 16:] == 91).all() if len(shape) == 2 else (pad[:, -1, :, :, C % 16:] == 91).all())
