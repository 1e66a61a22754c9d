"""CPU: tests/_q8_model.py (the oracle of the q8 tests) held to torch's CPU quantised operators with exact equality -- quantize_per_tensor,
quantized.mul, quantized.add, quantized conv2d and linear -- over all int8 pairs, dense sweeps, and random layers with three input zero
points, with and without bias, and one contraction whose accumulator passes 2^24. No kernels are launched."""
import pytest
import torch

import _q8_cases as QC
import _q8_model as M

# (s_mu, s_sigma, s_eps, s_mul, s_add): EVERY set a fixture or a GPU case runs the weight chain at -- the seven goldens', the GPU tests'
# synthetic cases' and the two-layer model's (the rounding of float(s_sigma * s_eps / s_mul) and of 1 / s_add depends on the scale) --
# and three more: the default branch's derived scales at two other parameter scales, and one more calibrated set
_D1 = M.scales_default(0.0031, 0.0004)
_D2 = M.scales_default(0.0002, 0.0173)
SCALE_SETS = dict(QC.scale_sets())
SCALE_SETS.update({"default, mu above sigma": (0.0031, 0.0004, _D1[0][0], _D1[1][0], _D1[2][0]), "default, sigma above mu": (0.0002, 0.0173, _D2[0][0], _D2[1][0], _D2[2][0]),
                   "calibrated": (0.00217, 0.00093, 0.0291, 0.00041, 0.0029)})
IN_SETS = sorted(set(QC.in_sets()) | {(0.1, 128), (0.2, 128), (0.0437, 0), (0.0713, 57)})


def _all_pairs():
    a = torch.arange(-128, 128, dtype=torch.int32)
    return a.repeat_interleave(256).to(torch.int8), a.repeat(256).to(torch.int8)


def _q(t, s):
    return torch._make_per_tensor_quantized_tensor(t, float(s), 0)


def test_scale_sets_cover_the_fixtures():
    assert len(QC.scale_sets()) == len(QC.EXPECTED_GOLDENS) + 3 and len(set(SCALE_SETS.values())) >= 9


@pytest.mark.parametrize("name", sorted(SCALE_SETS))
def test_mul_and_add_over_all_int8_pairs(name):
    s_mu, s_sigma, s_eps, s_mul, s_add = SCALE_SETS[name]
    a, b = _all_pairs()
    ref = torch.ops.quantized.mul(_q(a, s_sigma), _q(b, s_eps), s_mul, 0).int_repr()
    assert torch.equal(M.qmul(a, b, s_sigma, s_eps, s_mul), ref)
    ref = torch.ops.quantized.add(_q(a, s_mul), _q(b, s_mu), s_add, 0).int_repr()
    assert torch.equal(M.qadd(a, b, s_mul, s_mu, s_add), ref)


def test_quantize_sweeps():
    g = torch.Generator().manual_seed(3)
    eps = torch.cat([torch.randn(1_000_000, generator=g), torch.linspace(-4.0, 4.0, 1_000_001)])
    for s in sorted({v[2] for v in SCALE_SETS.values()} | {0.0173}):
        assert torch.equal(M.quant_eps(eps, s), torch.quantize_per_tensor(eps, s, 0, torch.qint8).int_repr())
    x = torch.cat([torch.randn(1_000_000, generator=g) * 9.0, torch.linspace(-30.0, 30.0, 1_000_001)])
    for s, z in IN_SETS:
        assert torch.equal(M.quant_in(x, s, z), torch.quantize_per_tensor(x, s, z, torch.quint8).int_repr())


def _torch_layer(x, w, s_add, b, pairs, conv):
    xq = torch.quantize_per_tensor(x, pairs[3][0], pairs[3][1], torch.quint8)
    wq = _q(w, s_add)
    if conv is None:
        out = torch.nn.quantized.functional.linear(xq, wq, b, scale=pairs[4][0], zero_point=pairs[4][1])
    else:
        out = torch.nn.quantized.functional.conv2d(xq, wq, b, conv["stride"], conv["padding"], conv["dilation"], 1, scale=pairs[4][0], zero_point=pairs[4][1])
    return out.int_repr()


def _case(seed, wshape, xshape, conv, inp, outp, bias, x_mean=0.0, x_std=3.0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-128, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
    x = torch.randn(xshape, generator=g) * x_std + x_mean
    b = torch.randn(wshape[0], generator=g) * 2.0 if bias else None
    s_add = 0.0029
    pairs = [(6 / 255, 0), (0.0004, 0), (s_add, 0), inp, outp]
    return x, w, s_add, b, pairs


GEOMS = [((12, 5, 3, 3), (3, 5, 9, 9), dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1))),
         ((9, 19, 3, 3), (2, 19, 11, 10), dict(stride=(2, 2), padding=(1, 1), dilation=(1, 1))),
         ((6, 7, 3, 3), (2, 7, 12, 12), dict(stride=(1, 1), padding=(2, 2), dilation=(2, 2))),
         ((10, 70), (37, 70), None)]


@pytest.mark.parametrize("engine", [e for e in ("x86", "fbgemm", "onednn") if e in torch.backends.quantized.supported_engines])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("inp", [(0.1, 128), (0.0437, 0), (0.0713, 57)])
def test_conv_and_linear_outputs(inp, bias, engine):
    prev = torch.backends.quantized.engine
    torch.backends.quantized.engine = engine
    try:
        for i, (wshape, xshape, conv) in enumerate(GEOMS):
            if conv is not None and conv["dilation"] != (1, 1) and engine != "fbgemm":
                continue      # oneDNN's dilated quantised conv (also what "x86" picks here) corrupts the heap in torch 2.10: fbgemm only
            for outp in [(0.1, 128), (0.153, 31)]:
                x, w, s_add, b, pairs = _case(10 + i, wshape, xshape, conv, inp, outp, bias)
                ref = _torch_layer(x, w, s_add, b, pairs, conv)
                acc = M.int_conv(M.quant_in(x, *inp), inp[1], w, conv)
                got = M.requant(acc, b, pairs)
                assert 0 < int((ref > 0).sum()) and int((ref < 255).sum()) > ref.numel() // 4      # the case is not saturated away
                assert torch.equal(got, ref), (wshape, outp, int((got != ref).sum()), ref.numel())
    finally:
        torch.backends.quantized.engine = prev


@pytest.mark.parametrize("bias", [False, True])
def test_accumulator_above_2_24(bias):
    """K = 512 * 9 = 4608 with biased data: |acc| passes 2^24, where float(acc) rounds."""
    g = torch.Generator().manual_seed(5)
    w = torch.randint(90, 128, (8, 512, 3, 3), generator=g, dtype=torch.int32).to(torch.int8)
    w[4:] = -w[4:]
    w = (w.float() * (torch.arange(8).view(8, 1, 1, 1) % 4 + 1) / 4).round().to(torch.int8)      # four magnitudes of output row, both signs
    x = (torch.rand((2, 512, 4, 4), generator=g) * 4.0 + 8.0) * (torch.rand((2, 1, 4, 4), generator=g) + 0.25)
    b = torch.randn(8, generator=g) * 50.0 if bias else None
    conv = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1))
    inp = (0.1, 128)
    s_add = 0.0029
    pairs = [(6 / 255, 0), (0.0004, 0), (s_add, 0), inp, (130.0, 128)]
    acc = M.int_conv(M.quant_in(x, *inp), inp[1], w, conv)
    assert int(acc.abs().max()) > 2 ** 24
    got = M.requant(acc, b, pairs)
    ref = _torch_layer(x, w, s_add, b, pairs, conv)
    assert len(torch.unique(ref)) > 20, torch.unique(ref)
    assert torch.equal(got, ref), int((got != ref).sum())
