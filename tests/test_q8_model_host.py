"""CPU: tests/_q8_model.py (the oracle of the q8 tests) held to torch's CPU quantised operators with exact equality -- quantize_per_tensor,
quantized.mul, quantized.add, quantized conv2d and linear -- over all int8 pairs, dense sweeps, and random layers with three input zero
points, with and without bias, and one contraction whose accumulator passes 2^24. No kernels are launched."""
import pytest
import torch

import _q8_cases as QC
import _q8_edges as E
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
    assert len(QC.scale_sets()) == len(QC.EXPECTED_GOLDENS) + 3 + len(QC.TIE_SETS) and len(QC.TIE_SETS) >= 2 and len(set(SCALE_SETS.values())) >= 12
    assert {(QC.DYADIC_S_IN, z) for z in (128, 0, 57)} <= set(IN_SETS)


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
    half = torch.arange(-300, 300, dtype=torch.float64) + 0.5      # half steps (n + 0.5) * s past both clamp ends: exact ties where s is dyadic
    ties = 0
    for s in sorted({v[2] for v in SCALE_SETS.values()} | {0.0173}):
        e = torch.cat([eps, (half * s).float()])
        ties += int((e[-600:] * M.rcp32(s) == half.float()).sum())
        assert torch.equal(M.quant_eps(e, s), torch.quantize_per_tensor(e, s, 0, torch.qint8).int_repr())
    assert ties >= 2 * 600                                         # (the two dyadic eps scales give 600 exact ties each)
    x = torch.cat([torch.randn(1_000_000, generator=g) * 9.0, torch.linspace(-30.0, 30.0, 1_000_001)])
    ties = 0
    for s, z in IN_SETS:
        xs = torch.cat([x, (half * s).float()])
        ties += int((xs[-600:] * M.rcp32(s) == half.float()).sum())
        assert torch.equal(M.quant_in(xs, s, z), torch.quantize_per_tensor(xs, s, z, torch.quint8).int_repr())
    assert ties >= 3 * 600


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


# ---------------------------------------------------------------------------- exact requantisation ties (output multiplier 0.5)
def _with_engine(engine, fn):
    prev = torch.backends.quantized.engine
    torch.backends.quantized.engine = engine
    try:
        return fn()
    finally:
        torch.backends.quantized.engine = prev


@pytest.mark.parametrize("bias", E.REQ_TIE_BIASES)
@pytest.mark.parametrize("zi", range(len(E.ZPAIRS)))
@pytest.mark.parametrize("shape", ["linear", "conv", "conv_undilated"])
def test_requantisation_ties_are_fbgemms(shape, zi, bias):
    """s_in = 2^-4, s_add = 2^-7, s_out = 2^-10 ('half_decimal': s_add = 0.006, s_out = s_add / 8): float(acc) * 0.5 (+ a half-integer
    bias term) is an exact tie for half of the accumulators. The contract there is fbgemm's -- the fp32 value rounded to nearest even -- and the model meets it on EVERY element.
    oneDNN rounds such ties by a rule of its own (none of to-even, half-away, half-up, half-down): the model is held to it off the ties
    only ('half_decimal': off the values within two ulps of one), and the counts are printed; that it differs at ties is torch's business
    and is not asserted. The dilated geometry runs under
    fbgemm only (test_conv_and_linear_outputs has the reason)."""
    c = E.requant_case(shape, zi, bias)
    conv, got = c["conv"], c["oq"]
    pre = E.run(c, 0)["pre"]["oq"]
    tie = (pre - torch.floor(pre) - 0.5).abs() <= 2.0 ** -15      # on a half step, or ('half_decimal') within two fp32 ulps of one: |pre| < 512
    st = E.stats(c)["oq"]
    assert 4 * int(tie.sum()) >= got.numel(), (int(tie.sum()), got.numel())
    ref = _with_engine("fbgemm", lambda: _torch_layer(c["x"], c["q_mu"], c["pairs"][2][0], c["mu_b"], c["pairs"], conv))
    print(f"{shape} z={E.ZPAIRS[zi]} bias={bias}: {got.numel()} outputs, {int(tie.sum())} ties, clamp ends {st['lo']} / {st['hi']}; fbgemm misses {int((got != ref).sum())}")
    assert torch.equal(got, ref)
    if "onednn" in torch.backends.quantized.supported_engines and (conv is None or conv["dilation"] == (1, 1)):
        ref = _with_engine("onednn", lambda: _torch_layer(c["x"], c["q_mu"], c["pairs"][2][0], c["mu_b"], c["pairs"], conv))
        miss = got != ref
        print(f"    onednn: {int(miss.sum())} misses, {int((miss & tie).sum())} of them at the {int(tie.sum())} ties")
        assert not bool((miss & ~tie).any()), int((miss & ~tie).sum())


@pytest.mark.parametrize("as_conv", [False, True])
@pytest.mark.parametrize("i", range(len(E.NEAR)))
def test_output_stage_beside_ties_is_fbgemms(i, as_conv):
    """Non-dyadic multipliers, every unclamped output on or an ulp or two beside a tie (E.near_case): what decides them is fbgemm's
    output stage to the last bit -- a = f32(s_in) * f32(s_add) and m = a / f32(s_out) as fp32 operations (NOT the double quotient rounded
    once: for these scales the two differ), and fma(b, 1 / a, float(acc)) * m with ONE rounding of the sum. Each other reading misses
    hundreds of these outputs; the counts are printed."""
    c = E.near_case(i, as_conv)
    s_in, s_add, s_out = c["pairs"][3][0], c["pairs"][2][0], c["pairs"][4][0]
    assert M.out_scales(s_in, s_add, s_out)[1] != M.f32(float(s_in) * float(s_add) / float(s_out))
    assert torch.equal(E.run(c, 0)["w"], c["q_mu"].to(torch.int32))
    ref = _with_engine("fbgemm", lambda: _torch_layer(c["x"], c["q_mu"], s_add, c["mu_b"], c["pairs"], c["conv"]))
    live = int(((ref > 0) & (ref < 255)).sum())
    others = {m: int((E.run_oq(c, m) != ref.to(torch.int32)).sum()) for m in ("m_double", "bias_after_m", "unfused_oq", "div_out")}
    print(f"near {i} {'conv' if as_conv else 'linear'}: {ref.numel()} outputs, {live} unclamped; fbgemm misses {int((c['oq'] != ref).sum())}; other readings miss {others}")
    assert live > ref.numel() // 4 and torch.equal(c["oq"], ref)
    assert all(v >= ref.numel() // 100 for k, v in others.items() if k in ("m_double", "bias_after_m"))
