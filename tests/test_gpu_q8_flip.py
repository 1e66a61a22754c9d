"""GPU: the INT8 quantised Flipout layers on the fused two-contraction int8 MFMA forward (csrc/bt_q8_flip.hip) against the model
(tests/_q8_flip_model.py, itself held to torch's CPU quantised operators by test_q8_flip_model_host.py). Integer accumulation has no
order: EVERY comparison is torch.equal on the u8 image and on the fp32 output it dequantises to."""
import math

import pytest
import torch
import torch.nn as nn

import _q8_flip_cases as FC
import _q8_flip_model as FM

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


def _launch(c, shared=True, draws=True, **kw):
    from bayesian_torch_amd import functional as F
    packs = F.q8_pack(_dev(c["q_mu"]), _dev(c["q_sigma"]))
    x = c["x"][0] if shared else c["x"].reshape((-1,) + tuple(c["x"].shape[2:]))
    d = {k: _dev(c[k]) for k in ("eps_w", "eps_b", "sign_in", "sign_out")} if draws else {}
    return F.q8_flip_forward(_dev(x), packs, c["wshape"], FC.S_MU, FC.S_SIGMA, c["pairs"], _dev(c["mu_b"]), _dev(c["sigma_b"]), conv=c["conv"], S=c["S"],
                             shared_x=shared, want_q=True, **d, **kw)


def _same(out, out_q, want_q, want, what):
    torch.cuda.synchronize()
    bad = int((out_q.cpu() != want_q).sum())
    print(f"{what}: {want_q.numel()} outputs, {len(torch.unique(want_q))} distinct levels, {bad} differ")
    assert torch.equal(out_q.cpu(), want_q), (what, bad)
    assert torch.equal(out.cpu(), want), what


# ---------------------------------------------------------------------------- 1. supplied draws against the model
@pytest.mark.parametrize("name,kind,bias,x_std", FC.LAYER_CASES)
def test_supplied_draw_equals_model(name, kind, bias, x_std):
    """Both tile edges and a partial last stage (conv_c37x70k3p1_9x7), stride / dilation, the 1 x 1 map whose padding-only taps are
    pruned (all zero points 128) and must not be (z_xp = 120), Linear; the three bias forms; the default pairs, a dict with every zero
    point != 128, x' = 256 -> 255, both clamp ends of o1, p, p' and oq, umul ties (test_q8_flip_model_host.py shows the cases reach them)."""
    from bayesian_torch_amd import _lib
    c = FC.case(name, kind, bias, 1, x_std)
    want_q, want, _ = FC.model(c)
    out, out_q = _launch(c)
    assert _lib.lib().bt_last_kernel_name().decode() == "q8_flip_fwd<i8 32x32x32,64x128,draws injected>"
    _same(out, out_q, want_q, want, f"{name} {kind} bias={bias}")


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("bias", ["full", "none", "mu_only"])
@pytest.mark.parametrize("name", ["conv_c5x6k3s2d2p2_8x5", "linear_70x10_b3"])
def test_three_samples_shared_and_per_sample_x(name, bias, shared):
    """S = 3 at sample0 = 5 (supplied draws do not depend on it): each sample reads its own draws, signs and -- per-sample x -- input."""
    c = FC.case(name, "dict", bias, 3, 1.5)
    want_q, want, _ = FC.model(c, shared_x=shared)
    out, out_q = _launch(c, shared=shared, sample0=5)
    _same(out, out_q, want_q, want, f"{name} bias={bias} S=3 shared={shared}")


def test_sign_tensor_convention():
    """A negative value means -1, anything else +1: magnitudes do not matter, +0 is +1."""
    c = dict(FC.case("linear_70x10_b3", "dict", "full", 1, 1.5))
    want_q, want, _ = FC.model(FC.case("linear_70x10_b3", "dict", "full", 1, 1.5))
    c["sign_in"] = torch.where(c["sign_in"] < 0, -0.25, 0.0)
    c["sign_out"] = torch.where(c["sign_out"] < 0, -7.0, 3.0)
    out, out_q = _launch(c)
    _same(out, out_q, want_q, want, "scaled sign tensors")


# ---------------------------------------------------------------------------- 1b. the walk's edge geometries (tests/_q8_edges.py, F)
@pytest.mark.parametrize("name,kind,bias,x_std", FC.EDGE_CASES)
def test_edge_geometry_supplied_draw_equals_model(name, kind, bias, x_std):
    """k3x5_2x7_uneven: two channel tiles, two pixel tiles, every stride / padding / dilation pair uneven -- with the default pairs (taps
    pruned) and the 'dict' pairs (nothing pruned, padding corrected through both row sums); k5x5_2x2_p2: 25 taps, so no pruning at zero
    points 128: padding is a true zero in both contractions; k2x8_3x2_p1x7: a pixel tile crosses images, and with it both sign offsets
    (test_q8_flip_model_host.py shows the cases are what they are for)."""
    c = FC.case(name, kind, bias, 1, x_std)
    want_q, want, _ = FC.model(c)
    assert len(torch.unique(want_q)) > 16       # the case is not saturated away
    out, out_q = _launch(c)
    _same(out, out_q, want_q, want, f"{name} {kind} bias={bias}")


def test_pruned_16_tap_geometry_on_chip_draws_equal_the_filled_streams():
    """k4x4_2x1_s2p3, zero points 128: eight of 16 taps are walked, and the draw of a walked unit is indexed by its TAP, not by its
    position in the walk -- the launch equals one fed the filled streams (tensors 0 to 3), and the model on them."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    name, kind, bias, x_std = FC.ON_CHIP_EDGE
    c = dict(FC.case(name, kind, bias, 2, x_std))
    assert FC.pruned(c)
    coords = dict(seed=0x5EED0F00D, call=6, layer_id=3, sample0=2)
    out, out_q = _launch(c, draws=False, **coords)
    assert _lib.lib().bt_last_kernel_name().decode() == "q8_flip_fwd<i8 32x32x32,64x128,draws on chip>"
    fill = lambda fn, tensor, shape: fn(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], tensor, 2, tuple(shape), DEV)
    c["eps_w"], c["eps_b"] = fill(F.rng_fill_normal, 0, c["wshape"]), fill(F.rng_fill_normal, 1, (c["wshape"][0],))
    c["sign_in"], c["sign_out"] = fill(F.rng_fill_sign, 2, c["x"].shape[1:]), fill(F.rng_fill_sign, 3, (c["x"].shape[1],) + tuple(out.shape[1:]))
    out2, out_q2 = _launch(c)
    torch.cuda.synchronize()
    assert torch.equal(out_q, out_q2) and torch.equal(out, out2)
    c = {k: v.cpu() if k in ("eps_w", "eps_b", "sign_in", "sign_out") else v for k, v in c.items()}
    want_q, want, _ = FC.model(c)
    assert len(torch.unique(want_q)) > 16
    _same(out, out_q, want_q, want, f"{name} on chip, S=2")
    per = out_q.shape[0] // 2
    assert not torch.equal(out_q[:per], out_q[per:])      # the samples differ


def test_guard_bands_on_a_pruned_geometry():
    """k3x3_1x5, S = 2, three live taps (VU = 6: no multiple of the stage): nothing is written outside out and out_q, every element of
    out is written, and sign_in and sign_out lie between NaN bands at an odd offset; the packs stay 16-byte aligned."""
    import _guard as G
    name, kind, bias, x_std = FC.GUARD_EDGE
    c = dict(FC.case(name, kind, bias, 2, x_std))
    want_q, want, _ = FC.model(c)
    assert FC.pruned(c) and len(torch.unique(want_q)) > 16
    c["sign_in"], c["sign_out"] = G.place(c["sign_in"].to(DEV), 1), G.place(c["sign_out"].to(DEV), 3)
    with G.guarded_allocations(lambda shape, dtype: 0 if dtype == torch.int8 else 1) as log:      # (the packs must be 16-byte aligned)
        out, out_q = _launch(c)
    torch.cuda.synchronize()
    assert {g.view.dtype for g in log} == {torch.int8, torch.float32, torch.uint8}      # the packs, out, out_q
    G.check_all(log)
    _same(out, out_q, want_q, want, f"{name} between guard bands, S=2")


# ---------------------------------------------------------------------------- 2. the layers: on-chip draws, materialize_last_draw
def _layer_of(c):
    """A quantised Flipout layer holding a case's images, scales, bias tensors and pairs (a checkpoint load), on the device."""
    import bayesian_torch_amd.layers as L
    w = c["wshape"]
    if c["conv"] is None:
        q = L.QuantizedLinearFlipout(w[1], w[0])
    else:
        q = L.QuantizedConv2dFlipout(w[1], w[0], w[2], c["conv"]["stride"], c["conv"]["padding"], c["conv"]["dilation"])
    sd = dict(quantized_mu_weight=c["q_mu"], quantized_sigma_weight=c["q_sigma"], quantized_mu_scale=torch.tensor([FC.S_MU], dtype=torch.float32),
              quantized_sigma_scale=torch.tensor([FC.S_SIGMA], dtype=torch.float32))
    if c["mu_b"] is not None:
        sd["quantized_mu_bias"] = c["mu_b"]
    if c["sigma_b"] is not None:
        sd["quantized_sigma_bias"] = c["sigma_b"]
    q.load_state_dict(sd)
    q.quant_dict = [dict(scale=s, zero_point=z) for s, z in c["pairs"]]
    q.want_q = True
    return q.to(DEV)


def _model_of_layer(q, x, d, s, conv):
    """The model's (u8, fp32) of layer ``q`` for sample s of the draw ``d`` (materialize_last_draw's), at the layer's own fp32 scales."""
    cpu = lambda t: None if t is None else t.detach().cpu()
    r = FM.forward(cpu(x), cpu(q.quantized_mu_weight), cpu(q.quantized_sigma_weight), float(q.quantized_mu_scale.item()), float(q.quantized_sigma_scale.item()),
                   q._last["pairs"], cpu(d["eps_w"][s]), cpu(d["sign_in"][s]), cpu(d["sign_out"][s]), cpu(q.quantized_mu_bias), cpu(q.quantized_sigma_bias),
                   None if d["eps_b"] is None else cpu(d["eps_b"][s]), conv)
    return r[0], r[1]


@pytest.mark.parametrize("name,kind,bias", [("conv_c37x70k3p1_9x7", "dict", "full"), ("conv_c5x6k3s2d2p2_8x5", "default", "mu_only"), ("linear_70x10_b3", "dict", "full")])
def test_on_chip_draws_equal_a_launch_fed_the_materialised_draw(name, kind, bias):
    from bayesian_torch_amd import mc, rng
    c = FC.case(name, kind, bias, 1, 1.5)
    q = _layer_of(c)
    x = c["x"][0].to(DEV)
    S = 3
    rng.set_mode("philox")
    rng.manual_seed(0x1234ABCD5678)
    rng.set_call(9)
    q.dnn_to_bnn_flag = True
    out = mc.mc_forward(q, x, S, sample0=5, with_kl=False)[0]
    torch.cuda.synchronize()
    assert q._last["kernel"] == "q8_flip_fwd<i8 32x32x32,64x128,draws on chip>" and q._last["S"] == S and q._last["shared_x"] is True
    out_q = q._last["out_q"].clone()
    d = q.materialize_last_draw()
    assert set(d) == {"eps_w", "eps_b", "sign_in", "sign_out"} and tuple(d["sign_in"].shape) == (S,) + tuple(x.shape)
    assert tuple(d["sign_out"].shape) == tuple(out.shape)
    for k in ("sign_in", "sign_out"):
        assert bool((d[k].abs() == 1).all()) and 0.3 < float((d[k] < 0).float().mean()) < 0.7
        assert not torch.equal(d[k][0], d[k][1])                    # one x for all samples, yet each sample has its own signs
    q.inject_draw = d
    out2 = mc.mc_forward(q, x, S, with_kl=False)[0]
    torch.cuda.synchronize()
    assert q._last["kernel"].endswith("draws injected>")
    assert torch.equal(q._last["out_q"], out_q) and torch.equal(out2, out)
    ref = [_model_of_layer(q, x, d, s, c["conv"]) for s in range(S)]
    want_q = torch.cat([r[0] for r in ref], 0)
    _same(out.reshape(want_q.shape), out_q, want_q, torch.cat([r[1] for r in ref], 0), f"{name} on chip, S=3")
    per = out_q.shape[0] // S
    assert not torch.equal(out_q[:per], out_q[per:2 * per])


def test_torch_rng_mode_draws_eps_w_eps_b_sign_in_sign_out_per_sample():
    """rng mode "torch": the draw comes from torch's generator on the device -- eps_w, eps_b, sign_in, sign_out, sample by sample -- and
    is the one the launch reads: the same seed drawn by hand in that order gives the tensors materialize_last_draw returns, and the
    output is the model's on them."""
    from bayesian_torch_amd import mc, rng
    c = FC.case("conv_c5x6k3s2d2p2_8x5", "dict", "full", 1, 1.5)
    q = _layer_of(c)
    q.dnn_to_bnn_flag = True
    x = c["x"][0].to(DEV)
    S = 2
    rng.set_mode("torch")
    try:
        torch.manual_seed(31)
        out = mc.mc_forward(q, x, S, with_kl=False)[0]
        torch.cuda.synchronize()
    finally:
        rng.set_mode("philox")
    d = q.materialize_last_draw()
    assert q._last["kernel"].endswith("draws injected>")
    torch.manual_seed(31)
    for s in range(S):
        want = [torch.empty(c["wshape"], device=DEV).normal_(), torch.empty(c["wshape"][0], device=DEV).normal_(),
                torch.empty(tuple(x.shape), device=DEV).uniform_(-1, 1).sign_(), torch.empty(tuple(out.shape[1:]), device=DEV).uniform_(-1, 1).sign_()]
        for k, w in zip(("eps_w", "eps_b", "sign_in", "sign_out"), want):
            assert torch.equal(d[k][s], w), (k, s)
    ref = [_model_of_layer(q, x, d, s, c["conv"]) for s in range(S)]
    want_q = torch.cat([r[0] for r in ref], 0)
    _same(out.reshape(want_q.shape), q._last["out_q"], want_q, torch.cat([r[1] for r in ref], 0), "torch rng mode, S=2")


# ---------------------------------------------------------------------------- 3. a converted model under mc_forward and McGraph
class _Block(nn.Module):
    def __init__(self, L, cin, planes, stride):
        super().__init__()
        self.conv1 = L.Conv2dFlipout(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = L.Conv2dFlipout(planes, planes, 3, 1, 1, bias=True)
        self.bn2 = nn.BatchNorm2d(planes)

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))))


class _Net(nn.Module):
    def __init__(self, L):
        super().__init__()
        self.layer1 = _Block(L, 3, 6, 1)
        self.layer2 = _Block(L, 6, 8, 2)
        self.fc = L.LinearFlipout(8 * 3 * 3, 4)

    def forward(self, x):
        return self.fc(torch.flatten(self.layer2(self.layer1(x)), 1))


def _toy_net(x_probe):
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    torch.manual_seed(23)
    net = _Net(L)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5), m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.2), m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
            elif hasattr(m, "rho_kernel"):
                m.rho_kernel.fill_(-2.0)
            elif hasattr(m, "rho_weight"):
                m.rho_weight.fill_(-2.0)
    net.eval()
    for m in net.modules():
        if hasattr(m, "dnn_to_bnn_flag"):
            m.dnn_to_bnn_flag = True
    rng.assign_layer_ids(net)
    bnn_to_qbnn(net, fuse_conv_bn=True, flipout=True)
    layers = [net.layer1.conv1, net.layer1.conv2, net.layer2.conv1, net.layer2.conv2, net.fc]
    assert [type(m).__name__ for m in layers] == ["QuantizedConv2dFlipout"] * 4 + ["QuantizedLinearFlipout"]
    assert all(type(b).__name__ == "Identity" for b in (net.layer1.bn1, net.layer1.bn2, net.layer2.bn1, net.layer2.bn2))
    # a quant_dict per layer from the ranges of the float Flipout formula's intermediates on one CPU pass with draws of its own
    # (observer_qparams: symmetric for eps and delta, affine for the other eight), so that every layer's levels span their range
    from bayesian_torch_amd.quantization.quantize import observer_qparams
    g = torch.Generator().manual_seed(5)
    h = x_probe
    for i, m in enumerate(layers):
        if i == 4:
            h = torch.flatten(h, 1)
        deq = lambda q, sc: q.float() * float(sc.item())
        mu, sigma = deq(m.quantized_mu_weight, m.quantized_mu_scale), deq(m.quantized_sigma_weight, m.quantized_sigma_scale)
        conv = m._conv()
        oshape = FM.float_flipout(h, mu, sigma, torch.zeros_like(mu), torch.ones_like(h), torch.ones(1), conv=conv)[0].shape
        rnd = lambda shape: torch.randn(shape, generator=g)
        sgn = lambda shape: torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        sb = m.quantized_sigma_bias
        out, mid = FM.float_flipout(h, mu, sigma, rnd(mu.shape), sgn(h.shape), sgn(oshape), m.quantized_mu_bias, sb, None if sb is None else rnd(sb.shape), conv)
        keys = ("eps", "delta", "inp", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")
        qp = [observer_qparams(mid[k].min().float(), mid[k].max().float(), torch.qint8 if j < 2 else torch.quint8) for j, k in enumerate(keys)]
        m.quant_dict = [dict(scale=float(sc), zero_point=int(zp)) for sc, zp in qp]
        h = torch.relu(out.float())
    return net.to(DEV), layers


def _model_chain(layers, x, S):
    """The per-layer model applied sample by sample with the draws the layers' last forward made -> fp32 logits [S, B, 4]."""
    draws = [m.materialize_last_draw() for m in layers]
    outs = []
    for s in range(S):
        h = x
        for i, (m, d) in enumerate(zip(layers, draws)):
            if i == 4:
                h = torch.flatten(h, 1)
            h = _model_of_layer(m, h, d, s, m._conv())[1]
            if i < 4:
                h = torch.relu(h)
        outs.append(h)
    return torch.stack(outs)


def test_converted_model_under_mc_forward_and_graph_replay():
    from bayesian_torch_amd import mc, rng
    x = torch.randn(3, 3, 6, 6, generator=torch.Generator().manual_seed(4)) * 1.5
    net, layers = _toy_net(x)
    S = 3
    rng.set_mode("philox")
    rng.manual_seed(99)
    rng.set_call(40)
    with torch.no_grad():
        logits, kl = mc.mc_forward(net, x.to(DEV), S)
    torch.cuda.synchronize()
    assert kl is None and tuple(logits.shape) == (S, 3, 4)
    assert layers[0]._last["shared_x"] is True and layers[1]._last["shared_x"] is False and all(m._last["kernel"].endswith("draws on chip>") for m in layers)
    want = _model_chain(layers, x, S)
    assert len(torch.unique(want)) > 8 and torch.equal(logits.cpu(), want)
    graph = mc.McGraph(net, x.to(DEV), S, with_kl=False, epilogue=False)
    rng.set_call(40)                       # a replay draws what an eager mc_forward at this position draws
    got = graph.replay()[0]
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)
    got2 = graph.replay()[0].clone()       # the next replay: the next calls, fresh draws
    rng.set_call(40 + len(layers))
    with torch.no_grad():
        again = mc.mc_forward(net, x.to(DEV), S)[0]
    torch.cuda.synchronize()
    assert torch.equal(got2, again) and not torch.equal(got2.cpu(), want)


# ---------------------------------------------------------------------------- 4. the output signs are fair coins
def test_output_signs_are_a_fair_coin():
    """One launch of B = 2048 rows x 128 outputs = 262 144 output signs, read off the kernel's OUTPUT: q_mu = 0 and mu_b = 0 make the
    mean path the constant z_mean, q_sigma = 0 leaves p = requant(0, sigma_b * eps_b), whose sign per channel is eps_b's (regenerated
    from tensor 1's stream), and the scales make oq - z_out = sign_out * (p - z_pert). Elements with p = z_pert (a channel property,
    independent of the sign) carry no sign and are left out; the count used is printed and the fraction of -1 held to 1/2 at 5 sigma
    of that count: |f - 1/2| <= 5 * 0.5 / sqrt(N). The same signs must be bt_rng_sign_fill's."""
    from bayesian_torch_amd import functional as F
    B, In, Out = 2048, 16, 128
    q0 = torch.zeros((Out, In), dtype=torch.int8, device=DEV)
    packs = F.q8_pack(q0, q0)
    s = 0.05
    pairs = [(6 / 255, 0), (0.01, 0), (0.1, 128), (s, 128), (0.1, 128), (0.1, 128), (0.1, 128), (s, 128), (s, 128), (s, 128)]
    mu_b = torch.zeros(Out, device=DEV)
    sigma_b = torch.full((Out,), 20 * s, device=DEV)
    coords = dict(seed=20261020, call=3, layer_id=6, sample0=2)
    out, out_q = F.q8_flip_forward(torch.randn(B, In, device=DEV), packs, (Out, In), 0.01, 0.01, pairs, mu_b, sigma_b, want_q=True, **coords)
    eps_b = F.rng_fill_normal(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], 1, 1, (Out,), DEV)[0]
    fill = F.rng_fill_sign(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], 3, 1, (B, Out), DEV)[0]
    torch.cuda.synchronize()
    lv = out_q.cpu().to(torch.int32) - 128
    p = torch.clamp(torch.round(20.0 * eps_b.cpu()), -128, 127)          # (a tie or an ulp of the model's fp32 chain could move p by one level, never its sign)
    carries = (lv != 0) & (p.abs() >= 2).view(1, -1)
    sign = torch.sign(lv.float()) * torch.sign(p).view(1, -1)
    N = int(carries.sum())
    neg = int(((sign < 0) & carries).sum())
    f = neg / N
    print(f"{N} output signs of {B * Out} read off one launch: {neg} are -1, fraction {f:.5f}, 5 sigma = {2.5 / math.sqrt(N):.5f}")
    assert N > 0.9 * B * Out
    assert abs(f - 0.5) <= 5 * 0.5 / math.sqrt(N)
    assert torch.equal(sign[carries], fill.cpu()[carries])
