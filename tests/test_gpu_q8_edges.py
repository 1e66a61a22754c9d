"""GPU: the fused int8 forward (csrc/bt_q8.hip) on the edge cases of tests/_q8_edges.py -- exact ties at each of its five roundings, both
ends of each clamp, uneven geometry (KH != KW, sh != sw, ph != pw, dh != dw), tap pruning with several live taps, at its 16-tap limit
and switched off above it -- against the model (tests/_q8_model.py, held to torch's CPU quantised operators on these very scale sets
by test_q8_model_host.py). tests/test_q8_edges_host.py shows on the CPU that a subtly wrong implementation changes these cases' answers.
Every comparison is torch.equal on the u8 image and on the fp32 output; every count asserted here is the model's, taken before the launch."""
import pytest
import torch

import _guard as G
import _q8_cases as QC
import _q8_edges as E
import _q8_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
INJECTED, ON_CHIP = "q8_fwd<i8 32x32x32,64x128,eps injected>", "q8_fwd<i8 32x32x32,64x128,eps on chip>"


def _dev(t):
    return None if t is None else t.to(DEV)


def _launch(c, eps=True, **kw):
    from bayesian_torch_amd import functional as F
    packs = F.q8_pack(_dev(c["q_mu"]), _dev(c["q_sigma"]))
    return F.q8_forward(_dev(c["x"]), packs, c["wshape"], c["s_mu"], c["s_sigma"], c["pairs"], _dev(c["mu_b"]), _dev(c["sigma_b"]), conv=c["conv"], S=c["S"],
                        shared_x=c["shared_x"], eps_w=_dev(c["eps_w"]) if eps else None, eps_b=_dev(c["eps_b"]) if eps else None, want_q=True, **kw)


def _same(out, out_q, c, what):
    from bayesian_torch_amd import _lib
    torch.cuda.synchronize()
    assert _lib.lib().bt_last_kernel_name().decode() == INJECTED
    bad = int((out_q.cpu() != c["oq"]).sum())
    print(f"{what}: {c['oq'].numel()} outputs, {len(torch.unique(c['oq']))} distinct levels, {bad} differ")
    assert torch.equal(out_q.cpu(), c["oq"]), (what, bad)
    assert torch.equal(out.cpu(), c["out"]), what


# ---------------------------------------------------------------------------- C. the weight chain, read out
@pytest.mark.parametrize("pat", E.CHAIN_PATTERNS)
@pytest.mark.parametrize("name", sorted(E.scale_sets()))
def test_weight_chain_read_out(name, pat):
    """x = eye, input pair (1, 128), output pair (s_add, 128): oq - 128 is the sampled int8 weight itself, all 65 536 of each of two
    samples -- every value of q_mu, p over all 256 values, e past both clamp ends; at the tie sets every e (and thousands of p and w) an
    exact tie."""
    c = E.chain_case(name, pat)
    sets = E.scale_sets()[name]
    w = torch.stack([M.sampled_weight(c["q_mu"], c["q_sigma"], c["eps_w"][s], *sets) for s in range(2)])
    assert len(torch.unique(w)) > 128
    out, out_q = _launch(c)
    _same(out, out_q, c, f"chain[{name}] pattern {pat}")
    assert torch.equal(out_q.cpu().view(2, E.CHAIN_N, E.CHAIN_N).to(torch.int32) - 128, w.transpose(1, 2).to(torch.int32))


# ---------------------------------------------------------------------------- D. the input quantiser, read out
@pytest.mark.parametrize("z", E.Z_INS)
@pytest.mark.parametrize("kind", list(E.INQ_KINDS))
def test_input_quantiser_read_out(kind, z):
    """An identity weight and an output multiplier of exactly 1: oq is xq -- 13 440 half steps of s_in past both clamp ends, two thirds
    of them exact ties at the dyadic scale."""
    c = E.inq_case(kind, z)
    s = E.stats(c)["xq"]
    assert s["lo"] >= 100 and s["hi"] >= 100 and (kind != "dyadic" or s["ties"] >= 1000)
    out, out_q = _launch(c)
    _same(out, out_q, c, f"input quantiser, {kind} scale, z_in={z}")
    assert torch.equal(out_q.cpu(), M.quant_in(c["x"], *c["pairs"][3]))


# ---------------------------------------------------------------------------- E. requantisation ties and clamps
@pytest.mark.parametrize("bias", E.REQ_TIE_BIASES)
@pytest.mark.parametrize("zi", range(len(E.ZPAIRS)))
@pytest.mark.parametrize("shape", ["linear", "conv"])
def test_requantisation_ties(shape, zi, bias):
    """Output multiplier exactly 0.5: about half of the outputs are exact ties (fbgemm's rule: to even), with and without a bias of
    half-integer multiples of s_out; the three zero-point pairs reach both output clamps."""
    c = E.requant_case(shape, zi, bias)
    assert 4 * E.stats(c)["oq"]["ties"] >= c["oq"].numel()
    out, out_q = _launch(c)
    _same(out, out_q, c, f"requant {shape} z={E.ZPAIRS[zi]} bias={bias}")


@pytest.mark.parametrize("as_conv", [False, True])
@pytest.mark.parametrize("i", range(len(E.NEAR)))
def test_output_stage_beside_ties(i, as_conv):
    """Non-dyadic multipliers with every unclamped output on or an ulp or two beside a tie: the fp32 a = s_in * s_add and m = a / s_out,
    the reciprocal of a, and the ONE rounding of fma(b, 1 / a, float(acc)) each decide outputs here (fbgemm's, held on the CPU)."""
    c = E.near_case(i, as_conv)
    assert int(((c["oq"] > 0) & (c["oq"] < 255)).sum()) > c["oq"].numel() // 4
    out, out_q = _launch(c)
    _same(out, out_q, c, f"near ties {i} {'conv' if as_conv else 'linear'}")


@pytest.mark.parametrize("shape", ["linear", "conv"])
def test_requantisation_with_a_full_bias_on_decimal_scales(shape):
    c = E.requant_case(shape, 2, "full")
    assert len(torch.unique(c["oq"])) > 16
    out, out_q = _launch(c)
    _same(out, out_q, c, f"requant {shape} full bias")


# ---------------------------------------------------------------------------- F. uneven geometry and tap pruning
@pytest.mark.parametrize("z_in", E.Z_INS)
@pytest.mark.parametrize("name", list(E.GEOMS))
def test_uneven_geometry_injected_draw_equals_model(name, z_in):
    c = E.geom_case(name, z_in)
    assert len(torch.unique(c["oq"])) > 16       # the case is not saturated away
    out, out_q = _launch(c)
    _same(out, out_q, c, f"{name} z_in={z_in}")


@pytest.mark.parametrize("name", ["k3x5_2x7_uneven", "k4x4_2x1_s2p3"])
def test_pruned_geometry_on_chip_draws_equal_the_filled_streams(name):
    """z_in = 128: the taps are pruned, and the draw of a walked unit is indexed by its TAP, not by its position in the walk."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    c = dict(E.geom_case(name, 128, 2))
    coords = dict(seed=0x5EED0F00D, call=6, layer_id=3, sample0=2)
    out, out_q = _launch(c, eps=False, **coords)
    assert _lib.lib().bt_last_kernel_name().decode() == ON_CHIP
    eps_w = F.rng_fill_normal(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], 0, 2, c["wshape"], DEV)
    eps_b = F.rng_fill_normal(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], 1, 2, (c["wshape"][0],), DEV)
    c["eps_w"], c["eps_b"] = eps_w, eps_b
    out2, out_q2 = _launch(c)
    torch.cuda.synchronize()
    assert torch.equal(out_q, out_q2) and torch.equal(out, out2)
    ref = [M.forward(c["x"], c["q_mu"], c["q_sigma"], c["s_mu"], c["s_sigma"], c["pairs"], eps_w[s].cpu(), c["mu_b"], c["sigma_b"], eps_b[s].cpu(), c["conv"])[0] for s in range(2)]
    assert torch.equal(out_q.cpu(), torch.cat(ref, 0))
    per = out_q.shape[0] // 2
    assert not torch.equal(out_q[:per], out_q[per:])      # the samples differ


def test_stacked_input_on_uneven_geometry():
    """S = 2 with shared_x=False: one x per sample, at the functional level."""
    c = E.geom_case("k3x2_9x7_uneven", 57, 2, True)
    assert not c["shared_x"] and c["x"].shape[0] == 2 * E.GEOMS["k3x2_9x7_uneven"][3] and not torch.equal(*c["x"].chunk(2, 0))
    out, out_q = _launch(c)
    _same(out, out_q, c, "k3x2_9x7_uneven, stacked x, S=2")


@pytest.mark.parametrize("name,off", [("k3x3_1x5", 1), ("k4x4_2x1_s2p3", 3)])
def test_guard_bands_on_pruned_geometries(name, off):
    c = E.geom_case(name, 128, 2)
    with G.guarded_allocations(lambda shape, dtype: 0 if dtype == torch.int8 else off) as log:      # (the packs must be 16-byte aligned)
        out, out_q = _launch(c)
    torch.cuda.synchronize()
    assert {g.view.dtype for g in log} == {torch.int8, torch.float32, torch.uint8}      # the packs, out, out_q
    G.check_all(log)
    assert torch.equal(out_q.cpu(), c["oq"]) and torch.equal(out.cpu(), c["out"])


@pytest.mark.parametrize("z_in", E.Z_INS)
def test_converted_layer_with_tuple_geometry(z_in):
    """A Conv2dReparameterization built with tuple kernel_size / stride / padding / dilation, converted by qbnn_conv_layer: the tuples
    reach the kernel in their order."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.models.bnn_to_qbnn import qbnn_conv_layer
    torch.manual_seed(33)
    d = L.Conv2dReparameterization(20, 9, kernel_size=(3, 2), stride=(2, 1), padding=(1, 0), dilation=(1, 2), bias=True)
    with torch.no_grad():
        d.rho_kernel.fill_(-2.0)
    q = qbnn_conv_layer(d).to(DEV)
    assert tuple(q.quantized_mu_weight.shape) == (9, 20, 3, 2)
    s_mu, s_sigma = float(q.quantized_mu_scale.item()), float(q.quantized_sigma_scale.item())
    q.quant_dict = [dict(scale=s, zero_point=z) for s, z in [(0.0291, 0), (s_sigma * 0.0291, 0), (max(s_sigma * 0.0291, s_mu), 0), (QC.GPU_S_IN, z_in), (0.03, 121)]]
    q.want_q = True
    x = torch.randn(7, 20, 9, 7, generator=torch.Generator().manual_seed(z_in)) * 1.5
    rng.manual_seed(5)
    with torch.no_grad():
        out, kl = q(x.to(DEV))
    torch.cuda.synchronize()
    assert kl == 0 and q._last["kernel"].startswith("q8_fwd<") and q._conv() == dict(stride=(2, 1), padding=(1, 0), dilation=(1, 2), groups=1)
    dr = q.materialize_last_draw()
    oq, want = QC.model_of_layer(q, x, dr["eps_w"][0], dr["eps_b"][0], q._last["pairs"], q._conv())
    assert tuple(oq.shape) == (7, 9, 5, 5) and len(torch.unique(oq)) > 16
    assert torch.equal(q._last["out_q"].cpu(), oq) and torch.equal(out.cpu(), want)
