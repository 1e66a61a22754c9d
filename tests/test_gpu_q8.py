"""GPU: the INT8 quantised layers on the fused int8 MFMA forward (csrc/bt_q8.hip) against the model (tests/_q8_model.py, itself held
to torch's CPU quantised operators by test_q8_model_host.py) and the reference's recorded outputs (tests/golden/q8_*.npz). Integer
accumulation has no order: EVERY comparison is torch.equal on the u8 image (and on the fp32 output it dequantises to)."""
import functools
import math
import zlib

import pytest
import torch

import _guard as G
import _q8_cases as QC
import _q8_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"

C3 = lambda s, p, d: dict(stride=(s, s), padding=(p, p), dilation=(d, d), groups=1)
# name -> (weight shape, x shape, conv or None, padded geometry)
GEOMS = {
    "conv_c5x7k3p1_9x9": ((7, 5, 3, 3), (2, 5, 9, 9), C3(1, 1, 1), True),
    "conv_c19x33k3s2p1": ((33, 19, 3, 3), (2, 19, 11, 10), C3(2, 1, 1), True),
    "conv_c6x5k3d2p2": ((5, 6, 3, 3), (2, 6, 10, 10), C3(1, 2, 2), True),
    "conv_c40x9k1": ((9, 40, 1, 1), (3, 40, 7, 7), C3(1, 0, 1), False),
    "conv_c512x8k3p1_2x2": ((8, 512, 3, 3), (2, 512, 2, 2), C3(1, 1, 1), True),
    "conv_c20x6k3p1_1x1": ((6, 20, 3, 3), (70, 20, 1, 1), C3(1, 1, 1), True),      # eight of nine taps read padding only: pruned when z_in = 128
    "conv_c9x70k3p1": ((70, 9, 3, 3), (2, 9, 6, 6), C3(1, 1, 1), True),      # two output-channel tiles: bias, row sum and draw index for co >= 64
    "linear_70x9_b5": ((9, 70), (5, 70), None, False),
    "linear_784x10": ((10, 784), (130, 784), None, False),      # more than one pixel tile
}
S_MU, S_SIGMA = QC.GPU_S_MU, QC.GPU_S_SIGMA


@functools.lru_cache(maxsize=None)
def _case(name, z_in, bias="full", S=1, big=False):
    """Random int8 images, an input, S draws and the model's answer per sample (computed once, on the CPU, and shared)."""
    wshape, xshape, conv, _ = GEOMS[name]
    g = torch.Generator().manual_seed(zlib.crc32(repr((name, z_in, bias, S)).encode()))
    q_mu = torch.randint(-128, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
    q_sigma = torch.randint(0, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
    K = math.prod(wshape[1:])
    x = torch.randn(xshape, generator=g) * 1.5
    s_in, s_out, z_out = QC.GPU_S_IN, 0.02 * math.sqrt(K), 121
    if big:      # biased data: every product has one sign per output row, |acc| passes 2^24
        q_mu = torch.randint(100, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
        q_mu[wshape[0] // 2:] = -q_mu[wshape[0] // 2:]
        q_mu = (q_mu.float() * (torch.arange(wshape[0]).view(-1, 1, 1, 1) % 4 + 1) / 4).round().to(torch.int8)      # four magnitudes of output row
        q_sigma = torch.randint(0, 8, wshape, generator=g, dtype=torch.int32).to(torch.int8)
        x = (torch.rand(xshape, generator=g) * 3.0 + 8.0) * (torch.rand((xshape[0], 1) + xshape[2:], generator=g) * 0.6 + 0.4)
        s_out = 50.0
    pairs = QC.GPU_PAIRS3 + [(s_in, z_in), (s_out, z_out)]
    Co = wshape[0]
    mu_b = torch.randn(Co, generator=g) * (3.0 * s_out) if bias != "none" else None
    sigma_b = torch.rand(Co, generator=g) * (2.0 * s_out) if bias == "full" else None
    eps_w = torch.randn((S,) + wshape, generator=g)
    eps_b = torch.randn((S, Co), generator=g) if bias == "full" else None
    ref = [M.forward(x, q_mu, q_sigma, S_MU, S_SIGMA, pairs, eps_w[s], mu_b, sigma_b, None if eps_b is None else eps_b[s], conv) for s in range(S)]
    oq = torch.cat([r[0] for r in ref], 0)
    out = torch.cat([r[1] for r in ref], 0)
    return dict(q_mu=q_mu, q_sigma=q_sigma, x=x, pairs=pairs, mu_b=mu_b, sigma_b=sigma_b, eps_w=eps_w, eps_b=eps_b, conv=conv, wshape=wshape, oq=oq, out=out, S=S)


def _dev(t):
    return None if t is None else t.to(DEV)


def _launch(c, eps=True, **kw):
    from bayesian_torch_amd import functional as F
    packs = F.q8_pack(_dev(c["q_mu"]), _dev(c["q_sigma"]))
    return F.q8_forward(_dev(c["x"]), packs, c["wshape"], S_MU, S_SIGMA, c["pairs"], _dev(c["mu_b"]), _dev(c["sigma_b"]), conv=c["conv"], S=c["S"],
                        eps_w=_dev(c["eps_w"]) if eps else None, eps_b=_dev(c["eps_b"]) if eps else None, want_q=True, **kw)


def _same(out, out_q, c, what):
    torch.cuda.synchronize()
    bad = int((out_q.cpu() != c["oq"]).sum())
    print(f"{what}: {c['oq'].numel()} outputs, {len(torch.unique(c['oq']))} distinct levels, {bad} differ")
    assert torch.equal(out_q.cpu(), c["oq"]), (what, bad)
    assert torch.equal(out.cpu(), c["out"]), what


# ---------------------------------------------------------------------------- 1. injected draws against the model
@pytest.mark.parametrize("name,z_in", [(n, z) for n, v in GEOMS.items() for z in ((128, 0, 57) if v[3] else (128,)) if n != "conv_c512x8k3p1_2x2"])
def test_injected_draw_equals_model(name, z_in):
    from bayesian_torch_amd import _lib
    c = _case(name, z_in)
    out, out_q = _launch(c)
    assert _lib.lib().bt_last_kernel_name().decode() == "q8_fwd<i8 32x32x32,64x128,eps injected>"
    assert len(torch.unique(c["oq"])) > 16       # the case is not saturated away
    _same(out, out_q, c, f"{name} z_in={z_in}")


@pytest.mark.parametrize("z_in", [128, 0, 57])
def test_accumulator_above_2_24(z_in):
    c = _case("conv_c512x8k3p1_2x2", z_in, big=True)
    w = M.sampled_weight(c["q_mu"], c["q_sigma"], c["eps_w"][0], S_MU, S_SIGMA, *(p[0] for p in QC.GPU_PAIRS3))
    acc = M.int_conv(M.quant_in(c["x"], *c["pairs"][3]), z_in, w, c["conv"])
    assert int(acc.abs().max()) > 2 ** 24 and len(torch.unique(c["oq"])) > 8
    out, out_q = _launch(c)
    _same(out, out_q, c, f"|acc| up to {int(acc.abs().max())}, z_in={z_in}")


@pytest.mark.parametrize("bias", ["full", "none", "mu_only"])
@pytest.mark.parametrize("name", ["conv_c5x7k3p1_9x9", "linear_70x9_b5"])
def test_three_samples_and_bias_forms(name, bias):
    """S = 3 at sample0 = 5 (injected draws do not depend on sample0), bias present / absent / sigma_b None."""
    c = _case(name, 57 if name.startswith("conv") else 128, bias=bias, S=3)
    out, out_q = _launch(c, sample0=5)
    _same(out, out_q, c, f"{name} bias={bias} S=3")


# ---------------------------------------------------------------------------- 2. the reference's recorded outputs, through the layers
@pytest.mark.parametrize("tag", QC.EXPECTED_GOLDENS)
def test_goldens_reproduce_byte_for_byte(tag):
    g = QC.load(tag)
    q = QC.from_golden(tag, g).to(DEV)       # the recorded images, scales and bias tensors: what is held here is the forward
    q.want_q = True
    q.inject_draw = dict(eps_w=g["eps_w"][None].to(DEV), eps_b=g["eps_b"][None].to(DEV) if "eps_b" in g else None)
    with torch.no_grad():
        out, kl = q(g["x"].to(DEV))
    torch.cuda.synchronize()
    assert kl == 0 and q._last["kernel"].startswith("q8_fwd<") and q._last["pairs"] == QC.pairs_of(g)
    bad = int((q._last["out_q"].cpu() != g["out_q"]).sum())
    print(f"{tag}: {g['out_q'].numel()} outputs, {bad} differ from the reference")
    assert torch.equal(q._last["out_q"].cpu(), g["out_q"]) and torch.equal(out.cpu(), g["out"])
    d = q.materialize_last_draw()
    assert torch.equal(d["eps_w"].cpu(), g["eps_w"][None])


# ---------------------------------------------------------------------------- 3. on-chip draws
@pytest.mark.parametrize("name", ["conv_c5x7k3p1_9x9", "conv_c19x33k3s2p1", "conv_c40x9k1", "conv_c9x70k3p1", "linear_70x9_b5"])
def test_on_chip_draws_equal_the_filled_streams(name):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    c = dict(_case(name, 57, S=3))
    coords = dict(seed=0x1234ABCD5678, call=9, layer_id=4, sample0=5)
    out, out_q = _launch(c, eps=False, **coords)
    assert _lib.lib().bt_last_kernel_name().decode() == "q8_fwd<i8 32x32x32,64x128,eps on chip>"
    eps_w = F.rng_fill_normal(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], 0, 3, c["wshape"], DEV)
    eps_b = F.rng_fill_normal(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], 1, 3, (c["wshape"][0],), DEV)
    c["eps_w"], c["eps_b"] = eps_w, eps_b
    out2, out_q2 = _launch(c)
    torch.cuda.synchronize()
    assert torch.equal(out_q, out_q2) and torch.equal(out, out2)
    ref = [M.forward(c["x"], c["q_mu"], c["q_sigma"], S_MU, S_SIGMA, c["pairs"], eps_w[s].cpu(), c["mu_b"], c["sigma_b"], eps_b[s].cpu(), c["conv"])[0] for s in range(3)]
    assert torch.equal(out_q.cpu(), torch.cat(ref, 0))
    per = out_q.shape[0] // 3
    assert not torch.equal(out_q[:per], out_q[per:2 * per])      # the samples differ


def test_sample_split_does_not_change_the_result():
    c = dict(_case("conv_c19x33k3s2p1", 0, S=4))
    coords = dict(seed=77, call=3, layer_id=2)
    whole, whole_q = _launch(c, eps=False, sample0=0, **coords)
    c["S"] = 2
    a, a_q = _launch(c, eps=False, sample0=0, **coords)
    b, b_q = _launch(c, eps=False, sample0=2, **coords)
    torch.cuda.synchronize()
    assert torch.equal(whole_q, torch.cat([a_q, b_q], 0)) and torch.equal(whole, torch.cat([a, b], 0))


# ---------------------------------------------------------------------------- 4. a converted model under mc_forward and McGraph
def _two_layer_model():
    return QC.two_layer_model().to(DEV)


def _model_chain(net, x, S):
    """The per-layer model applied sample by sample with the draws the layers' last forward made -> u8-exact fp32 logits [S, B, 4]."""
    d0, d3 = net[0].materialize_last_draw(), net[3].materialize_last_draw()
    outs = []
    for s in range(S):
        eb = lambda d: None if d["eps_b"] is None else d["eps_b"][s]
        h = QC.model_of_layer(net[0], x, d0["eps_w"][s], eb(d0), net[0]._last["pairs"], net[0]._conv())[1]
        h = torch.flatten(torch.relu(h), 1)
        outs.append(QC.model_of_layer(net[3], h, d3["eps_w"][s], eb(d3), net[3]._last["pairs"], None)[1])
    return torch.stack(outs)


def test_mc_forward_and_graph_replay_agree_with_the_model():
    from bayesian_torch_amd import mc, rng
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    net = _two_layer_model()
    x = torch.randn(3, 3, 5, 5, generator=torch.Generator().manual_seed(4)) * 1.5
    S = 3
    rng.manual_seed(99)
    rng.set_call(40)
    logits, kl = mc.mc_forward(net, x.to(DEV), S)
    torch.cuda.synchronize()
    assert kl is None and float(get_kl_loss(net)) == 0.0
    assert tuple(logits.shape) == (S, 3, 4) and net[0]._last["S"] == S and net[3]._last["shared_x"] is False
    want = _model_chain(net, x, S)
    assert len(torch.unique(want)) > 8 and torch.equal(logits.cpu(), want)
    graph = mc.McGraph(net, x.to(DEV), S, with_kl=False, epilogue=False)
    rng.set_call(40)                       # a replay draws what an eager mc_forward at this position draws
    got, _, _ = graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)
    got2 = graph.replay()[0].clone()       # the next replay: the next calls, other draws
    rng.set_call(42)
    again = mc.mc_forward(net, x.to(DEV), S)[0]
    torch.cuda.synchronize()
    assert torch.equal(got2, again) and not torch.equal(got2.cpu(), want)


# ---------------------------------------------------------------------------- 5. guard bands
@pytest.mark.parametrize("name,off", [("conv_c19x33k3s2p1", 1), ("linear_70x9_b5", 3), ("conv_c5x7k3p1_9x9", 2)])
def test_guard_bands_around_out_and_out_q(name, off):
    c = _case(name, 57, S=3)
    with G.guarded_allocations(lambda shape, dtype: 0 if dtype == torch.int8 else off) as log:      # (the packs must be 16-byte aligned)
        out, out_q = _launch(c)
    torch.cuda.synchronize()
    assert {g.view.dtype for g in log} == {torch.int8, torch.float32, torch.uint8}      # the packs, out, out_q
    G.check_all(log)
    assert torch.equal(out_q.cpu(), c["oq"]) and torch.equal(out.cpu(), c["out"])


# ---------------------------------------------------------------------------- 6. the i8 fragment map
def test_fragment_map_with_asymmetric_integers():
    """Exact integer data that tells every (output row, k, pixel) apart: sigma = 0 and s_add = s_mu make w = q_mu; s_in = 1 makes
    xq - z_in = x; s_in * s_add / s_out = 1 makes oq = acc + z_out. One-hot inputs read out single weights (a wrong k or row of either
    operand's lane map moves a value); a dense input checks the sum over both K chunks of both stages."""
    from bayesian_torch_amd import functional as F
    Out, In, B = 70, 112, 140                     # two row tiles, seven units (a second stage with a missing unit), two pixel tiles
    co, k = torch.arange(Out).view(-1, 1), torch.arange(In).view(1, -1)
    q_mu = ((3 * co + 5 * k + (co * k) % 7) % 13 - 6).to(torch.int8)
    s = 2.0 ** -6
    pairs = [(6 / 255, 0), (1e-4, 0), (s, 0), (1.0, 128), (s, 128)]
    b = torch.arange(B)
    onehot = torch.zeros(B, In)
    onehot[b, (b * 5) % In] = (1 + b % 7).float() * torch.where(b % 3 == 0, -1.0, 1.0)
    dense = ((b.view(-1, 1) + 2 * k) % 5 - 2).float()
    packs = F.q8_pack(q_mu.to(DEV), torch.zeros_like(q_mu).to(DEV))
    for what, x in (("one-hot", onehot), ("dense", dense)):
        acc = x.to(torch.int64) @ q_mu.to(torch.int64).t()
        assert int((acc != 0).sum()) > B * Out // 2
        acc = torch.clamp(acc, -128, 127)                        # the u8 range around z_out = 128
        assert int(((acc == -128) | (acc == 127)).sum()) < B * Out // 8
        out, out_q = F.q8_forward(x.to(DEV), packs, (Out, In), s, 1e-3, pairs, eps_w=torch.randn(1, Out, In, device=DEV), want_q=True)
        torch.cuda.synchronize()
        assert torch.equal(out_q.cpu().to(torch.int64) - 128, acc), what
        assert torch.equal(out.cpu(), acc.float() * s), what
