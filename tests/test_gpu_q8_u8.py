"""GPU: u8 activations between the INT8 layers (quantization/qact.py; csrc/bt_q8_act.hip and the u8-source / blocked-destination
instantiations of csrc/bt_q8_common.h's walk) against the model (tests/_q8_u8_model.py, itself held to torch's CPU quantised operators
by test_q8_u8_model_host.py). Integer accumulation has no order: EVERY comparison is torch.equal -- on the whole blocked image, so the
bytes of the padding channels (the zero point) are held too."""
import functools
import math
import zlib

import pytest
import torch
import torch.nn as nn

import _guard as G
import _q8_cases as QC
import _q8_flip_cases as FC
import _q8_flip_model as FM
import _q8_model as M
import _q8_u8_model as U

pytestmark = pytest.mark.gpu
DEV = "cuda"

C3 = lambda s, p, d=1: dict(stride=(s, s), padding=(p, p), dilation=(d, d), groups=1)
# name -> (weight shape, x shape, conv or None)
GEOMS = {
    "conv_c3x70k3p1_7x6": ((70, 3, 3, 3), (2, 3, 7, 6), C3(1, 1)),        # a partial input block; two channel tiles, 10 padding channels of the blocked output
    "conv_c20x9k3s2p1_9x8": ((9, 20, 3, 3), (2, 20, 9, 8), C3(2, 1)),      # two input blocks, the second partial; stride 2
    "conv_c32x6k3p1_1x1": ((6, 32, 3, 3), (12, 32, 1, 1), C3(1, 1)),       # two whole input blocks; eight of nine taps read padding only (pruned at z = 128)
    "conv_c20x17k1_13x10": ((17, 20, 1, 1), (1, 20, 13, 10), C3(1, 0)),    # 130 output pixels: two pixel tiles, the second nearly empty; two output blocks
    "linear_20x9_b5": ((9, 20), (5, 20), None),
}
S_MU, S_SIGMA = QC.GPU_S_MU, QC.GPU_S_SIGMA
OWN_IN = (0.5, 9)      # the layer's own `in` pair: a quint8 input is read with the CARRIER's pair, this one must not matter


def _dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(chain, name, z_in, bias="full", S=1, kind="dict"):
    """Random int8 images, S quint8 inputs (xq[0]: the shared one) at the carrier's pair, S draws and the model's u8 answer per sample
    for shared and per-sample x (computed once, on the CPU, and shared)."""
    wshape, xshape, conv = GEOMS[name]
    g = torch.Generator().manual_seed(zlib.crc32(repr((chain, name, z_in, bias, S, kind)).encode()))
    q_mu = torch.randint(-128, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
    q_sigma = torch.randint(0, 128, wshape, generator=g, dtype=torch.int32).to(torch.int8)
    K = math.prod(wshape[1:])
    Co = wshape[0]
    eps_w = torch.randn((S,) + wshape, generator=g)
    eps_b = torch.randn((S, Co), generator=g) if bias == "full" else None
    c = dict(chain=chain, name=name, q_mu=q_mu, q_sigma=q_sigma, eps_w=eps_w, eps_b=eps_b, conv=conv, wshape=wshape, xshape=xshape, S=S)
    if chain == "reparam":
        pair = (QC.GPU_S_IN, z_in)
        s_out = 0.02 * math.sqrt(K)
        pairs = QC.GPU_PAIRS3 + [OWN_IN, (s_out, 121)]
        s_b, s_sb, i_in = 3.0 * s_out, 2.0 * s_out, 3
    else:
        pairs = FC.pairs_of(kind, K)
        pair = (pairs[FM.IN][0], z_in)
        pairs[FM.IN] = OWN_IN
        s_b, s_sb, i_in = 3.0 * pairs[FM.MEAN][0], 2.0 * pairs[FM.PERT][0], FM.IN
    xq = M.quant_in(torch.randn((S,) + xshape, generator=g) * 1.5, *pair)
    mu_b = torch.randn(Co, generator=g) * s_b if bias != "none" else None
    sigma_b = torch.rand(Co, generator=g) * s_sb if bias == "full" else None
    c.update(pair=pair, pairs=pairs, launch_pairs=U.with_in(pairs, pair, i_in), xq=xq, mu_b=mu_b, sigma_b=sigma_b)
    eb = lambda s: None if eps_b is None else eps_b[s]
    if chain == "reparam":
        one = lambda s, xs: U.reparam_from_u8(xq[xs], pair, q_mu, q_sigma, S_MU, S_SIGMA, pairs, eps_w[s], mu_b, sigma_b, eb(s), conv)
    else:
        oshape = tuple(U.reparam_from_u8(xq[0], pair, q_mu, q_sigma, S_MU, S_SIGMA, QC.GPU_PAIRS3 + [OWN_IN, (1.0, 0)], eps_w[0], None, None, None, conv).shape)
        c["sign_in"] = torch.randint(0, 2, (S,) + xshape, generator=g).float() * 2 - 1
        c["sign_out"] = torch.randint(0, 2, (S,) + oshape, generator=g).float() * 2 - 1
        one = lambda s, xs: U.flip_from_u8(xq[xs], pair, q_mu, q_sigma, S_MU, S_SIGMA, pairs, eps_w[s], c["sign_in"][s], c["sign_out"][s], mu_b, sigma_b, eb(s), conv)
    c["one"] = one
    c["oq_shared"] = torch.cat([one(s, 0) for s in range(S)], 0)
    return c


def _out_pair(c):
    return c["pairs"][4 if c["chain"] == "reparam" else FM.OUT]


def _launch(c, shared=True, draws=True, dest="both", src="u8", x=None, **kw):
    """The functional forward on the blocked image of the case's levels (src 'u8') or on their dequantised fp32 values (src 'f32': the
    kernel quantises them back to the same levels in its producer)."""
    from bayesian_torch_amd import functional as F
    packs = F.q8_pack(_dev(c["q_mu"]), _dev(c["q_sigma"]))
    lv = c["xq"][0] if shared else c["xq"].reshape((-1,) + tuple(c["xshape"][1:]))
    if x is None:
        x = _dev(U.block(lv, c["pair"][1])) if src == "u8" else _dev(U.deq(lv, c["pair"]))
    keys = ("eps_w", "eps_b") + (("sign_in", "sign_out") if c["chain"] == "flip" else ())
    d = {k: _dev(c[k]) for k in keys} if draws else {}
    fn = F.q8_forward if c["chain"] == "reparam" else F.q8_flip_forward
    return fn(x, packs, c["wshape"], S_MU, S_SIGMA, c["launch_pairs"], _dev(c["mu_b"]), _dev(c["sigma_b"]), conv=c["conv"], S=c["S"], shared_x=shared,
              x_shape=tuple(lv.shape) if src == "u8" else None, dest=dest, **d, **kw)


def _same(out, out_b, want_q, c, what):
    """The whole blocked image (padding channels: z_out) and, where asked for, the fp32 output it dequantises to."""
    torch.cuda.synchronize()
    po = _out_pair(c)
    want_b = U.block(want_q, po[1])
    assert tuple(out_b.shape) == tuple(want_b.shape) and out_b.dtype == torch.uint8, what
    bad = int((out_b.cpu() != want_b).sum())
    print(f"{what}: {want_q.numel()} outputs, {len(torch.unique(want_q))} distinct levels, {want_b.numel() - want_q.numel()} padding bytes, {bad} bytes differ")
    assert torch.equal(out_b.cpu(), want_b), (what, bad)
    if out is not None:
        assert torch.equal(out.cpu(), U.deq(want_q, po)), what


# ---------------------------------------------------------------------------- 1. the layers' launches against the model
REPARAM_CASES = [(n, z) for n, v in GEOMS.items() for z in ((128, 0, 57) if v[2] is not None and v[2]["padding"] != (0, 0) else (128,))]


@pytest.mark.parametrize("name,z_in", REPARAM_CASES)
def test_u8_source_and_blocked_destination_equal_model(name, z_in):
    from bayesian_torch_amd import _lib
    c = _case("reparam", name, z_in)
    assert len(torch.unique(c["oq_shared"])) > 16       # the case is not saturated away
    out, out_b = _launch(c)
    assert _lib.lib().bt_last_kernel_name().decode() == "q8_fwd<i8 32x32x32,64x128,eps injected,x u8 blocked,out u8 blocked>"
    _same(out, out_b, c["oq_shared"], c, f"{name} z_in={z_in} u8 -> both")
    out, out_b = _launch(c, dest="u8")                  # nothing fp32-sized is written
    assert out is None
    _same(None, out_b, c["oq_shared"], c, f"{name} z_in={z_in} u8 -> u8")
    out, none = _launch(c, dest="f32")                  # what a Linear layer does: the fp32 result alone
    assert none is None and _lib.lib().bt_last_kernel_name().decode() == "q8_fwd<i8 32x32x32,64x128,eps injected,x u8 blocked>"
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), U.deq(c["oq_shared"], _out_pair(c)))


@pytest.mark.parametrize("name,z_in", [("conv_c3x70k3p1_7x6", 57), ("conv_c20x17k1_13x10", 128), ("linear_20x9_b5", 0)])
def test_fp32_source_and_blocked_destination_equal_model(name, z_in):
    """The first layer of a u8 network: fp32 in (quantised in the producer, as today), the blocked image out."""
    from bayesian_torch_amd import _lib
    c = _case("reparam", name, z_in)
    out, out_b = _launch(c, src="f32", dest="u8")
    assert out is None and _lib.lib().bt_last_kernel_name().decode() == "q8_fwd<i8 32x32x32,64x128,eps injected,out u8 blocked>"
    _same(None, out_b, c["oq_shared"], c, f"{name} z_in={z_in} f32 -> u8")
    out, out_b = _launch(c, src="f32", dest="both")
    _same(out, out_b, c["oq_shared"], c, f"{name} z_in={z_in} f32 -> both")


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("bias", ["full", "none", "mu_only"])
@pytest.mark.parametrize("name", ["conv_c20x9k3s2p1_9x8", "linear_20x9_b5"])
def test_three_samples_and_bias_forms(name, bias, shared):
    """S = 3 at sample0 = 5 (injected draws do not depend on it), shared and per-sample x; bias present / absent / sigma_b None."""
    c = _case("reparam", name, 57 if name.startswith("conv") else 128, bias=bias, S=3)
    want = c["oq_shared"] if shared else torch.cat([c["one"](s, s) for s in range(3)], 0)
    out, out_b = _launch(c, shared=shared, sample0=5)
    _same(out, out_b, want, c, f"{name} bias={bias} S=3 shared={shared}")


@pytest.mark.parametrize("name,z_in,kind,S,shared", [("conv_c3x70k3p1_7x6", 57, "dict", 1, True), ("conv_c20x9k3s2p1_9x8", 0, "dict", 3, False),
                                                     ("conv_c32x6k3p1_1x1", 128, "default", 2, True), ("linear_20x9_b5", 120, "dict", 3, False)])
def test_flipout_chain_equals_model(name, z_in, kind, S, shared):
    """The sign of an input element is indexed by its offset in the LOGICAL [B][Ci][H][W], whatever layout the bytes come in."""
    from bayesian_torch_amd import _lib
    c = _case("flip", name, z_in, S=S, kind=kind)
    want = c["oq_shared"] if shared else torch.cat([c["one"](s, s) for s in range(S)], 0)
    assert len(torch.unique(want)) > 8
    out, out_b = _launch(c, shared=shared, sample0=5)
    assert _lib.lib().bt_last_kernel_name().decode() == "q8_flip_fwd<i8 32x32x32,64x128,draws injected,x u8 blocked,out u8 blocked>"
    _same(out, out_b, want, c, f"flip {name} z_in={z_in} {kind} S={S} shared={shared}")
    if S == 1:
        out, out_b = _launch(c, src="f32", dest="u8")
        _same(None, out_b, want, c, f"flip {name} f32 -> u8")
        out, none = _launch(c, dest="f32")
        torch.cuda.synchronize()
        assert none is None and torch.equal(out.cpu(), U.deq(want, _out_pair(c)))


@pytest.mark.parametrize("chain,name", [("reparam", "conv_c20x9k3s2p1_9x8"), ("flip", "conv_c3x70k3p1_7x6")])
def test_on_chip_draws_equal_the_filled_streams(chain, name):
    from bayesian_torch_amd import functional as F
    c = dict(_case(chain, name, 57, S=3))
    coords = dict(seed=0x1234ABCD5678, call=9, layer_id=4, sample0=5)
    out, out_b = _launch(c, draws=False, **coords)
    fill = lambda fn, tensor, shape: fn(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], tensor, 3, tuple(shape), DEV)
    c["eps_w"], c["eps_b"] = fill(F.rng_fill_normal, 0, c["wshape"]), fill(F.rng_fill_normal, 1, (c["wshape"][0],))
    if chain == "flip":
        c["sign_in"], c["sign_out"] = fill(F.rng_fill_sign, 2, c["xshape"]), fill(F.rng_fill_sign, 3, c["sign_out"].shape[1:])
    out2, out_b2 = _launch(c)
    torch.cuda.synchronize()
    assert torch.equal(out_b, out_b2) and torch.equal(out, out2)
    per = out_b.shape[0] // 3
    assert not torch.equal(out_b[:per], out_b[per:2 * per])      # the samples differ
    eb = c["eps_b"].cpu()
    if chain == "reparam":
        ref = [U.reparam_from_u8(c["xq"][0], c["pair"], c["q_mu"], c["q_sigma"], S_MU, S_SIGMA, c["pairs"], c["eps_w"][s].cpu(), c["mu_b"], c["sigma_b"], eb[s], c["conv"])
               for s in range(3)]
    else:
        ref = [U.flip_from_u8(c["xq"][0], c["pair"], c["q_mu"], c["q_sigma"], S_MU, S_SIGMA, c["pairs"], c["eps_w"][s].cpu(), c["sign_in"][s].cpu(), c["sign_out"][s].cpu(),
                              c["mu_b"], c["sigma_b"], eb[s], c["conv"]) for s in range(3)]
    _same(out, out_b, torch.cat(ref, 0), c, f"{chain} {name} on chip")


# ---------------------------------------------------------------------------- 2. consistency with the fp32-between-layers path
def _two_convs():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    torch.manual_seed(33)
    net = nn.Sequential(L.Conv2dReparameterization(3, 20, 3, padding=1, bias=True), L.Conv2dReparameterization(20, 7, 3, stride=2, padding=1, bias=False))
    with torch.no_grad():
        net[0].rho_kernel.fill_(-2.0), net[1].rho_kernel.fill_(-2.0)
    net[0].dnn_to_bnn_flag = net[1].dnn_to_bnn_flag = True
    rng.assign_layer_ids(net)
    bnn_to_qbnn(net)
    dicts = [((0.0291, 0), (0.0009, 0), (0.004, 0), (0.04, 120), (0.03, 100)), ((0.0291, 0), (0.0009, 0), (0.004, 0), (0.03, 100), (0.09, 131))]
    for layer, pairs in zip(net, dicts):      # the second layer's `in` pair IS the first's `out` pair
        layer.quant_dict = [dict(scale=sc, zero_point=z) for sc, z in pairs]
    return net.eval().to(DEV)


def test_u8_pipeline_equals_the_fp32_between_layers_pipeline():
    """Requantising (q - z) * s at the same pair returns q: with the second layer's `in` pair equal to the first's `out` pair, the u8
    pipeline's final image is the existing path's, bit for bit -- which ties the new path to code the existing tests hold."""
    from bayesian_torch_amd.quantization import qact
    net = _two_convs()
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 3, 9, 8, generator=g) * 1.5).to(DEV)
    draws = [dict(eps_w=torch.randn((1,) + tuple(l.quantized_mu_weight.shape), generator=g).to(DEV),
                  eps_b=torch.randn(1, 20, generator=g).to(DEV) if l.quantized_sigma_bias is not None else None) for l in net]
    for l, d in zip(net, draws):
        l.inject_draw, l.want_q = d, True
    with torch.no_grad():
        mid = net[0](x)
        want = net[1](mid)
    want_q, mid_q = net[1]._last["out_q"].clone(), net[0]._last["out_q"].clone()
    assert mid.dtype == torch.float32 and net[0]._last["kernel"] == "q8_fwd<i8 32x32x32,64x128,eps injected>"
    net[0].return_quantized = True
    with torch.no_grad():
        qmid = net[0](x)
        qout = net[1](qmid)
    torch.cuda.synchronize()
    assert isinstance(qmid, qact.QActivation) and isinstance(qout, qact.QActivation) and qmid.dtype == torch.quint8
    assert qmid.pair == (0.03, 100) and qout.pair == (0.09, 131) and qmid.shape == (2, 20, 9, 8) and qout.shape == (2, 7, 5, 4)
    assert net[0]._last["kernel"].endswith("eps injected,out u8 blocked>") and net[1]._last["kernel"].endswith("eps injected,x u8 blocked,out u8 blocked>")
    assert net[1]._last["pairs"][3] == (0.03, 100) and net[1]._last["out"] is qout
    assert len(torch.unique(want_q)) > 16
    assert torch.equal(qmid.int_repr(), mid_q) and torch.equal(qout.int_repr(), want_q)
    assert torch.equal(qout.dequantize(), want) and torch.equal(qmid.dequantize(), mid)
    # a carrier at ANOTHER pair replaces the layer's own `in` pair (the reference reads input.q_scale() / q_zero_point())
    other = qact.QActivation(qmid.data, 0.021, 93, qmid.shape)
    with torch.no_grad():
        qo2 = net[1](other)
    d = draws[1]
    ref = QC.model_of_layer(net[1], U.deq(qmid.int_repr().cpu(), (0.021, 93)), d["eps_w"][0], None, U.with_in(net[1]._last["pairs"], (0.021, 93)), net[1]._conv())[0]
    assert net[1]._last["pairs"][3] == (0.021, 93) and torch.equal(qo2.int_repr().cpu(), ref) and not torch.equal(ref, want_q.cpu())


# ---------------------------------------------------------------------------- 3. the element-wise launches against their models
ADD_SETS = {"equal scales": ((0.1, 128), (0.1, 128), (0.1, 0)),
            "qresnet default": ((0.05, 100), (0.073, 57), (0.073, 0)),
            "odd output zero point": ((0.031, 0), (0.02, 255), (0.045, 121)),
            "dyadic ties": ((2.0 ** -4, 128), (2.0 ** -5, 64), (2.0 ** -4, 3)),
            "narrow output": ((0.21, 7), (0.4, 250), (0.05, 31))}


def _lv(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(torch.uint8)


def _carrier(lv, pair):
    from bayesian_torch_amd.quantization import qact
    return qact.from_int_repr(lv.to(DEV), *pair)


def _blocked_equal(q, want_lv, pair):
    torch.cuda.synchronize()
    assert q.pair == (float(pair[0]), int(pair[1])) and tuple(q.shape) == tuple(want_lv.shape)
    return torch.equal(q.data.cpu(), U.block(want_lv, pair[1]))


@pytest.mark.parametrize("name", sorted(ADD_SETS))
def test_add_and_add_relu_over_all_u8_pairs(name):
    """One 256 x 256 plane per pair set: every pair of levels, as [1, 1, 256, 256] (15 padding channels, which must read z_out)."""
    from bayesian_torch_amd.quantization import qact
    pa, pb, po = ADD_SETS[name]
    v = torch.arange(256, dtype=torch.int32)
    a, b = v.repeat_interleave(256).to(torch.uint8).view(1, 1, 256, 256), v.repeat(256).to(torch.uint8).view(1, 1, 256, 256)
    qa, qb = _carrier(a, pa), _carrier(b, pb)
    assert _blocked_equal(qact.add(qa, qb, *po), U.add(a, pa, b, pb, po), po)
    assert _blocked_equal(qact.add_relu(qa, qb, *po), U.add_relu(a, pa, b, pb, po), po)
    if name == "qresnet default":
        r = qact.add_relu(qa, qb)
        assert r.pair == (0.073, 0) and _blocked_equal(r, U.add_relu(a, pa, b, pb, po), po)
        assert _blocked_equal(qact.QFunctional().add(qa, qb), U.add(a, pa, b, pb, po), po)


def test_add_on_uneven_shapes():
    from bayesian_torch_amd.quantization import qact
    pa, pb, po = ADD_SETS["odd output zero point"]
    for shape in ((3, 20, 5, 3), (2, 70, 1, 1), (5, 20)):
        a, b = _lv(shape, 1), _lv(shape, 2)
        assert _blocked_equal(qact.add_relu(_carrier(a, pa), _carrier(b, pb), *po), U.add_relu(a, pa, b, pb, po), po)


@pytest.mark.parametrize("z", [0, 100, 255])
def test_relu_quantize_dequantize(z):
    from bayesian_torch_amd.quantization import qact
    lv = torch.arange(256, dtype=torch.int32).to(torch.uint8).repeat(3 * 20 * 2).view(3, 20, 16, 32)
    lv = lv.roll(z, 3)
    q = _carrier(lv, (0.07, z))
    r = qact.relu(q)
    assert r is not q and _blocked_equal(r, U.relu(lv, z), (0.07, z)) and torch.equal(q.int_repr().cpu(), lv)
    r2 = nn.ReLU(inplace=True)(q)                       # in place: the carrier's own bytes
    assert r2 is q and _blocked_equal(q, U.relu(lv, z), (0.07, z))
    x = torch.randn(3, 20, 7, 5, generator=torch.Generator().manual_seed(z)) * 6.0
    x[0, 0, 0, :4] = torch.tensor([0.035, 0.105, -0.035, 1e9])      # ties at s = 0.07, and a value far past the clamp
    qx = qact.quantize_per_tensor(x.to(DEV), 0.07, z)
    assert _blocked_equal(qx, M.quant_in(x, 0.07, z), (0.07, z))
    assert torch.equal(qx.dequantize().cpu(), U.deq(M.quant_in(x, 0.07, z), (0.07, z)))
    x2 = torch.randn(5, 20, generator=torch.Generator().manual_seed(z + 1))
    q2 = qact.QuantStub(0.011, z)(x2.to(DEV))
    assert _blocked_equal(q2, M.quant_in(x2, 0.011, z), (0.011, z)) and torch.equal(qact.DeQuantStub()(q2).cpu(), U.deq(M.quant_in(x2, 0.011, z), (0.011, z)))


@pytest.mark.parametrize("shape,kernel,stride,padding", [((2, 20, 9, 7), 3, 2, 1), ((2, 3, 4, 4), 2, 2, 0)])
def test_max_pool2d(shape, kernel, stride, padding):
    lv = _lv(shape, 11)
    lv[0, 0] = 0          # a plane of the lowest level: padding must not win
    for z in (0, 131):
        got = nn.MaxPool2d(kernel, stride, padding)(_carrier(lv, (0.05, z)))
        assert _blocked_equal(got, U.max_pool2d(lv, kernel, stride, padding), (0.05, z))


@pytest.mark.parametrize("z", [0, 1, 57, 128, 255])
def test_global_average_pool_and_flatten(z):
    for h, w in ((2, 2), (4, 4), (3, 5), (7, 7)):
        cases = [_lv((3, 20, h, w), 100 * h + w)]
        if (h * w) % 2 == 0:
            cases.append(U.tie_planes(h, w, z))           # sum - z * n an exact tie of the mean
        for lv in cases:
            q = _carrier(lv, (0.043, z))
            got = nn.AdaptiveAvgPool2d(1)(q)
            assert _blocked_equal(got, U.avg_pool(lv, z), (0.043, z)), (h, w)
            assert _blocked_equal(nn.AvgPool2d((h, w))(q), U.avg_pool(lv, z), (0.043, z))
            flat = torch.flatten(got, 1)                # a 1 x 1 map: free
            assert flat.data.data_ptr() == got.data.data_ptr() and _blocked_equal(flat, U.avg_pool(lv, z).flatten(1), (0.043, z))
            assert _blocked_equal(nn.Flatten()(q), lv.flatten(1), (0.043, z))      # a larger map: reordered to the NCHW feature order


# ---------------------------------------------------------------------------- 4. a converted ResNet under mc_forward and McGraph
PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization", "moped_enable": False,
         "moped_delta": 0.5}


def _u8_resnet():
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(0)
    net = H.resnet18(10, 8)
    dnn_to_bnn(net, PRIOR)
    with torch.no_grad():
        H.fill_bayes_params(net, 1)
    net = net.to(DEV).eval()
    rng.assign_layer_ids(net)
    bnn_to_qbnn(net, fuse_conv_bn=True)
    return H.u8_inference(net)


def _resnet_model(net, x, S):
    """The per-layer model applied sample by sample with the draws (and pairs) of the layers' last forward -> fp32 logits [S, B, 10]."""
    outs = []
    draws = {id(m): m.materialize_last_draw() for m in net.modules() if hasattr(m, "materialize_last_draw")}

    def layer(m, lv, pair, s):
        d = draws[id(m)]
        eb = None if d["eps_b"] is None else d["eps_b"][s]
        xin = lv if pair is None else U.deq(lv, pair)
        assert pair is None or m._last["pairs"][3] == pair
        oq, out = QC.model_of_layer(m, xin, d["eps_w"][s], eb, m._last["pairs"], m._conv())
        return oq, m._last["pairs"][4], out

    for s in range(S):
        lv, pr, _ = layer(net.conv1, x, None, s)
        lv = U.max_pool2d(U.relu(lv, pr[1]), 3, 2, 1)
        for stage in (net.layer1, net.layer2, net.layer3, net.layer4):
            for blk in stage:
                skip, ps = (lv, pr) if blk.downsample is None else layer(blk.downsample[0], lv, pr, s)[:2]
                y, py, _ = layer(blk.conv1, lv, pr, s)
                y, py, _ = layer(blk.conv2, U.relu(y, py[1]), py, s)
                pr = (max(py[0], ps[0]), 0)
                lv = U.add_relu(y, py, skip, ps, pr)
        assert lv.shape[-2:] == (1, 1)
        outs.append(layer(net.fc, lv.flatten(1), pr, s)[2])
    return torch.stack(outs)


def test_resnet_u8_inference_under_mc_forward_and_graph_replay():
    from bayesian_torch_amd import mc, rng
    from bayesian_torch_amd.quantization import qact
    net = _u8_resnet()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    S = 2
    seen = []
    hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: seen.append((n, type(inp[0]), type(out[0] if isinstance(out, tuple) else out))))
             for n, m in net.named_modules() if n and not list(m.children())]
    rng.manual_seed(99)
    rng.set_call(40)
    logits, _ = mc.mc_forward(net, x.to(DEV), S, with_kl=False)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    # no fp32 activation between the stem and fc: every module behind conv1 takes a carrier, every one before fc returns one
    assert seen[0] == ("conv1", torch.Tensor, qact.QActivation) and seen[-1] == ("fc", qact.QActivation, torch.Tensor) and len(seen) > 40
    assert all(i is qact.QActivation and o is qact.QActivation for _, i, o in seen[1:-1]), [e for e in seen[1:-1] if e[1] is not qact.QActivation or e[2] is not qact.QActivation]
    convs = [m for n, m in net.named_modules() if hasattr(m, "_last") and n != "fc"]
    assert len(convs) == 20 and all(isinstance(m._last["out"], qact.QActivation) and m._last["out_q"].dtype == torch.uint8 for m in convs)
    assert "out" not in net.fc._last and net.fc._last["kernel"].endswith("x u8 blocked>") and tuple(logits.shape) == (S, 2, 10)
    assert net.layer1[0].conv1._last["shared_x"] is False and net.conv1._last["shared_x"] is True
    want = _resnet_model(net, x, S)
    assert len(torch.unique(want)) > 8 and torch.equal(logits.cpu(), want)
    graph = mc.McGraph(net, x.to(DEV), S, with_kl=False, epilogue=False)
    rng.set_call(40)                       # a replay draws what an eager mc_forward at this position draws
    got = graph.replay()[0]
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)
    got2 = graph.replay()[0].clone()       # the next replay: the next calls, other draws
    torch.cuda.synchronize()
    assert not torch.equal(got2.cpu(), want)


# ---------------------------------------------------------------------------- 5. guard bands and alignment
@pytest.mark.parametrize("chain,name", [("reparam", "conv_c3x70k3p1_7x6"), ("reparam", "linear_20x9_b5"), ("flip", "conv_c20x9k3s2p1_9x8")])
def test_guard_bands_around_the_blocked_outputs(chain, name):
    c = _case(chain, name, 57, S=3)
    # (the packs and the blocked image must be 16-byte aligned; the fp32 out sits one element off)
    with G.guarded_allocations(lambda shape, dtype: 1 if dtype == torch.float32 else 0) as log:
        out, out_b = _launch(c, sample0=5)
    torch.cuda.synchronize()
    assert {g.view.dtype for g in log} == {torch.int8, torch.float32, torch.uint8}
    G.check_all(log, body=lambda g: g.view.dtype in (torch.float32, torch.uint8))      # every byte of the blocked image is written, padding channels included
    _same(out, out_b, c["oq_shared"], c, f"guarded {chain} {name}")


def test_guard_bands_around_the_element_wise_outputs():
    from bayesian_torch_amd.quantization import qact
    lv, lv2 = _lv((3, 20, 9, 7), 1), _lv((3, 20, 9, 7), 2)
    a, b = _carrier(lv, (0.05, 100)), _carrier(lv2, (0.073, 57))
    x = torch.randn(3, 20, 9, 7, generator=torch.Generator().manual_seed(3)).to(DEV)
    with G.guarded_allocations(lambda shape, dtype: 1 if dtype == torch.float32 else 0) as log:
        r = [qact.add_relu(a, b), qact.relu(a), qact.max_pool2d(a, 3, 2, 1), qact.adaptive_avg_pool2d(a, 1), qact.flatten(a, 1), qact.quantize_per_tensor(x, 0.05, 100)]
        d = qact.dequantize(a)
    torch.cuda.synchronize()
    assert len(log) == 7
    G.check_all(log, body=lambda g: True)
    assert torch.equal(r[0].int_repr().cpu(), U.add_relu(lv, a.pair, lv2, b.pair, (0.073, 0))) and torch.equal(r[4].int_repr().cpu(), lv.flatten(1))
    assert torch.equal(d.cpu(), U.deq(lv, a.pair))


def test_misaligned_blocked_images_are_refused_not_launched():
    """A view of a blocked image 16 ELEMENTS into its buffer is still aligned and runs; one that starts 4 bytes in is refused by the C
    ABI before any launch -- the guard bands around it stay untouched."""
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.quantization import qact
    c = _case("reparam", "conv_c20x9k3s2p1_9x8", 57)
    img = U.block(c["xq"][0], c["pair"][1])
    buf = torch.full((img.numel() + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    for off, ok in ((16, True), (4, False), (8, False)):
        view = buf[off:off + img.numel()].view(img.shape)
        view.copy_(img.to(DEV))
        assert view.data_ptr() % 16 == off % 16
        if ok:
            out, out_b = _launch(c, x=view)
            _same(out, out_b, c["oq_shared"], c, "x 16 elements into its buffer")
            continue
        with G.guarded_allocations(0) as log:
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                _launch(c, x=view)
        torch.cuda.synchronize()
        G.check_all(log, body=lambda g: False)
        for g in log:
            if g.view.dtype != torch.int8:
                assert bool((g.words == G._i32(G.PATTERN)).all())      # nothing was launched: out and the blocked image still hold the pattern
        q = qact.QActivation(view, 0.05, 100, c["xq"][0].shape)
        for fn in (lambda: qact.relu(q), lambda: qact.add(q, q), lambda: qact.max_pool2d(q, 3, 2, 1), lambda: qact.dequantize(q), lambda: qact.flatten(q, 1),
                   lambda: qact.adaptive_avg_pool2d(q, 1)):
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                fn()
    assert F.q8_blocked_shape((2, 20, 9, 8)) == (2, 2, 9, 8, 16)
