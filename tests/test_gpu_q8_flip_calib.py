"""GPU: the observers of the INT8 Flipout layers (csrc/bt_q8_observe.hip's input sweep; csrc/bt_fused_flipout_obs.hip, the fused forward's OBS form) and the
prepare(flipout=True) / calibrate / convert(flipout=True) flow built on them.

The oracle of the ranges is tests/_q8_flip_model.py's ``float_flipout`` (double) through tests/_q8cal_flip_cases.py. Operands and the
statistics sit inside guard bands (tests/_guard.py). Tolerances (the project's): mu, eps, in, sign_in, sign_out, xp exact; sigma, delta 8
fp32 ulps of the row's largest magnitude; mean, pert, pert_signed, out 1e-4 of the row's largest magnitude. Every test prints what it
measured."""
import re

import pytest
import torch

import _guard as G
import _q8_flip_model as FM
import _q8cal_cases as K
import _q8cal_flip_cases as KF
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

INF = float("inf")
R = KF.ROWS.index
ACT_ROWS = ("in", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed")      # what the two new launches fill


def dev():
    return torch.device("cuda:0")


def C3(s, p, d=1):
    return dict(stride=(s, s), padding=(p, p), dilation=(d, d), groups=1)


def fresh_stats(off=0):
    mm = G.place_result((13, 2), off, device=dev(), tag="stats")
    mm.view[:, 0], mm.view[:, 1] = INF, -INF
    bad = G.place_result((1,), (off + 1) & 3, device=dev(), dtype=torch.int32, tag="nonfinite")
    bad.view.zero_()
    return mm, bad


def read(mm, bad):
    torch.cuda.synchronize()
    G.check(mm, body=False), G.check(bad, body=True)
    return mm.view.cpu(), int(bad.view.cpu())


def make_case(wshape, xshape, conv, S=1, bias=True, affine=False, shared=True, seed=0):
    """A seeded layer, input and whole draw on the CPU. xshape: one sample's [B, ...]."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    Co, B = wshape[0], xshape[0]
    c = dict(conv=conv, S=S, shared=shared, mu=r(*wshape) * 0.2, rho=-2.0 + 0.3 * r(*wshape), x=r(*((B if shared else S * B,) + tuple(xshape[1:]))) * 1.5 + 0.1)
    c["mu_b"], c["rho_b"] = (r(Co) * 0.3, -1.5 + 0.2 * r(Co)) if bias else (None, None)
    c["coef"], c["shift"] = (0.5 + torch.rand(Co, generator=g), r(Co) * 0.4) if affine else (None, None)
    if conv is None:
        oshape = (B, Co)
    else:
        from bayesian_torch_amd import functional as F
        oshape = (B, Co) + F.conv_out_hw(xshape[2], xshape[3], wshape[2], wshape[3], *conv["stride"], *conv["padding"], *conv["dilation"])
    c["eps_w"], c["eps_b"] = r(S, *wshape), r(S, Co) if bias else None
    c["sign_in"], c["sign_out"] = KF.sgn(r(S, *xshape)), KF.sgn(r(S, *oshape))
    c["oshape"] = oshape
    return c


def observe(c, mm, bad, x_off=0, draws=True, **coords):
    """The two new launches on a case: supplied draws (``draws``) or the on-chip streams of ``coords``. -> their kernel names."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    d = lambda t, off=0: None if t is None else G.place(t.to(dev()), off)
    x = d(c["x"], x_off)
    at = dict(S=c["S"], shared_x=c["shared"], **coords)
    sin = d(c["sign_in"], x_off) if draws else None
    F.q8_flip_observe_x(x, mm.view[R("in")], mm.view[R("sign_in")], mm.view[R("xp")], bad.view, sign_in=sin, **at)
    names = [_lib.lib().bt_last_kernel_name().decode()]
    dr = dict(eps_w=d(c["eps_w"]), eps_b=d(c["eps_b"]), sign_in=sin, sign_out=d(c["sign_out"], 1 if x_off else 0)) if draws else {}
    F.q8_flip_observe(x, d(c["mu"]), d(c["rho"]), d(c["mu_b"]), d(c["rho_b"]), mm.view[R("mean")], mm.view[R("pert")], mm.view[R("pert_signed")],
                      mm.view[R("sign_out")], bad.view, conv=c["conv"], coef=d(c["coef"], 3), shift=d(c["shift"], 1), **dr, **at)
    names.append(_lib.lib().bt_last_kernel_name().decode())
    c["launch"] = _lib.last_launch_info()
    return names


def want_of(c):
    return KF.host_stats(c["x"], c["mu"], c["rho"], c["eps_w"], c["sign_in"], c["sign_out"], c["mu_b"], c["rho_b"], c["eps_b"], c["conv"], c["coef"], c["shift"],
                         c["shared"])


# name: (weight shape, one sample's x shape, conv, the kernel form expected, S, bias, affine, shared x, x offset)
PARITY = {
    "conv_5x7_9x9": ((7, 5, 3, 3), (2, 5, 9, 9), C3(1, 1), "conv,notrans", 1, True, False, True, 0),        # 162 positions: a partial third tile; padding taps
    "conv_5x7_9x9_s2": ((7, 5, 3, 3), (2, 5, 9, 9), C3(2, 1), "conv,notrans", 3, True, True, False, 1),     # 5 x 5 outputs; S = 3, per-sample x, misaligned
    "conv_5x70_6x6": ((70, 5, 3, 3), (2, 5, 6, 6), C3(1, 1), "conv,notrans", 1, False, True, True, 0),      # two channel tiles, the second of 6 channels
    "conv_8x7_8x8_patch": ((7, 8, 3, 3), (3, 8, 8, 8), C3(1, 1), "conv,notrans", 2, True, False, True, 3),  # 64-pixel images: x staged as a patch
    "conv_20x6_1x1": ((6, 20, 3, 3), (5, 20, 1, 1), C3(1, 1), "conv,trans", 1, True, False, True, 0),       # a 3 x 3 kernel on a 1 x 1 map
    "conv_5x7_2x2_pix": ((7, 5, 3, 3), (3, 5, 2, 2), C3(1, 1), "conv,trans", 3, False, False, False, 2),    # pixel-major tiles
    "linear_567x4": ((4, 567), (5, 567), None, "conv,trans", 3, True, False, True, 0),                      # K % 4 != 0: the 1 x 1 convolution
    "linear_64x70": ((70, 64), (67, 64), None, "linear,trans", 1, True, True, True, 0),                     # float4 rows; two tiles both ways
    "linear_64x70_off": ((70, 64), (5, 64), None, "conv,trans", 2, False, False, False, 1),                 # misaligned x: no float4 rows
}


@pytest.mark.parametrize("name", list(PARITY))
def test_model_parity_injected_draws(name):
    wshape, xshape, conv, form, S, bias, affine, shared, off = PARITY[name]
    c = make_case(wshape, xshape, conv, S, bias, affine, shared, seed=len(name))
    mm, bad = fresh_stats(off)
    names = observe(c, mm, bad, x_off=off, sample0=5)
    st, nbad = read(mm, bad)
    assert names[0] == "q8_flip_observe_x<signs injected>", names
    m = re.fullmatch(r"fused_fwd_kernel<(\d+),(\d+),\d+,flip,(\w+,\w+),inj=1,obs>", names[1])
    assert m and m.group(3) == form, names
    bn, bm = int(m.group(1)), int(m.group(2))
    if name == "conv_5x70_6x6":
        assert wshape[0] > bn and c["launch"]["n_tiles"] == 2          # more output channels than one channel tile of the instantiation that ran
    if name in ("conv_5x7_9x9", "linear_64x70"):
        assert c["launch"]["m_tiles"] > 1 and (c["oshape"][0] * (c["oshape"][2] * c["oshape"][3] if conv else 1)) % bm
    want, mags = want_of(c)
    assert nbad == 0
    KF.check_rows(st, want, mags, name, rows=ACT_ROWS)
    untouched = [R(n) for n in KF.ROWS if n not in ACT_ROWS]
    assert bool((st[untouched, 0] == INF).all()) and bool((st[untouched, 1] == -INF).all())


def test_padding_lanes_stay_out():
    """mu, x and mu_b all positive: every valid mean is strictly positive, and a kernel that lets the zero-filled lanes of a partial
    tile (7 of 64 channels, 50 of 64 positions) into a range reports a minimum of 0. The mirror for pert_signed: sigma * eps, x and
    sigma_b * eps_b positive, sign_in = sign_out = +1."""
    c = make_case((7, 5, 3, 3), (2, 5, 9, 9), C3(2, 1), seed=3)
    c["mu"], c["x"], c["mu_b"] = c["mu"].abs() + 0.05, c["x"].abs() + 0.1, c["mu_b"].abs() + 0.2
    c["eps_w"], c["eps_b"] = c["eps_w"].abs() + 0.1, c["eps_b"].abs() + 0.1
    c["sign_in"], c["sign_out"] = torch.ones_like(c["sign_in"]), torch.ones_like(c["sign_out"])
    mm, bad = fresh_stats()
    observe(c, mm, bad)
    st, nbad = read(mm, bad)
    want, mags = want_of(c)
    print(f"positive case: mean min {float(st[R('mean'), 0]):.5f}, pert_signed min {float(st[R('pert_signed'), 0]):.5f}, sign_out {st[R('sign_out')].tolist()}")
    assert nbad == 0 and float(st[R("mean"), 0]) > 0 and float(st[R("pert"), 0]) > 0 and float(st[R("pert_signed"), 0]) > 0
    assert st[R("sign_out")].tolist() == [1.0, 1.0] and st[R("sign_in")].tolist() == [1.0, 1.0]
    KF.check_rows(st, want, mags, "positive", rows=ACT_ROWS)
    c["sign_out"] = -c["sign_out"]          # all -1: pert_signed strictly negative, a zero lane would report a maximum of 0
    mm, bad = fresh_stats()
    observe(c, mm, bad)
    st, _ = read(mm, bad)
    assert float(st[R("pert_signed"), 1]) < 0 and st[R("sign_out")].tolist() == [-1.0, -1.0]


@pytest.mark.parametrize("where", ["first", "last", "tile_edge"])
def test_planted_extremes(where):
    """One large x makes a chosen output element the mean's maximum: the first element, the last valid one, and the last column of the
    first position tile (position 63 of 162)."""
    c = make_case((7, 5, 3, 3), (2, 5, 9, 9), C3(1, 1), seed=8)
    b, co, ho, wo = {"first": (0, 0, 0, 0), "last": (1, 6, 8, 8), "tile_edge": (0, 3, 7, 0)}[where]          # (0, ., 7, 0): m = 63
    c["mu"] = c["mu"].abs() + 0.05
    c["mu"][:, :, 1, 1] += 1.0          # the centre tap dominates: the planted pixel's own output position wins ...
    c["mu"][co, :, 1, 1] += 2.0         # ... in the chosen channel
    c["x"][b, :, ho, wo] = 400.0
    mm, bad = fresh_stats()
    observe(c, mm, bad)
    st, nbad = read(mm, bad)
    want, mags = want_of(c)
    _, t = FM.float_flipout(c["x"], c["mu"], K.softplus_host(c["rho"]), c["eps_w"][0], c["sign_in"][0], c["sign_out"][0], c["mu_b"], K.softplus_host(c["rho_b"]),
                            c["eps_b"][0], c["conv"])
    at = tuple(int(v) for v in torch.unravel_index(t["mean"].flatten().argmax(), t["mean"].shape))
    assert at == (b, co, ho, wo) and nbad == 0          # the mean's maximum is the chosen output element
    assert float(st[R("in"), 1]) == 400.0
    KF.check_rows(st, want, mags, f"planted {where}", rows=ACT_ROWS)


@pytest.mark.parametrize("name", ["conv_5x7_9x9_s2", "conv_5x7_2x2_pix", "linear_567x4", "linear_64x70"])
def test_on_chip_draws_equal_the_filled_streams(name):
    from bayesian_torch_amd import functional as F
    wshape, xshape, conv, form, _, bias, affine, shared, off = PARITY[name]
    S, coords = 3, dict(seed=1234, call=17, layer_id=3, sample0=5)
    c = make_case(wshape, xshape, conv, S, bias, affine, shared, seed=21)
    mm, bad = fresh_stats(off)
    names = observe(c, mm, bad, x_off=off, draws=False, **coords)
    st, nbad = read(mm, bad)
    assert names[0] == "q8_flip_observe_x<signs on chip>" and names[1].endswith("inj=0,obs>") and form in names[1], names
    fill = lambda fn, t, shape: fn(coords["seed"], coords["call"], coords["layer_id"], coords["sample0"], t, S, shape, dev()).cpu()
    c["eps_w"], c["eps_b"] = fill(F.rng_fill_normal, 0, wshape), fill(F.rng_fill_normal, 1, (wshape[0],)) if bias else None
    c["sign_in"], c["sign_out"] = fill(F.rng_fill_sign, 2, xshape), fill(F.rng_fill_sign, 3, c["oshape"])
    mm2, bad2 = fresh_stats(off)
    observe(c, mm2, bad2, x_off=off)
    st2, nbad2 = read(mm2, bad2)
    assert nbad == 0 and nbad2 == 0 and torch.equal(st, st2), (st, st2)
    assert st[R("sign_in")].tolist() == [-1.0, 1.0] and st[R("sign_out")].tolist() == [-1.0, 1.0]
    want, mags = want_of(c)
    KF.check_rows(st, want, mags, f"on chip {name}", rows=ACT_ROWS)


def test_merging_and_nonfinite():
    c = make_case((7, 5, 3, 3), (2, 5, 9, 9), C3(1, 1), S=4, seed=13)
    mm, bad = fresh_stats()
    observe(c, mm, bad)
    st4, _ = read(mm, bad)
    halves = []
    for lo in (0, 2):          # S = 4 equals two calls of S = 2 into the same statistics
        h = dict(c, S=2, **{k: c[k][lo:lo + 2].contiguous() for k in ("eps_w", "eps_b", "sign_in", "sign_out")})
        halves.append(h)
    mm2, bad2 = fresh_stats()
    observe(halves[0], mm2, bad2)
    first, _ = read(mm2, bad2)
    observe(halves[1], mm2, bad2)
    both, _ = read(mm2, bad2)
    assert torch.equal(both, st4)
    fin = torch.isfinite(first)
    assert bool((both[:, 0][fin[:, 0]] <= first[:, 0][fin[:, 0]]).all()) and bool((both[:, 1][fin[:, 1]] >= first[:, 1][fin[:, 1]]).all())          # a second call only widens
    assert not torch.equal(first, both)
    observe(halves[0], mm2, bad2)          # a subset: nothing can widen
    again, nbad = read(mm2, bad2)
    assert torch.equal(again, both) and nbad == 0
    # an infinite x: counted (by the sweep, and by every output it reaches), and the statistics stay finite
    c1 = make_case((7, 5, 3, 3), (2, 5, 9, 9), C3(1, 1), seed=13)
    c1["x"][1, 2, 4, 4] = INF
    mm3, bad3 = fresh_stats()
    observe(c1, mm3, bad3)
    st, nbad = read(mm3, bad3)
    acts = [R(n) for n in ACT_ROWS]
    print(f"an infinite x: {nbad} non-finite values counted")
    assert nbad >= 2 + 3 * 9 and bool(torch.isfinite(st[acts]).all())          # x and xp; mean, pert, pert_signed of at least the nine positions of one channel
    c1["x"][1, 2, 4, 4] = 0.0
    fin_x = c1["x"].clone()
    mask = torch.ones(2, 7, 9, 9, dtype=torch.bool)
    mask[1, :, 3:6, 3:6] = False          # the outputs the infinite element reached
    _, t = FM.float_flipout(fin_x, c1["mu"], K.softplus_host(c1["rho"]), c1["eps_w"][0], c1["sign_in"][0], c1["sign_out"][0], c1["mu_b"], K.softplus_host(c1["rho_b"]),
                            c1["eps_b"][0], c1["conv"])
    for n in ("mean", "pert", "pert_signed"):
        v = t[n][mask]
        mag = float(t[n].abs().max())
        assert abs(float(st[R(n), 0]) - float(v.min())) <= 1e-4 * mag and abs(float(st[R(n), 1]) - float(v.max())) <= 1e-4 * mag, n


# ---------------------------------------------------------------------------- the layers
def _layer_of(tag, g):
    import bayesian_torch_amd.layers as L
    if tag.startswith("linear"):
        layer = L.LinearFlipout(g["mu_w"].shape[1], g["mu_w"].shape[0])
        names = ("mu_weight", "rho_weight")
    else:
        layer = L.Conv2dFlipout(g["mu_w"].shape[1], g["mu_w"].shape[0], 3, padding=1)
        names = ("mu_kernel", "rho_kernel")
    with torch.no_grad():
        getattr(layer, names[0]).copy_(g["mu_w"]), getattr(layer, names[1]).copy_(g["rho_w"])
        layer.mu_bias.copy_(g["mu_b"]), layer.rho_bias.copy_(g["rho_b"])
    layer.dnn_to_bnn_flag = True
    return layer.to(dev()).eval()


def test_prepared_layer_computes_what_its_twin_computes(monkeypatch):
    import copy
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    torch.manual_seed(5)
    rng.set_mode("philox")
    for make, x in ((lambda: L.Conv2dFlipout(5, 7, 3, padding=1), torch.randn(2, 5, 9, 9)), (lambda: L.LinearFlipout(33, 6), torch.randn(5, 33))):
        a = make().to(dev()).eval()
        b = copy.deepcopy(a)
        b._layer_id = a._layer_id
        b.prepare(flipout=True)
        assert b.calib_minmax.shape == (13, 2) and b.quant_prepare
        xd = x.to(dev())
        with torch.no_grad():
            call = rng.peek_call()
            out_a, kl_a = a(xd)
            rng.set_call(call)          # the twin's forward at the same RNG coordinates
            out_b, kl_b = b(xd)
        torch.cuda.synchronize()
        assert a._last["rng"] == b._last["rng"]
        assert torch.equal(out_a, out_b) and torch.equal(kl_a, kl_b)
        assert b._last["observed"] is True and "observed" not in a._last
        ks = b._last["observer_kernels"]
        assert ks[0] == "q8_observe_w<eps on chip>" and ks[1] == "q8_flip_observe_x<signs on chip>" and ks[2].endswith("inj=0,obs>") and ks[3] == "minmax_update<1 segs>", ks
        assert bool(torch.isfinite(b.calib_minmax).all()) and int(b.calib_nonfinite) == 0
        d = {k: v.cpu() for k, v in b.materialize_last_draw().items()}
        conv = None if x.dim() == 2 else C3(1, 1)
        w = "weight" if conv is None else "kernel"
        want, mags = KF.host_stats(x, getattr(b, "mu_" + w), getattr(b, "rho_" + w), d["eps_w"], d["sign_in"], d["sign_out"], b.mu_bias, b.rho_bias, d["eps_b"], conv)
        KF.check_rows(b.calib_minmax.cpu(), want, mags, type(b).__name__)
        with pytest.raises(RuntimeError, match="no_grad"):
            b(xd.clone().requires_grad_(True))
        with monkeypatch.context() as mp:          # what the observers ask before they launch; no capture is started here
            mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            with pytest.raises(RuntimeError, match="graph capture"), torch.no_grad():
                b(xd)
        torch.cuda.synchronize()


def test_torch_rng_mode_observes_the_draw_it_read():
    """rng mode "torch": the draw comes from torch's generator and is read by the forward; the observers read the same tensors."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    torch.manual_seed(9)
    layer = L.Conv2dFlipout(5, 7, 3, stride=2, padding=1).to(dev()).eval()
    layer.prepare(flipout=True)
    x = torch.randn(2, 5, 9, 9)
    rng.set_mode("torch")
    try:
        with torch.no_grad(), mc.mc_samples(3, batch=2):
            layer(x.to(dev()))
        torch.cuda.synchronize()
        ks = layer._last["observer_kernels"]
        assert ks[0] == "q8_observe_w<eps injected>" and ks[1] == "q8_flip_observe_x<signs injected>" and ks[2].endswith("inj=1,obs>"), ks
        d = {k: v.cpu() for k, v in layer.materialize_last_draw().items()}
    finally:
        rng.set_mode("philox")
    assert d["eps_w"].shape[0] == 3 and int(layer.calib_nonfinite) == 0
    want, mags = KF.host_stats(x, layer.mu_kernel, layer.rho_kernel, d["eps_w"], d["sign_in"], d["sign_out"], layer.mu_bias, layer.rho_bias, d["eps_b"], C3(2, 1))
    KF.check_rows(layer.calib_minmax.cpu(), want, mags, "torch mode")


@pytest.mark.parametrize("tag", KF.FIXTURES)
def test_fixtures_through_the_layers(tag):
    from bayesian_torch_amd.quantization import convert
    g = KF.load(tag)
    layer = _layer_of(tag, g)
    layer.prepare(flipout=True)
    n = g["x"].shape[0]
    layer.inject_draw = [dict(eps_w=g["eps_w"][i:i + 1].to(dev()), eps_b=g["eps_b"][i:i + 1].to(dev()), sign_in=g["sign_in"][i:i + 1].to(dev()),
                              sign_out=g["sign_out"][i:i + 1].to(dev())) for i in range(n)]
    with torch.no_grad():
        for i in range(n):
            layer(g["x"][i].to(dev()))
            assert layer._last["observed"] is True and layer._last["observer_kernels"][0] == "q8_observe_w<eps injected>"
    torch.cuda.synchronize()
    st = layer.calib_minmax.cpu()
    assert int(layer.calib_nonfinite) == 0
    want = g["minmax13"]          # the reference's twelve recorded ranges in CALIB_FLIP_ROWS' order ("add": not an observer of the reference's)
    mags = {k: float(want[KF.ROWS.index(k)].abs().max()) for k in KF.ROWS}
    KF.check_rows(st, want, mags, f"layer {tag} vs the recorded ranges")
    seq = torch.nn.Sequential(layer)
    convert(seq, flipout=True)
    qd = seq[0].quant_dict
    assert type(seq[0]).__name__.startswith("Quantized") and len(qd) == 10 and qd == KF.dict_of(st)
    for i, name in enumerate(FM.PAIRS):
        zp, sc = int(g["dict_zero_points"][i]), float(g["dict_scales"][i])
        rel = abs(qd[i]["scale"] - sc) / sc
        bound = 0.0 if name in KF.EXACT else (8 * 2.0 ** -23 if name in KF.ULPS8 else KF.REL_TOL)
        print(f"{tag}: {name}: scale {qd[i]['scale']:.8g} vs recorded {sc:.8g} (relative {rel:.2e}, bound {bound:.2e}); zero point {qd[i]['zero_point']} vs {zp}")
        assert qd[i]["zero_point"] == zp and rel <= bound, (name, qd[i], sc, zp)


def _inject(net, d):
    for name in ("conv1", "fc"):
        getattr(net, name).inject_draw = {k: v.to(dev()) for k, v in d[name].items()}


def _q8_model_forward(qnet, x, d):
    """The converted FoldNet through the INT8 Flipout model (tests/_q8_flip_model.py) on the CPU, with the layers' own pairs -> logits."""
    cpu = lambda t: None if t is None else t.detach().cpu()

    def one(q, xin, dd, conv):
        pairs = FM.scales_from_dict(q.quant_dict) if q.quant_dict is not None else q._last["pairs"]
        eb = dd["eps_b"][0] if q.quantized_sigma_bias is not None else None
        return FM.forward(xin, cpu(q.quantized_mu_weight), cpu(q.quantized_sigma_weight), float(q.quantized_mu_scale.item()), float(q.quantized_sigma_scale.item()),
                          pairs, dd["eps_w"][0], dd["sign_in"][0], dd["sign_out"][0], cpu(q.quantized_mu_bias), cpu(q.quantized_sigma_bias), eb, conv)[1]

    y = one(qnet.conv1, x, d["conv1"], KF.CONV1)
    return one(qnet.fc, torch.relu(y).flatten(1), d["fc"], None)


def test_folded_model_calibrates_converts_and_helps():
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch_amd.quantization import convert, prepare
    net, xs, draws = KF.fold_net()
    ref, _, _ = KF.fold_net()
    net = net.to(dev())
    prepare(net, fuse_conv_bn=True, flipout=True)
    assert net.conv1.quant_prepare and net.fc.quant_prepare and net.conv1._calib_fused and not net.fc._calib_fused
    with torch.no_grad():
        for x, d in zip(xs, draws):
            _inject(net, d)
            net(x.to(dev()))
    torch.cuda.synchronize()
    host = KF.fold_host_stats(ref, xs, draws)
    stats = {}
    for name in ("conv1", "fc"):
        stats[name] = getattr(net, name).calib_minmax.cpu()
        want, mags = host[name]
        # fc reads the device's fp32 BatchNorm / ReLU output, which the host repeats in double: its input rows are held to the relative bound
        KF.check_rows(stats[name], want, mags, f"folded {name}", exact=KF.EXACT if name == "conv1" else ("mu", "eps", "sign_in", "sign_out"))
        assert int(getattr(net, name).calib_nonfinite) == 0
    bn = net.bn1
    convert(net, fuse_conv_bn=True, flipout=True)
    assert not bn._forward_hooks and type(net.bn1).__name__ == "Identity"
    assert type(net.conv1).__name__ == "QuantizedConv2dFlipout" and type(net.fc).__name__ == "QuantizedLinearFlipout"
    assert net.conv1.quant_dict == KF.dict_of(stats["conv1"]) and net.fc.quant_dict == KF.dict_of(stats["fc"])
    dflt, _, _ = KF.fold_net()
    bnn_to_qbnn(dflt, fuse_conv_bn=True, flipout=True)
    dflt = dflt.to(dev())
    errs = {"calibrated": [], "default": []}
    with torch.no_grad():
        for x, d in zip(xs, draws):
            _inject(net, d), _inject(dflt, d)
            out = net(x.to(dev())).cpu()
            assert torch.equal(out, _q8_model_forward(net, x, d))
            want = KF.float_forward(ref, x, d)[1]
            errs["calibrated"].append((out.double() - want).abs().reshape(-1))
            errs["default"].append((dflt(x.to(dev())).cpu().double() - want).abs().reshape(-1))
    cal, dft = (float(torch.cat(errs[k]).mean()) for k in ("calibrated", "default"))
    print(f"mean |int8 - float Flipout|: calibrated {cal:.5f}, default pairs {dft:.5f}")
    assert cal < dft


def test_mc_forward_observes_every_sample():
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.quantization import prepare
    net, xs, _ = KF.fold_net()
    net = net.to(dev())
    prepare(net, fuse_conv_bn=True, flipout=True)
    rng.set_mode("philox")
    out, _ = mc_forward(net, xs[0].to(dev()), 4)
    torch.cuda.synchronize()
    assert out.shape == (4, 4, 4)
    for layer in (net.conv1, net.fc):
        last = layer._last
        assert last["observed"] and last["S"] == 4 and last["observer_kernels"][1] == "q8_flip_observe_x<signs on chip>"
        d = layer.materialize_last_draw()
        assert d["eps_w"].shape[0] == 4 and tuple(layer.calib_minmax[R("eps")].tolist()) == K.aminmax(d["eps_w"])
        assert len({K.aminmax(d["eps_w"][s]) for s in range(4)}) == 4          # four different streams, all four inside the range
        # the perturbation's range is the union over the four samples' own draws
        st = layer.calib_minmax.cpu()
        assert int(layer.calib_nonfinite) == 0 and bool(torch.isfinite(st).all())
        assert st[R("sign_in")].tolist() == [-1.0, 1.0] and st[R("sign_out")].tolist() == [-1.0, 1.0]
    c = net.conv1
    d = {k: v.cpu() for k, v in c.materialize_last_draw().items()}
    coef, shift = KF.bn_affine(net.bn1)
    want, mags = KF.host_stats(xs[0], c.mu_kernel, c.rho_kernel, d["eps_w"], d["sign_in"], d["sign_out"], c.mu_bias, c.rho_bias, d["eps_b"], KF.CONV1, coef.cpu(), shift.cpu())
    KF.check_rows(c.calib_minmax.cpu(), want, mags, "mc_forward conv1", skip=("add", "out"))          # (out: the BatchNorm output's range, checked in the folded test)


def test_input_sweep_with_signs_off_xs_alignment():
    """bt_q8_flip_observe_x over the walk's every branch: x starts 0 to 3 elements past a 16-byte boundary and the supplied signs 0 to
    3, independently (only equal offsets read the signs as 16-byte quads); n of 1, 3, 4, 5, 8, 9 (head only; head and tail; one quad;
    ...) and 1030 (more than one workgroup's threads); S = 2 with x shared and stacked (a stacked sample 1 starts n elements on: its
    head differs from sample 0's). The extremes of x and of x * sign_in are planted, launch by launch, at the first element, the last
    head element, the first quad element and the last tail element of one sample. The three rows are exact: ``torch.equal`` to
    ``torch.aminmax`` of the host tensors. Operands and statistics sit inside guard bands; all of them are held intact."""
    from bayesian_torch_amd import functional as F
    S, rows = 2, ("in", "sign_in", "xp")
    g = torch.Generator().manual_seed(11)
    mm, bad = fresh_stats()
    got, want = [], []
    stray = torch.zeros((), dtype=torch.int64, device=dev())       # words of an operand's bands that no longer hold NaN, over all launches
    for n in (1, 3, 4, 5, 8, 9, 1030):
        for shared in (True, False):
            for x_off in range(4):
                for s_off in range(4):
                    for sp in range(1 if shared else S):
                        head = min((4 - (x_off + sp * n)) % 4, n)
                        tail0 = head + (n - head) // 4 * 4
                        spots = sorted({0, n - 1} | ({head - 1} if head else set()) | ({head} if tail0 > head else set()))
                        for k, hi in enumerate(spots):
                            x = torch.rand((1 if shared else S, n), generator=g) * 2 - 1
                            sg = torch.where(torch.rand((S, n), generator=g) < 0.5, -1.0, 1.0)
                            lo = spots[(k + 1) % len(spots)]
                            x[sp, lo], x[sp, hi] = -9.0, 9.0                        # (one spot: the maximum stays)
                            sg[:, lo] = sg[:, hi] = -1.0                            # x * sign: 9 at ``lo``, -9 at ``hi``
                            xd, sd = G.place(x.reshape(-1).to(dev()), x_off), G.place(sg.reshape(-1).to(dev()), s_off)
                            assert xd.data_ptr() % 16 == 4 * x_off and sd.data_ptr() % 16 == 4 * s_off
                            mm.view[:, 0], mm.view[:, 1] = INF, -INF
                            F.q8_flip_observe_x(xd, mm.view[R("in")], mm.view[R("sign_in")], mm.view[R("xp")], bad.view, S=S, shared_x=shared, sign_in=sd)
                            got.append(mm.view[[R(r) for r in rows]])
                            want.append(torch.tensor([K.aminmax(x), K.aminmax(sg), K.aminmax(x * sg)]))
                            for t in (xd, sd):
                                stray += t._base.numel() - t.numel() - t._base.view(torch.float32).isnan().sum()
    got, (_, nonfinite) = torch.stack(got).cpu(), read(mm, bad)
    print(f"{len(want)} launches; non-finite values met: {nonfinite}; operand band words changed: {int(stray)}")
    assert len(want) == 876 and nonfinite == 0 and int(stray) == 0
    assert torch.equal(got, torch.stack(want))
