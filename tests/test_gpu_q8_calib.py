"""GPU: the observer kernels (csrc/bt_q8_observe.hip) and the prepare / calibrate / convert flow built on them.

Inputs and the statistics buffers sit inside guard bands (tests/_guard.py). Rows that pass through the device softplus (sigma, mul, add)
are held to 8 fp32 ulps of the largest magnitude of the tensor concerned (2 from the softplus, one per further rounding, doubled);
mu, eps, in and out are exact. Every test prints the deviation it measured."""
import pytest
import torch

import _guard as G
import _q8cal_cases as K
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

SHAPES = [(7, 5, 3, 3), (33, 19, 3, 3), (70, 9, 3, 3), (10, 784)]
INF = float("inf")


def dev():
    return torch.device("cuda:0")


def fresh_stats(off=0):
    """A guarded [7, 2] statistics buffer of (+inf, -inf) pairs and a guarded zero counter."""
    mm = G.place_result((7, 2), off, device=dev(), tag="stats")
    mm.view[:, 0], mm.view[:, 1] = INF, -INF
    bad = G.place_result((1,), (off + 1) & 3, device=dev(), dtype=torch.int32, tag="nonfinite")
    bad.view.zero_()
    return mm, bad


def read(mm, bad, rows=7):
    torch.cuda.synchronize()
    G.check(mm, body=False), G.check(bad, body=True)
    return mm.view.cpu(), int(bad.view.cpu())


def params(shape, seed, off):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(shape, generator=g) * 0.1
    rho = -1.0 + 0.2 * torch.randn(shape, generator=g)          # sigma about 0.3: five sigmas dwarf every mu
    return mu, rho, G.place(mu.to(dev()), off), G.place(rho.to(dev()), (off + 2) & 3 if off else 0)


def positions(n, S):
    """(flat index into eps [S, n], value): first, n - 1 of sample 0, a workgroup boundary (thread 256's first element), sample 2, last."""
    wg = 1024 if n > 1025 else n // 2
    return [(0, 5.0), (n - 1, -5.0), (wg, 5.0), (wg - 1, -5.0), (2 * n + n // 3, -5.0), (S * n - 1, 5.0)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off4B"])
def test_planted_extremes_injected(shape, off):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    S = 3
    mu, rho, mu_d, rho_d = params(shape, 3, off)
    n = mu.numel()
    assert n % 4 != 0 or shape != (7, 5, 3, 3)          # 315: a tail that is no multiple of 4
    worst = 0.0
    for idx, val in positions(n, S):
        eps = torch.zeros((S,) + shape)
        eps.view(-1)[idx] = val
        mm, bad = fresh_stats(off)
        F.q8_observe_w(mu_d, rho_d, mm.view, bad.view, S=S, eps=G.place(eps.to(dev()), off))
        assert _lib.lib().bt_last_kernel_name() == b"q8_observe_w<eps injected>"
        st, nbad = read(mm, bad)
        assert nbad == 0
        assert (float(st[2, 0]), float(st[2, 1])) == (min(0.0, val), max(0.0, val)), (idx, st[2])
        assert bool((st[5:, 0] == INF).all()) and bool((st[5:, 1] == -INF).all())          # the activation rows are not the sweep's
        rows = K.host_weight_rows(mu, rho, eps)
        e = idx % n
        t_p = float(rows["sigma"].view(-1)[e] * val)          # one fp32 rounding
        assert K.aminmax(rows["mul"]) == (min(0.0, t_p), max(0.0, t_p))
        w = rows["add"].view(-1)
        assert int(w.argmax() if val > 0 else w.argmin()) == idx                          # the add extreme is found at the planted element
        worst = max(worst, K.check_weight_rows(st, rows, f"{shape} idx {idx}"))
    print(f"planted {shape} off {off}: worst deviation {worst:.2f} ulps")


COUNTS = [1, 3, 315, 1027, 4099]          # 1027, 4099: above one workgroup's span of 256 threads x 4 elements


def test_minmax_update_planted_and_random():
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    g = torch.Generator().manual_seed(5)
    for n in COUNTS:
        for off in (0, 1, 3):
            for idx, val in ((0, 5.0), (n - 1, -5.0), (n // 2, 5.0)):
                x = torch.zeros(n)
                x[idx] = val
                mm, bad = fresh_stats()
                F.minmax_update([(G.place(x.to(dev()), off), mm.view[5])], bad.view)
                st, nbad = read(mm, bad)
                assert nbad == 0 and (float(st[5, 0]), float(st[5, 1])) == K.aminmax(x), (n, off, idx, st[5])          # (n = 1: the planted value alone)
                assert bool((st[:5, 0] == INF).all()) and bool((st[6:, 1] == -INF).all())
    # four segments in one launch, every misalignment, random data, all-positive and all-negative tensors
    xs = [torch.randn(n, generator=g) * 3 + sh for n, sh in zip((1, 3, 315, 4099), (0.0, 10.0, -10.0, 0.5))]
    mm, bad = fresh_stats()
    extra = G.place_result((2, 2), 2, device=dev(), tag="more pairs")
    extra.view[:, 0], extra.view[:, 1] = INF, -INF
    dsts = [mm.view[5], mm.view[6], extra.view[0], extra.view[1]]
    F.minmax_update([(G.place(x.to(dev()), off), d) for x, off, d in zip(xs, (0, 1, 2, 3), dsts)], bad.view)
    assert _lib.lib().bt_last_kernel_name() == b"minmax_update<4 segs>"
    st, nbad = read(mm, bad)
    G.check(extra, body=True)
    got = [tuple(st[5].tolist()), tuple(st[6].tolist()), tuple(extra.view[0].tolist()), tuple(extra.view[1].tolist())]
    assert nbad == 0 and got == [K.aminmax(x) for x in xs]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("with_coef", [False, True], ids=["plain", "coef"])
def test_on_chip_draws(shape, with_coef):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    S, sample0, seed, call, lid = 3, 5, 1234, 17, 3
    mu, rho, mu_d, rho_d = params(shape, 9, 0 if shape == (10, 784) else 1)          # (10, 784) aligned: the 16-byte path of taps == 1
    coef = 0.5 + torch.rand(shape[0], generator=torch.Generator().manual_seed(2)) if with_coef else None
    mm, bad = fresh_stats(2)
    F.q8_observe_w(mu_d, rho_d, mm.view, bad.view, S=S, coef=None if coef is None else G.place(coef.to(dev()), 3), seed=seed, call=call, layer_id=lid, sample0=sample0)
    assert _lib.lib().bt_last_kernel_name() == b"q8_observe_w<eps on chip>"
    st, nbad = read(mm, bad)
    eps = F.rng_fill_normal(seed, call, lid, sample0, 0, S, shape, dev())
    assert nbad == 0 and (float(st[2, 0]), float(st[2, 1])) == K.aminmax(eps)
    K.check_weight_rows(st, K.host_weight_rows(mu, rho, eps, coef), f"on chip {shape} coef {with_coef}")


def test_merging_and_nonfinite():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    mm, bad = fresh_stats()
    a, b, c = torch.linspace(-1.0, 2.0, 700), torch.linspace(0.5, 7.0, 50), torch.linspace(0.0, 1.0, 9)
    for x, want in ((a, (-1.0, 2.0)), (b, (-1.0, 7.0)), (c, (-1.0, 7.0))):          # the union; a narrower range changes nothing
        F.minmax_update([(x.to(dev()), mm.view[5])], bad.view)
        st, nbad = read(mm, bad)
        assert (float(st[5, 0]), float(st[5, 1])) == want and nbad == 0
    shape = (7, 5, 3, 3)
    mu, rho, mu_d, rho_d = params(shape, 4, 0)
    e1, e2 = torch.randn((2,) + shape), 3 * torch.randn((1,) + shape)
    F.q8_observe_w(mu_d, rho_d, mm.view, bad.view, S=2, eps=e1.to(dev()))
    F.q8_observe_w(mu_d, rho_d, mm.view, bad.view, S=1, eps=e2.to(dev()))
    st, _ = read(mm, bad)
    K.check_weight_rows(st, K.host_weight_rows(mu, rho, torch.cat([e1, e2])), "two calls")
    F.q8_observe_w(mu_d, rho_d, mm.view, bad.view, S=1, eps=e1[1:].contiguous().to(dev()))          # a subset: nothing can widen
    st2, _ = read(mm, bad)
    assert torch.equal(st, st2)
    # a NaN and an inf are skipped and counted; the converter refuses a layer that met any
    layer = L.LinearReparameterization(6, 3).to(dev())
    layer.prepare()
    x = torch.linspace(-2.0, 3.0, 1030)
    x[7], x[1029] = float("nan"), INF
    F.minmax_update([(x.to(dev()), layer.calib_minmax[5])], layer.calib_nonfinite)
    torch.cuda.synchronize()
    assert int(layer.calib_nonfinite) == 2 and tuple(layer.calib_minmax[5].tolist()) == K.aminmax(x[torch.isfinite(x)])
    e = torch.zeros(1, 3, 6)
    e[0, 1, 2] = -INF
    F.q8_observe_w(layer.mu_weight.detach(), layer.rho_weight.detach(), layer.calib_minmax, layer.calib_nonfinite, eps=e.to(dev()))
    torch.cuda.synchronize()
    assert int(layer.calib_nonfinite) == 2 + 3          # eps, its product and the sum
    layer.calib_minmax[6] = torch.tensor([0.0, 1.0])
    with pytest.raises(RuntimeError, match="non-finite"):
        bnn_to_qbnn(torch.nn.Sequential(layer))


def _layer_of(tag, g):
    import bayesian_torch_amd.layers as L
    if tag.startswith("linear"):
        layer = L.LinearReparameterization(g["mu_w"].shape[1], g["mu_w"].shape[0])
        names = ("mu_weight", "rho_weight")
    else:
        layer = L.Conv2dReparameterization(g["mu_w"].shape[1], g["mu_w"].shape[0], 3, padding=1)
        names = ("mu_kernel", "rho_kernel")
    with torch.no_grad():
        getattr(layer, names[0]).copy_(g["mu_w"]), getattr(layer, names[1]).copy_(g["rho_w"])
        layer.mu_bias.copy_(g["mu_b"]), layer.rho_bias.copy_(g["rho_b"])
    layer.dnn_to_bnn_flag = True
    return layer.to(dev()).eval()


@pytest.mark.parametrize("tag", K.FIXTURES)
def test_through_the_layers_against_the_reference(tag):
    from bayesian_torch_amd.quantization import convert
    g = K.load(tag)
    layer = _layer_of(tag, g)
    x0 = g["x"][0].to(dev()).requires_grad_(True)
    layer.prepare()
    with pytest.raises(RuntimeError, match="no_grad"):          # a forward that needs grad refuses while the layer calibrates
        layer(x0)
    layer.inject_draw = [dict(eps_w=g["eps_w"][i:i + 1].to(dev()), eps_b=g["eps_b"][i:i + 1].to(dev())) for i in range(3)]
    with torch.no_grad():
        for i in range(3):
            layer(g["x"][i].to(dev()))
            assert layer._last["observed"] is True and layer._last["observer_kernel"] == "q8_observe_w<eps injected>"
            assert layer._last["observer_kernels"][1] == "minmax_update<2 segs>" and not layer._last["kernel"].startswith(("q8_observe", "minmax"))
    torch.cuda.synchronize()
    st, want = layer.calib_minmax.cpu(), g["minmax"]
    assert int(layer.calib_nonfinite) == 0
    assert torch.equal(st[2], want[2]) and torch.equal(st[5], want[5]) and torch.equal(st[1], want[1]), (st, want)          # eps, in (and mu) exactly
    K.check_weight_rows(st, K.host_weight_rows(g["mu_w"], g["rho_w"], g["eps_w"]), f"layer {tag}")
    for i, name in ((0, "sigma"), (3, "mul"), (4, "add")):          # and against the reference's RECORDED ranges (its host's softplus)
        mag = float(want[i].abs().max()) if name != "add" else float(want[1].abs().max()) + float(want[3].abs().max())
        d = float((st[i] - want[i]).abs().max())
        print(f"{tag}: {name} vs the recorded range: {d / (K.ulps(mag) / 8):.2f} ulps")
        assert d <= K.ulps(mag), (name, st[i], want[i])
    rel = ((st[6] - want[6]).abs() / want[6].abs()).max()
    print(f"{tag}: out range relative deviation {float(rel):.3e} (bound 1e-4)")
    assert float(rel) <= 1e-4, (st[6], want[6])
    seq = torch.nn.Sequential(layer)
    convert(seq)
    assert seq[0].quant_dict == K.dict_of(st) and type(seq[0]).__name__.startswith("Quantized")
    ref = [dict(scale=float(s), zero_point=int(z)) for s, z in zip(g["dict_scales"].tolist(), g["dict_zero_points"].tolist())]
    print(f"{tag}: quant_dict {seq[0].quant_dict}\n   the reference's {ref}")


def _prepared_fold_net(fuse=True):
    from bayesian_torch_amd.quantization import prepare
    net, xs, draws = K.fold_net()
    net = net.to(dev())
    prepare(net, fuse_conv_bn=fuse)
    return net, xs, draws


def _inject(net, d):
    for name in ("conv1", "fc"):
        getattr(net, name).inject_draw = {k: v.to(dev()) for k, v in d[name].items()}


def _calibrate(net, xs, draws):
    with torch.no_grad():
        for x, d in zip(xs, draws):
            _inject(net, d)
            net(x.to(dev()))
    torch.cuda.synchronize()


def test_folding_and_it_helps():
    from bayesian_torch_amd.quantization import convert
    net, xs, draws = _prepared_fold_net(True)
    ref, _, _ = K.fold_net()
    _calibrate(net, xs, draws)
    host = K.host_stats(ref, xs, draws, True)
    coef = K.bn_coef(ref.bn1)
    st = net.conv1.calib_minmax.cpu()
    K.check_weight_rows(st, K.host_weight_rows(ref.conv1.mu_kernel, ref.conv1.rho_kernel, torch.cat([d["conv1"]["eps_w"] for d in draws]), coef), "folded conv1")
    assert torch.equal(st[5], host["conv1"][5])
    for name, row in (("conv1", 6), ("fc", 5), ("fc", 6)):          # conv1's out is the BatchNorm output's range; fc reads its ReLU
        have, want = getattr(net, name).calib_minmax.cpu()[row], host[name][row]
        rel = float(((have - want).abs() / want.abs().clamp_min(1e-30)).max()) if float(want.abs().min()) > 0 else float((have - want).abs().max())
        print(f"folded {name} row {K.ROWS[row]}: deviation {rel:.3e} (bound 1e-4)")
        assert rel <= 1e-4, (name, row, have, want)
    with torch.no_grad():          # not the conv's own output: the unfolded range differs
        y = [K.float_forward(ref, x, d)[0] for x, d in zip(xs, draws)]
    assert abs(K.aminmax(torch.cat(y))[1] - float(st[6, 1])) > 1e-3
    stats = {n: getattr(net, n).calib_minmax.cpu() for n in ("conv1", "fc")}
    bn = net.bn1
    convert(net, fuse_conv_bn=True)
    assert not bn._forward_hooks and type(net.bn1).__name__ == "Identity"
    assert net.conv1.quant_dict == K.dict_of(stats["conv1"]) and net.fc.quant_dict == K.dict_of(stats["fc"])
    # the calibrated model against the INT8 model (tests/_q8_model.py) with the same pairs, bit for bit
    dflt, _, _ = K.converted_cpu(False, True)
    dflt = dflt.to(dev())
    errs = {"calibrated": [], "default": []}
    with torch.no_grad():
        for x, d in zip(xs, draws):
            _inject(net, d), _inject(dflt, d)
            out = net(x.to(dev())).cpu()
            assert torch.equal(out, K.q8_model_forward(net, x, d))          # (the model reads the layers' int8 images, scales and calibrated pairs)
            want = K.float_forward(ref, x, d)[2]
            errs["calibrated"].append((out - want).abs().reshape(-1))
            errs["default"].append((dflt(x.to(dev())).cpu() - want).abs().reshape(-1))
    cal, dft = (float(torch.cat(errs[k]).mean()) for k in ("calibrated", "default"))
    print(f"mean |int8 - float|: calibrated {cal:.5f}, default branch {dft:.5f}")
    assert cal < dft


def test_mc_forward_observes_every_sample():
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import mc_forward
    net, xs, _ = _prepared_fold_net(True)
    rng.set_mode("philox")
    out, _ = mc_forward(net, xs[0].to(dev()), 4)
    torch.cuda.synchronize()
    assert out.shape == (4, 4, 4)
    for layer in (net.conv1, net.fc):
        last = layer._last
        assert last["observed"] and last["S"] == 4 and last["observer_kernel"] == "q8_observe_w<eps on chip>"
        eps = layer.materialize_last_draw()["eps_w"]
        assert eps.shape[0] == 4 and tuple(layer.calib_minmax[2].tolist()) == K.aminmax(eps)
        per_sample = [K.aminmax(eps[s]) for s in range(4)]
        assert len(set(per_sample)) == 4                                        # four different streams, all four inside the range
        assert int(layer.calib_nonfinite) == 0 and bool(torch.isfinite(layer.calib_minmax).all())
