"""GPU: the training path against float64 torch autograd of the CPU oracle (inputs and references: tests/_grad_cases.py).
A. the KL gradient ALONE -- kl_normal_bwd_kernel, kl_normal_bwd_segs_kernel, kl_elem_grad inside wgrad's finishing pass and the
   public routes that reach them -- over rho sweeps to +-80, per element, against the uncancelled size of the expression;
B. the backward kernels' supplied-draw branches (inject_draw, rng mode "torch"), at the smallest shapes that split the launches;
C. the two LSTM layers differentiated through time."""
import pytest
import torch

import _grad_cases as GC
from conftest import assert_close, load_golden

pytestmark = pytest.mark.gpu

ROWS = range(len(GC.KL_ROWS))


def _cuda(t):
    return None if t is None else t.cuda()


def _g():
    return torch.tensor(GC.KL_G, device="cuda")


def _hold(tag, row, t, got, ref64, g=GC.KL_G):
    """Print the kernel's and the fp32 reference's worst scaled errors, then hold the kernel to KL_FACTOR times the reference's."""
    r, lim = GC.kl_row(row), GC.kl_limits(row)
    err = GC.kl_errors(r["kind"], t["mu"], t["rho"], t["psig"], got, ref64, g)
    print(f"{tag} {GC.KL_ROW_IDS[row]} n={t['mu'].numel()}: kernel dmu {err['dmu']:.3e} drho {err['drho']:.3e} | fp32 reference dmu "
          f"{r['ref32_err']['dmu']:.3e} drho {r['ref32_err']['drho']:.3e}")
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), f"{tag}: non-finite gradient where the float64 reference is finite"
    assert err["dmu"] <= lim["dmu"], f"{tag} {GC.KL_ROW_IDS[row]}: dmu {err['dmu']:.3e} > {lim['dmu']:.3e}"
    assert err["drho"] <= lim["drho"], f"{tag} {GC.KL_ROW_IDS[row]}: drho {err['drho']:.3e} > {lim['drho']:.3e}"
    return err


# ------------------------------------------------------------------------------------------------------------ A. KL gradient alone
@pytest.mark.parametrize("row", ROWS, ids=GC.KL_ROW_IDS)
def test_kl_backward_kernel_matches_fp64_autograd(row):
    """functional.kl_backward (bt_kl_normal_bwd) on the whole 4001-element row."""
    from bayesian_torch_amd import functional as F
    r = GC.kl_row(row)
    t = r["inputs"]
    got = F.kl_backward(_cuda(t["mu"]), _cuda(t["rho"]), _cuda(t["pmu"]), _cuda(t["psig"]), _g(), laplace=r["kind"] == "laplace")
    _hold("kl_backward", row, t, got, r["ref64"])


@pytest.mark.parametrize("row", ROWS, ids=GC.KL_ROW_IDS)
def test_kl_backward_segs_matches_fp64_autograd_and_the_single_tensor_kernel(row):
    """functional.kl_backward_segs on 70 segments (two launches: 64 + 6) at odd element offsets of one buffer, lengths around the
    1024-element blocks and the 256 threads: every segment against ITS mean's float64 gradient (g / numel(segment)), and bit for
    bit against bt_kl_normal_bwd on the same elements."""
    from bayesian_torch_amd import functional as F
    r = GC.kl_row(row)
    lap = r["kind"] == "laplace"
    segs = GC.kl_segments()
    v = {k: GC.odd_offset_views(_cuda(r["inputs"][k]), segs) for k in ("mu", "rho", "pmu", "psig")}
    out = F.kl_backward_segs(list(zip(v["mu"], v["rho"], v["pmu"], v["psig"])), _g(), laplace=lap)
    assert len(out) == len(segs)
    worst = dict(dmu=0.0, drho=0.0)
    for i, ((s, n), got) in enumerate(zip(segs, out)):
        assert got[0].shape == (n,) and got[1].shape == (n,)
        t, ref = GC.kl_slice_ref(row, s, n)
        r32, lim = GC.kl_row(row)["ref32_err"], GC.kl_limits(row)
        err = GC.kl_errors(r["kind"], t["mu"], t["rho"], t["psig"], got, ref)
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), (i, s, n)
        assert err["dmu"] <= lim["dmu"] and err["drho"] <= lim["drho"], f"segment {i} [{s}, {s + n}): {err} > {lim} (fp32 reference {r32})"
        worst = {k: max(worst[k], err[k]) for k in worst}
        one = F.kl_backward(v["mu"][i], v["rho"][i], v["pmu"][i], v["psig"][i], _g(), laplace=lap)
        assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]), f"segment {i} [{s}, {s + n}): bits differ from bt_kl_normal_bwd"
    print(f"kl_backward_segs {GC.KL_ROW_IDS[row]} 70 segments: kernel dmu {worst['dmu']:.3e} drho {worst['drho']:.3e} | fp32 reference dmu "
          f"{r32['dmu']:.3e} drho {r32['drho']:.3e}")


FUSED_GEOMS = {
    "24x16x3x3": dict(w=(24, 16, 3, 3), x=(2, 16, 6, 6), conv=dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1)),
    "20x6x3x2 groups=2": dict(w=(20, 6, 3, 2), x=(2, 12, 6, 6), conv=dict(stride=(1, 1), padding=(1, 0), dilation=(1, 1), groups=2)),      # Cig4 = 8 != Cig = 6
}


@pytest.mark.parametrize("geom", list(FUSED_GEOMS))
@pytest.mark.parametrize("row", ROWS, ids=GC.KL_ROW_IDS)
def test_kl_inside_wgrad_finish_matches_fp64_autograd_and_the_other_two_kernels(row, geom):
    """functional.fused_backward(kl=...) with grad_out = 0: the contraction partials are exact zeros, so dmu / drho are
    kl_elem_grad's of wgrad_finish_body alone (natural element <- tap-major partial, Cig4 padding).  Same bits as bt_kl_normal_bwd
    and as a segment of bt_kl_normal_bwd_segs on the same elements -- what the comment above kl_elem_grad promises."""
    from bayesian_torch_amd import functional as F
    r, gm = GC.kl_row(row), FUSED_GEOMS[geom]
    lap = r["kind"] == "laplace"
    n = 1
    for d in gm["w"]:
        n *= d
    t, ref = GC.kl_slice_ref(row, 0, n)
    c = {k: _cuda(a).reshape(gm["w"]) for k, a in t.items()}
    x = torch.randn(gm["x"], generator=torch.Generator().manual_seed(5)).cuda()
    Ho, Wo = F.conv_out_hw(gm["x"][2], gm["x"][3], gm["w"][2], gm["w"][3], *gm["conv"]["stride"], *gm["conv"]["padding"], *gm["conv"]["dilation"])
    gout = torch.zeros(gm["x"][0], gm["w"][0], Ho, Wo, device="cuda")
    dx, dmu, drho = F.fused_backward(x, gout, c["mu"], c["rho"], F.pack_params(c["mu"], c["rho"]), conv=gm["conv"], S=1, seed=7, call=3, layer_id=2,
                                     kl=(_g(), c["pmu"], c["psig"], r["kind"]))
    assert dmu.shape == gm["w"] and not dx.any()
    _hold("fused_backward(kl) " + geom, row, t, (dmu, drho), ref)
    flat = {k: a.reshape(-1) for k, a in c.items()}
    one = F.kl_backward(flat["mu"], flat["rho"], flat["pmu"], flat["psig"], _g(), laplace=lap)
    assert torch.equal(dmu.reshape(-1), one[0]) and torch.equal(drho.reshape(-1), one[1]), "wgrad's finishing pass and bt_kl_normal_bwd differ in bits"
    short = (flat["mu"][:5], flat["rho"][:5], flat["pmu"][:5], flat["psig"][:5])
    seg = F.kl_backward_segs([short, (flat["mu"], flat["rho"], flat["pmu"], flat["psig"])], _g(), laplace=lap)[1]
    assert torch.equal(dmu.reshape(-1), seg[0]) and torch.equal(drho.reshape(-1), seg[1]), "wgrad's finishing pass and bt_kl_normal_bwd_segs differ in bits"


def _spread(layer, row):
    """Set a layer's parameters and per-element priors to elements of row ``row``, every tensor spread over the WHOLE rho range
    -> [(the four attribute names, the row indices taken)] for the weight and the bias."""
    t = GC.kl_row(row)["inputs"]
    used = []
    wn = layer._wname
    groups = [("mu_" + wn, "rho_" + wn, "prior_weight_mu", "prior_weight_sigma")]
    if layer.mu_bias is not None:
        groups.append(("mu_bias", "rho_bias", "prior_bias_mu", "prior_bias_sigma"))
    with torch.no_grad():
        for names in groups:
            p = getattr(layer, names[0])
            n = p.numel()
            idx = (torch.arange(n) * (GC.KL_N - 1)) // (n - 1)
            for nm, k in zip(names, ("mu", "rho", "pmu", "psig")):
                getattr(layer, nm).copy_(t[k][idx].reshape(p.shape))
            used.append((names, idx))
    return used


def _hold_layer(tag, row, layer, used):
    """Each parameter tensor of a layer against the float64 autograd of O.kl_layer_ref: the KL is a sum of per-tensor means, so a
    tensor's gradient is that of ITS mean, upstream 1."""
    from oracle import bt_oracle as O
    t = GC.kl_row(row)["inputs"]
    leaves = []
    for names, idx in used:
        leaves += [t["mu"][idx].double().requires_grad_(True), t["rho"][idx].double().requires_grad_(True), t["pmu"][idx].double(), t["psig"][idx].double()]
    O.kl_layer_ref(*leaves).backward()
    for j, (names, idx) in enumerate(used):
        got = (getattr(layer, names[0]).grad, getattr(layer, names[1]).grad)
        assert got[0] is not None and got[1] is not None, names
        _hold(f"{tag}.{names[0]}", row, {k: a[idx] for k, a in t.items()}, got, (leaves[4 * j].grad, leaves[4 * j + 1].grad), g=1.0)


@pytest.mark.parametrize("row", [0, 1], ids=GC.KL_ROW_IDS[:2])
def test_public_kl_routes_match_fp64_autograd(row):
    """layer.train(); layer.kl_loss().backward() on a LinearReparameterization and a Conv2dFlipout with bias, and
    get_kl_loss(model).backward() on a converted MLP, parameters and priors spread over the row."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn, get_kl_loss
    for tag, layer in (("LinearReparameterization", L.LinearReparameterization(64, 48)), ("Conv2dFlipout", L.Conv2dFlipout(8, 12, 3))):
        layer = layer.cuda()
        used = _spread(layer, row)
        layer.train()
        layer.kl_loss().backward()
        _hold_layer(tag + ".kl_loss", row, layer, used)
    net = H.mlp((32, 64, 4))
    dnn_to_bnn(net, {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization",
                     "moped_enable": False, "moped_delta": 0.5})
    net = net.cuda().train()
    per_layer = [(m, _spread(m, row)) for _, m in H.bayes_layers(net)]
    get_kl_loss(net).backward()
    for i, (m, used) in enumerate(per_layer):
        _hold_layer(f"get_kl_loss.layer{i}", row, m, used)


@pytest.mark.parametrize("row", [0, 2], ids=[GC.KL_ROW_IDS[0], GC.KL_ROW_IDS[2]])
def test_aten_checker_of_the_kl_gradient_matches_fp64_autograd(row):
    """autograd._kl_grads_aten on the device: what "HIP equals the checker" elsewhere in the suite rests on."""
    from bayesian_torch_amd.autograd import _kl_grads_aten
    r = GC.kl_row(row)
    t = r["inputs"]
    got = _kl_grads_aten(_cuda(t["mu"]), _cuda(t["rho"]), _cuda(t["pmu"]), _cuda(t["psig"]), _g(), r["kind"])
    _hold("_kl_grads_aten", row, t, got, r["ref64"])


# ------------------------------------------------------------------------------------------------------------ B. supplied draws
def _layer_and_input(row_id, stacked):
    import bayesian_torch_amd.layers as L
    _, cls, ctor, xshape, S = GC.DRAW_ROW[row_id]
    torch.manual_seed(3)
    layer = getattr(L, cls)(**ctor).cuda().train()
    x0 = torch.randn(((S if stacked else 1) * xshape[0],) + tuple(xshape[1:])).cuda()
    return layer, x0, S, xshape[0]


def _params(layer):
    wn = layer._wname
    return dict(mu_w=getattr(layer, "mu_" + wn), rho_w=getattr(layer, "rho_" + wn), mu_b=layer.mu_bias, rho_b=layer.rho_bias)


def _step(layer, x0, S, B, gout=None, deferred=False):
    """One forward + backward of L = (out * gout).sum() -> (out, gout, [dx, dmu_w, drho_w, dmu_b, drho_b])."""
    from bayesian_torch_amd import mc
    for p in layer.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    if S > 1 or deferred:
        with mc.mc_samples(S, B) as ctx:
            if deferred:
                ctx.train_fused, ctx.deferred = True, []
            out = layer(x, return_kl=False)
    else:
        ctx, out = None, layer(x, return_kl=False)
    if gout is None:
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).cuda()
    (out * gout).sum().backward()
    if deferred:
        assert len(ctx.deferred) == 1      # the weight gradients went through the side stream
        mc.finish_deferred(ctx)
        layer._kl_live = None
    torch.cuda.synchronize()
    return out.detach(), gout, [x.grad] + [None if p is None else p.grad for p in _params(layer).values()]


def _hold_to_oracle(tag, layer, x0, S, shared, draws, out, gout, grads):
    conv = layer._conv_desc() if layer._kind == "conv" else None
    o_ref, gx_ref, gp_ref = GC.oracle_grads(layer._flip, _params(layer), x0, draws, conv, gout, S, shared)
    assert_close(out, o_ref, 1e-4, 1e-5, tag + " out")
    assert_close(grads[0], gx_ref, 1e-4, 1e-5, tag + " dL/dx")
    for g, (k, ref) in zip(grads[1:], gp_ref.items()):
        assert (g is None) == (ref is None), (tag, k)
        if ref is not None:
            assert_close(g, ref, 2e-4, 2e-5, f"{tag} dL/d{k}")


GRAD_NAMES = ("dx", "dmu_w", "drho_w", "dmu_b", "drho_b")


def _same_bits(tag, a, b):
    for nm, u, v in zip(GRAD_NAMES, a, b):
        assert (u is None) == (v is None), (tag, nm)
        if u is not None:
            assert torch.equal(u, v), f"{tag}: {nm} differs, max abs {float((u - v).abs().max()):.3e} at {int((u != v).sum())} of {u.numel()} elements"


# (one sample: shared and stacked x are the same launch)
DRAW_CASES = [(r[0], st) for r in GC.DRAW_ROWS for st in (False, True) if not (st and r[4] == 1)]


@pytest.mark.parametrize("row_id,stacked", DRAW_CASES, ids=[f"{r}-{'stacked' if st else 'shared'} x" for r, st in DRAW_CASES])
def test_backward_on_supplied_draws_equals_on_chip_draws_and_fp64_autograd(row_id, stacked):
    """dgrad_body / wgrad_body and FusedForward.backward reading eps_w, eps_b, sign_in, sign_out: the draws an on-chip step made,
    handed back through inject_draw, give the same gradient bits (both branches hand identical values to identical code; padded
    channels multiply a zero sigma), and those gradients match float64 autograd of the oracle on the same draws."""
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    rng.manual_seed(11)
    layer, x0, S, B = _layer_and_input(row_id, stacked)
    out1, gout, g1 = _step(layer, x0, S, B)
    draws = layer.materialize_last_draw()
    assert draws["eps_w"].shape[0] == S and (not layer._flip or draws["sign_in"].shape[:2] == (S, B))
    layer.inject_draw = draws
    out2, _, g2 = _step(layer, x0, S, B, gout)
    assert layer._last["draw"] is not None
    _same_bits(f"row {row_id}: supplied vs on-chip draws", g2, g1)
    _hold_to_oracle(f"row {row_id} (inject_draw)", layer, x0, S, not stacked, draws, out2, gout, g2)


@pytest.mark.parametrize("row_id", ["A", "C", "D"])
def test_backward_in_torch_draw_mode_matches_fp64_autograd(row_id):
    """rng.set_mode("torch"): the draws come from torch's generator in the reference's order and the backward reads them."""
    from bayesian_torch_amd import rng
    layer, x0, S, B = _layer_and_input(row_id, False)
    rng.set_mode("torch")
    try:
        torch.manual_seed(23)
        out, gout, grads = _step(layer, x0, S, B)
        draws = layer.materialize_last_draw()
    finally:
        rng.set_mode("philox")
    assert layer._last["draw"] is not None and draws["eps_w"].shape[0] == S
    _hold_to_oracle(f"row {row_id} (torch mode)", layer, x0, S, True, draws, out, gout, grads)


@pytest.mark.parametrize("row_id", ["A", "C"])
def test_deferred_wgrad_on_supplied_draws_equals_the_paired_launch(row_id):
    """mc.finish_deferred (ctx.deferred): wgrad and dgrad as launches of their own, the weight gradients on the side stream -- the
    same bits as the one paired launch, on supplied draws."""
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    rng.manual_seed(11)
    layer, x0, S, B = _layer_and_input(row_id, False)
    with torch.no_grad(), mc.mc_samples(S, B):
        layer(x0, return_kl=False)
    layer.inject_draw = layer.materialize_last_draw()
    _, gout, paired = _step(layer, x0, S, B)
    assert layer._last["draw"] is not None
    _, _, split = _step(layer, x0, S, B, gout, deferred=True)
    assert layer._last["draw"] is not None      # both steps read the supplied draw
    _same_bits(f"row {row_id}: deferred vs paired", split, paired)


@pytest.mark.parametrize("row_id", ["A", "C"])
def test_unpaired_launches_equal_the_paired_launch(row_id):
    """bt_debug_bwd_pair(0): dgrad, its finishing pass, wgrad and its finishing pass as four launches instead of two -- the same
    bodies, block decode and finishing order, so the same bits (A: two reduction chunks, three dgrad pieces; C: Flipout, stride 2,
    groups 2).  Both steps read the same supplied draws."""
    import ctypes as C
    from bayesian_torch_amd import _lib, mc, rng
    hooks = C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
    rng.set_mode("philox")
    rng.manual_seed(11)
    layer, x0, S, B = _layer_and_input(row_id, False)
    with torch.no_grad(), mc.mc_samples(S, B):
        layer(x0, return_kl=False)
    layer.inject_draw = layer.materialize_last_draw()
    try:
        hooks.bt_debug_bwd_pair(1)
        _, gout, paired = _step(layer, x0, S, B)
        hooks.bt_debug_bwd_pair(0)
        _, _, unpaired = _step(layer, x0, S, B, gout)
    finally:
        hooks.bt_debug_bwd_pair(1)
    assert all(g is not None for g in paired[:3])
    _same_bits(f"row {row_id}: unpaired vs paired", unpaired, paired)


# ------------------------------------------------------------------------------------------------------------ C. LSTM through time
@pytest.mark.parametrize("name", ["lstm_reparam_7x5", "lstm_flipout_7x5"])
def test_lstm_gradients_through_time_match_fp64_autograd(name):
    """Two fused Linear launches per step, a draw of its own per call, the same parameters collecting gradients from every step:
    dx and the eight parameter gradients of L = (hidden_seq * g1).sum() + (c_ts * g2).sum() against float64 autograd of O.lstm_ref
    on the stored per-step draws."""
    import bayesian_torch_amd.layers as L
    g = load_golden(name)
    lstm = (L.LSTMFlipout if "flipout" in name else L.LSTMReparameterization)(7, 5).cuda()
    with torch.no_grad():
        for nm in ("ih", "hh"):
            lin = getattr(lstm, nm)
            lin.mu_weight.copy_(g[nm + "_mu_w"]), lin.rho_weight.copy_(g[nm + "_rho_w"]), lin.mu_bias.copy_(g[nm + "_mu_b"]), lin.rho_bias.copy_(g[nm + "_rho_b"])
            lin.inject_draw = GC.lstm_inject_lists(g, nm, "cuda")
    lstm.train()
    x = g["x"].cuda().requires_grad_()
    hs, (_, cs), _ = lstm(x)
    g1, g2 = GC.lstm_upstream(hs.shape)
    ((hs * g1.cuda()).sum() + (cs * g2.cuda()).sum()).backward()
    assert lstm.ih.inject_draw == [] and lstm.hh.inject_draw == []      # every step consumed its own draw
    hr, cr, xr, pr = GC.lstm_ref_run(name, torch.float64)
    ((hr * g1).sum() + (cr * g2).sum()).backward()
    assert_close(hs, hr, 1e-4, 1e-5, name + " hidden_seq")
    assert_close(cs, cr, 1e-4, 1e-5, name + " c_ts")
    assert_close(x.grad, xr.grad, 1e-4, 1e-5, name + " dL/dx")
    for nm in ("ih", "hh"):
        lin = getattr(lstm, nm)
        for k, p in (("mu_w", lin.mu_weight), ("rho_w", lin.rho_weight), ("mu_b", lin.mu_bias), ("rho_b", lin.rho_bias)):
            assert_close(p.grad, pr[f"{nm}_{k}"].grad, 2e-4, 2e-5, f"{name} dL/d{nm}.{k}")
