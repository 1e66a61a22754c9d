"""GPU: the draws the forward kernels consume, held to the distribution the layers define (tests/_draw_stats.py).

Every other GPU test here replays the kernel's own draws (rng_fill_*, materialize_last_draw share philox_block, box_muller, hash_sign and
the stream keys with the kernels) or supplies draws from outside: a draw shared by two weight elements, a bias draw equal to a weight
draw, a sign index without the batch coordinate, a sample that reuses its neighbour's stream or a truncated coordinate word all pass
them, because fill and kernel move together.  Here nothing is replayed.  The impulse probe reads the standardised draws back out of
functional.fused_forward's output, one weight element per output element, and the dense form holds mean and full covariance of up to
512 outputs of a launch against the float64 analytic moments; every statistic is in standard errors and the bound is 7.0
(_draw_stats: the reasoning; test_draw_stats_host.py: the reference arithmetic on the same inputs stays inside it, seeded faults do
not).  S = 1024 per row, as eight launches of 128 samples at sample0 = 0, 128, ... of one call (the streamed K = 512 row: 256)."""
import math

import pytest
import torch

import _draw_stats as DS
from conftest import assert_close

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(autouse=True)
def _restore_switches():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import _lib, rng
    mode, p3, pt = _lib.lib().bt_get_contraction(), L.get_conv3d_path(), L.get_transpose_path()
    rng.set_mode("philox")
    yield
    _lib.lib().bt_set_contraction(mode)
    L.set_conv3d_path(p3)
    L.set_transpose_path(pt)


def _show(tag, st):
    print(f"\n{tag}: worst {DS.worst(st):.2f}  " + "  ".join(f"{k} {v:.3g}" for k, v in st.items()))


# ------------------------------------------------------------------------------------------------------------- functional rows
class _Launcher:
    """A row's launches of functional.fused_forward at explicit coordinates, parameters on the device once."""

    def __init__(self, rid, form):
        from bayesian_torch_amd import functional as F
        self.rid, self.row, self.p = rid, DS.ROWS[rid], DS.parameters(rid, form)
        dev = _dev()
        self.t = {k: self.p[k].to(dev) for k in ("mu_w", "rho_w", "mu_b", "rho_b")}
        self.packed = F.pack_params(self.t["mu_w"], self.t["rho_w"]) if self.row["packs"] else None
        self.names = set()

    def __call__(self, x, sample0, bias=True, call=DS.CALL, layer_id=DS.LAYER):
        """-> one chunk's output [CHUNK, rows * Co * Ho * Wo] on the device."""
        from bayesian_torch_amd import _lib
        from bayesian_torch_amd import functional as F
        L, row, t = _lib.lib(), self.row, self.t
        _lib.check(L.bt_set_contraction(row["mode"]))
        try:
            r = F.fused_forward(x, t["mu_w"], t["rho_w"], t["mu_b"] if bias else None, t["rho_b"] if bias else None, flip=row["flip"], conv=DS.conv_desc(row),
                                S=DS.CHUNK, shared_x=True, packed=self.packed, seed=DS.SEED, call=call, layer_id=layer_id, sample0=sample0)
            assert r is not None, "the library declined the launch"
            self.names.add(L.bt_last_kernel_name().decode().replace(",walk", ""))      # (the stem's sample walk is planned from the CU count)
        finally:
            L.bt_set_contraction(0)
        return r[0].reshape(DS.CHUNK, -1)

    def check_name(self):
        assert self.names == {DS.PINS[self.rid][0]}, (self.rid, self.names, DS.PINS[self.rid][0])


def gpu_probe(rid, call=DS.CALL, layer_id=DS.LAYER, S_total=None):
    """The standardised draws the row's kernel consumed at (SEED, call, layer_id) -> (E [S, K + Co], E2 or None)."""
    row, pr = DS.ROWS[rid], DS.probe(rid)
    run = _Launcher(rid, "probe")
    xs = [x.to(_dev()) for x in pr["xs"]]
    Es, E2s = [], []
    for c in range((S_total or row["S_total"]) // DS.CHUNK):
        s0 = c * DS.CHUNK
        outs = [run(x, s0, bias=not row["flip"], call=call, layer_id=layer_id).cpu() for x in xs]
        bias_out = run(torch.zeros_like(xs[0]), s0, call=call, layer_id=layer_id).cpu() if row["flip"] else None
        E, E2 = DS.probe_draws(rid, run.p, outs, bias_out)
        Es.append(E)
        E2s.append(E2)
    run.check_name()
    return torch.cat(Es), (torch.cat(E2s) if row["flip"] else None)


PROBE_ROWS = [rid for rid, r in DS.ROWS.items() if "probe" in r["forms"]]
DENSE_ROWS = [rid for rid, r in DS.ROWS.items() if "dense" in r["forms"]]


@pytest.mark.parametrize("rid", PROBE_ROWS)
def test_probe_row(rid):
    E, E2 = gpu_probe(rid)
    assert bool(torch.isfinite(E).all())
    st = DS.probe_stats(E, DS.shapes(DS.ROWS[rid])[1][0], E2)
    _show(f"{rid} probe S={E.shape[0]} {DS.PINS[rid][0]}", st)
    assert DS.worst(st) < DS.BOUND, (rid, st)
    if E2 is not None:
        assert st["abs_gap"] <= DS.ABS_GAP, (rid, st)


@pytest.mark.parametrize("rid", DENSE_ROWS)
def test_dense_row(rid):
    row = DS.ROWS[rid]
    x, p, sel, mean, Cv, Q = DS.dense_case(rid)
    run = _Launcher(rid, "dense")
    xd, seld = x.to(_dev()), sel.to(_dev())
    Y = torch.cat([run(xd, c * DS.CHUNK)[:, seld].double().cpu() for c in range(row["S_total"] // DS.CHUNK)])
    run.check_name()
    st = DS.dense_stats(Y, mean, Cv, Q)
    _show(f"{rid} dense S={Y.shape[0]} N={sel.numel()} {DS.PINS[rid][0]}", st)
    assert DS.worst(st) < DS.BOUND, (rid, st)      # (Flipout: Cv is diagonal, so ``cov`` held every entry between examples, pixels and channels to zero)


# ------------------------------------------------------------------------------------------------------------- coordinates
def test_streams_of_neighbouring_coordinates_are_independent():
    """The one-pixel probe row at (call, layer) against (call + 1, layer) and (call, layer + 1): the cross-correlation of matching
    columns.  Tensor 0 against tensor 1 is the bias columns' correlation with the weight columns inside test_probe_row's ``corr``.
    layer_id 5 + 2^28: layer_tensor_word keeps 28 bits of the layer id (include/bt_hip.h: layer_id < 2^28), so the launch draws layer 5's
    own streams again, bit for bit -- the id wraps and does not spill into the tensor field, which would hand the wrapped layer's
    weights the bias stream (tensor 1) of layer 5.  The equality is the whole check: whatever test_probe_row holds for layer 5 (its
    weight columns against its bias columns among it) then holds for the wrapped id."""
    rid = "g_xm1"
    E0, _ = gpu_probe(rid)
    Ec, _ = gpu_probe(rid, call=DS.CALL + 1)
    El, _ = gpu_probe(rid, layer_id=DS.LAYER + 1)
    Ew, _ = gpu_probe(rid, layer_id=DS.LAYER + (1 << 28))
    st = dict(call=DS.cross_stat(E0, Ec), layer=DS.cross_stat(E0, El), call_layer=DS.cross_stat(Ec, El))
    _show(f"{rid} coordinates S={E0.shape[0]}", st)
    assert DS.worst(st) < DS.BOUND, st
    assert torch.equal(Ew, E0), "layer_id 5 + 2^28 no longer draws layer 5's streams: state what it does instead"
    Co = DS.shapes(DS.ROWS[rid])[1][0]
    for E in (Ec, El):
        assert DS.worst(DS.probe_stats(E, Co)) < DS.BOUND


def test_an_eager_call_and_a_graph_replay_at_the_next_call_word_draw_independently():
    """The one-pixel probe row as a converted one-layer model (Conv2d 8 -> 32, 1 x 1, on the row's impulse input and parameters), S = 1024
    in one call: an eager mc_forward, then McGraph replays, each at the next call word, then an eager call again."""
    from bayesian_torch_amd import mc, rng
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    rid, S = "g_xm1", 1024
    row, g, p, pr = DS.ROWS[rid], DS.geometry(DS.ROWS[rid]), DS.parameters(rid, "probe"), DS.probe(rid)
    assert len(pr["xs"]) == 1
    net = torch.nn.Sequential(torch.nn.Conv2d(g["Ci"], g["Co"], g["k"]))
    dnn_to_bnn(net, dict(_PRI, type="Reparameterization"))
    net = net.cuda().eval()
    with torch.no_grad():
        for name, key in (("mu_kernel", "mu_w"), ("rho_kernel", "rho_w"), ("mu_bias", "mu_b"), ("rho_bias", "rho_b")):
            getattr(net[0], name).copy_(p[key])
    rng.manual_seed(31)
    x = pr["xs"][0].to(_dev())
    draws = lambda out: DS.probe_draws(rid, p, [out.reshape(S, -1).cpu()])[0]
    Ee = draws(mc.mc_forward(net, x, S)[0])
    kernel = net[0]._last["kernel"]
    assert kernel.startswith("fused_split_kernel<") and kernel.endswith("xm=1>"), kernel
    gr = mc.McGraph(net, x, S, epilogue=False)
    c = rng.peek_call()
    Er = draws(gr.replay()[0])
    assert rng.peek_call() == c + 1
    Er2 = draws(gr.replay()[0])
    Ea = draws(mc.mc_forward(net, x, S)[0])
    st = dict(eager_replay=DS.cross_stat(Ee, Er), replay_replay=DS.cross_stat(Er, Er2), replay_eager=DS.cross_stat(Er2, Ea))
    for tag, E in (("eager", Ee), ("replay", Er), ("replay2", Er2)):
        st[tag] = DS.worst(DS.probe_stats(E, g["Co"]))
    _show(f"{rid} as a model, eager / McGraph replay S={S} {kernel}", st)
    assert DS.worst(st) < DS.BOUND, st


def _identity_probe(n):
    """[n + 1, n]: example i holds a 1 at feature i, the last example is zero."""
    return torch.cat([torch.eye(n), torch.zeros(1, n)]).to(_dev())


def _linear_draws(layer, out, S):
    """out [S, n + 1, Co] of a Linear layer on the identity probe -> E [S, Co * In + Co] (Reparameterization, or Flipout whose bias
    perturbation was switched off: sigma_b = 0)."""
    mu, rho = layer.mu_weight.detach().double().cpu(), layer.rho_weight.detach().double().cpu()
    mb, rb = layer.mu_bias.detach().double().cpu(), layer.rho_bias.detach().double().cpu()
    o = out.double().cpu()
    zero = o[:, -1:, :]                                           # [S, 1, Co]: mu_b + sigma_b * eps_b
    ew = (o[:, :-1, :] - zero).transpose(1, 2) - mu              # [S, Co, In]: sigma * eps
    ew = ew / torch.log1p(torch.exp(rho))
    if layer._flip:
        return ew.reshape(S, -1)
    eb = (zero[:, 0, :] - mb) / torch.log1p(torch.exp(rb))
    return torch.cat([ew.reshape(S, -1), eb], 1)


_PRI = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "moped_enable": False, "moped_delta": 0.5}


def _deep(kind, n_layers=70, width=16, seed=11):
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(seed)
    net = torch.nn.Sequential(*[torch.nn.Linear(width, width) for _ in range(n_layers)])
    dnn_to_bnn(net, dict(_PRI, type=kind))
    return net.cuda().eval()


# ------------------------------------------------------------------------------------------------------------- layer-API rows
LAYER_CASES = [(r[0], path) for r in DS.LAYER_ROWS for path in ({"convt": ("upsample", "native"), "conv3d": ("unfold", "native")}.get(r[4]) or ("default",))]


@pytest.mark.parametrize("rid,path", LAYER_CASES, ids=[f"{r}-{p}" for r, p in LAYER_CASES])
def test_layer_row_dense(rid, path):
    """The layer classes through mc.mc_samples, S = 1024 as eight calls of 128 samples: mean and covariance of up to 512 outputs against
    the analytic moments of the layer's own float64 reference (oracle.bt_oracle._contract in the reference's layout).  The Flipout
    classes: zero covariance between the two examples, under the default path and under the native one, whose input signs are drawn
    over different tensors."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    cls, switch = next((r[1], r[4]) for r in DS.LAYER_ROWS if r[0] == rid)
    if switch == "convt":
        L.set_transpose_path(path)
    elif switch == "conv3d":
        L.set_conv3d_path(path)
    layer, x, _, _, sel, moments, oshape = DS.layer_case(rid)
    xshape = tuple(x.shape)
    layer, xd, seld = layer.cuda().eval(), x.cuda(), sel.cuda()
    rng.manual_seed(77)
    Ys, kernels, paths = [], set(), set()
    with torch.no_grad():
        for c in range(1024 // DS.CHUNK):
            with mc.mc_samples(DS.CHUNK, xshape[0], sample0=c * DS.CHUNK):
                out = layer(xd, return_kl=False)
            assert tuple(out.shape) == (DS.CHUNK * oshape[0],) + oshape[1:]
            Ys.append(out.reshape(DS.CHUNK, -1)[:, seld].double().cpu())
            kernels.add(layer._last["kernel"].replace(",walk", ""))
            paths.add(layer._last.get("x_path"))
    if path == "native":
        assert paths == {"native"}, (rid, paths, kernels)
    st = DS.dense_stats(torch.cat(Ys), *moments)
    _show(f"{rid} {cls} path={path} S=1024 N={sel.numel()} {sorted(kernels)}", st)
    assert DS.worst(st) < DS.BOUND, (rid, path, st)


# ------------------------------------------------------------------------------------------------------------- more than 64 layers
def _kl_refs(net):
    from oracle import bt_oracle as O
    t = lambda v: v.detach().double().cpu()
    return [float(O.kl_layer_ref(t(m.mu_weight), t(m.rho_weight), t(m.prior_weight_mu), t(m.prior_weight_sigma), t(m.mu_bias), t(m.rho_bias),
                                 t(m.prior_bias_mu), t(m.prior_bias_sigma))) for m in net]


def _count_pack_launches(monkeypatch):
    from bayesian_torch_amd import functional as F
    calls, real = [], F._pack_sync_launch

    def counted(arr, karr, owner, dev):
        calls.append((len(arr), karr is not None))
        return real(arr, karr, owner, dev)

    monkeypatch.setattr(F, "_pack_sync_launch", counted)
    return calls


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_seventy_layers_pack_check_in_chunks_with_the_kl_of_every_layer(kind, monkeypatch):
    """70 layers: the model's pack check takes the first layer in the launch stream and the other 69 on the side stream, in chunks of
    at most 64 -- 1, 64 and 5 segments, every one with its KL entries: the chunked loop of functional.pack_sync, never run by a smaller
    model.  Every layer's KL term and the sum against the float64 oracle at 1e-5, eagerly and from a McGraph replay."""
    from bayesian_torch_amd import mc, rng
    rng.manual_seed(3)
    net = _deep(kind)
    assert [m._layer_id for m in net] == list(range(1, 71))
    refs = _kl_refs(net)
    x = torch.randn(5, 16, generator=torch.Generator().manual_seed(1)).cuda()
    calls = _count_pack_launches(monkeypatch)
    out, kl = mc.mc_forward(net, x, 4)
    assert calls == [(1, True), (64, True), (5, True)], calls
    assert out.shape == (4, 5, 16) and bool(torch.isfinite(out).all())
    assert abs(float(kl) - sum(refs)) <= 1e-5 * abs(sum(refs)), (float(kl), sum(refs))
    with torch.no_grad(), mc.mc_samples(4, 5, collect_kl=True) as ctx:
        mc.sync_model_packs(net, ctx)
        net(x)
        mc.join_packs(ctx)
    assert len(ctx.kls) == 70
    for i, (got, ref) in enumerate(zip(ctx.kls, refs)):
        assert abs(float(got) - ref) <= 1e-5 * abs(ref), (kind, i, float(got), ref)
    del calls[:]
    g = mc.McGraph(net, x, 4)
    assert calls == [(1, True), (64, True), (5, True)] * 3, calls      # two warm-up runs and the capture
    _, gkl, _ = g.replay()
    assert abs(float(gkl) - sum(refs)) <= 1e-5 * abs(sum(refs)), (float(gkl), sum(refs))


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_seventy_layers_kl_loss_value_and_gradient(kind):
    """get_kl_loss over 140 segments (the chunked loop of _lib.kl_normal: 64 + 64 + 12) without grad, and under grad with its backward
    (kl_backward_segs) against float64 autograd at _grad_cases' limits, parameters and priors spread over its row 0."""
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    from test_gpu_grad_oracle import _hold_layer, _spread
    net = _deep(kind)
    refs = _kl_refs(net)
    with torch.no_grad():
        kl0 = get_kl_loss(net)
    assert abs(float(kl0) - sum(refs)) <= 1e-5 * abs(sum(refs)), (float(kl0), sum(refs))
    net.train()
    kl = get_kl_loss(net)
    assert kl.requires_grad and abs(float(kl.detach()) - sum(refs)) <= 1e-5 * abs(sum(refs)), (float(kl.detach()), sum(refs))
    per_layer = [(m, _spread(m, 0)) for m in net]      # every tensor over the whole rho range of _grad_cases' row 0
    kl = get_kl_loss(net)
    kl.backward()
    for i, (m, used) in enumerate(per_layer):
        _hold_layer(f"get_kl_loss.layer{i}", 0, m, used)


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_seventy_layers_rebuild_exactly_the_packs_whose_parameters_changed(kind):
    from bayesian_torch_amd import mc, rng
    from oracle import bt_oracle as O
    rng.manual_seed(9)
    net = _deep(kind)
    x = torch.randn(5, 16, generator=torch.Generator().manual_seed(2)).cuda()
    mc.mc_forward(net, x, 4)
    before = [m.pack_rebuilds() for m in net]
    assert all(b >= 1 for b in before)
    mc.mc_forward(net, x, 4)
    assert [m.pack_rebuilds() for m in net] == before
    with torch.no_grad():
        net[3].mu_weight.data.mul_(1.5)
        net[67].rho_weight.data.add_(0.75)
    out, kl = mc.mc_forward(net, x, 4)
    after = [m.pack_rebuilds() for m in net]
    assert [a - b for a, b in zip(after, before)] == [1 if i in (3, 67) else 0 for i in range(70)]
    refs = _kl_refs(net)
    assert abs(float(kl) - sum(refs)) <= 1e-5 * abs(sum(refs))
    # that forward against the float64 reference chain on the draws the layers report
    t = lambda v: v.detach().double().cpu()
    draws = [m.materialize_last_draw() for m in net]
    hs = [t(x)] * 4
    for m, d in zip(net, draws):
        par = (t(m.mu_weight), t(m.rho_weight))
        bias = (t(m.mu_bias), t(m.rho_bias))
        if kind == "Flipout":
            hs = [O.flipout_fwd_ref(h, *par, t(d["eps_w"][s]), t(d["sign_in"][s]), t(d["sign_out"][s]), *bias, t(d["eps_b"][s])) for s, h in enumerate(hs)]
        else:
            hs = [O.reparam_fwd_ref(h, *par, t(d["eps_w"][s]), *bias, t(d["eps_b"][s])) for s, h in enumerate(hs)]
    assert_close(out.cpu(), torch.stack(hs), 1e-4, 1e-5, "70-layer forward after two in-place writes")
    for i in (3, 67):
        m = net[i]
        assert torch.equal(m._pack[1].reshape(16, -1)[:, :16], m.mu_weight.detach())
        assert_close(m._pack[2].reshape(16, -1)[:, :16].cpu(), torch.log1p(torch.exp(m.rho_weight.detach().double().cpu())), 1e-6, 1e-7, "sigma pack")


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_seventy_layers_draw_pairwise_uncorrelated_streams(kind):
    """Every layer alone on one identity probe inside a single mc_samples context per chunk of 128 samples, the call word set back
    before each layer so that the 70 launches differ in the layer id ALONE (1 ... 70: past 64): the recovered draws of the layers,
    column by column, pairwise uncorrelated.  Flipout (bias perturbation switched off, sigma_b ~ 1e-13, to keep an output one draw):
    s_out * s_in * eps hides a shared eps from the correlation, |e| mapped back to N(0,1) does not."""
    from bayesian_torch_amd import mc, rng
    rng.manual_seed(123)
    net, S = _deep(kind), 1024
    if kind == "Flipout":
        with torch.no_grad():
            for m in net:
                m.rho_bias.fill_(-30.0)
    x = _identity_probe(16)
    c0 = rng.peek_call()
    chunks = []
    with torch.no_grad():
        for c in range(S // DS.CHUNK):
            with mc.mc_samples(DS.CHUNK, 17, sample0=c * DS.CHUNK):
                outs = []
                for m in net:
                    rng.set_call(c0)
                    outs.append(m(x).reshape(DS.CHUNK, 17, 16))
                    assert m._last["rng"].call == c0 and m._last["rng"].sample0 == c * DS.CHUNK
            chunks.append(torch.stack([_linear_draws(m, o, DS.CHUNK) for m, o in zip(net, outs)]))
    E = torch.cat(chunks, 1)                                       # [70, S, columns]
    assert bool(torch.isfinite(E).all())

    def pairwise(V):
        Cm = torch.einsum("lsj,msj->lmj", V, V) / S
        Cm[torch.arange(70), torch.arange(70)] = 0
        return float(Cm.abs().max()) * math.sqrt(S)

    st = dict(layers=pairwise(E), mean=float(E.mean(1).abs().max()) * math.sqrt(S), var=float(((E * E).mean(1) - 1).abs().max()) / math.sqrt(2.0 / S))
    if kind == "Flipout":
        st["layers_abs"] = pairwise(math.sqrt(2.0) * torch.special.erfinv((2 * torch.special.erf(E.abs() / math.sqrt(2.0)) - 1).clamp(-1 + 1e-15, 1 - 1e-15)))
    _show(f"70 x Linear{kind}(16, 16), layer ids 1..70 at one call, S={S}, {E.shape[2]} columns", st)
    assert DS.worst(st) < DS.BOUND, st
