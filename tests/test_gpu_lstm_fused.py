"""GPU: the LSTM cell kernels (csrc/bt_lstm.hip) and the two LSTM layers under ``set_lstm_path("fused")``.
1. the cell kernels alone against float64 of the torch gate arithmetic and its autograd (tests/_lstm_cases.py), inside guard bands;
2. the reference goldens with per-step draws under "fused";  3. gradients through time under "fused";
4. MC batching on both paths, both classes;  5. a converted model through mc_forward and McGraph;  6. eager training.
Cell-kernel figures (this file's test 1 prints them; DESIGN.md 4.6c holds a run's table): max |got - ref64| / (1 + |ref64|) per output,
held to FACTOR = 8 x the same measure of CPU torch's float32 evaluation."""
import pytest
import torch

import _grad_cases as GC
import _guard as G
import _lstm_cases as LC
from conftest import assert_close, load_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5      # test_gpu_layers.py's, for the goldens
PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization",
         "moped_enable": False, "moped_delta": 0.5}


def _cuda(t):
    return None if t is None else t.cuda()


@pytest.fixture()
def lstm_path():
    """set_lstm_path for the duration of a test -> the setter."""
    import bayesian_torch_amd.layers as BL
    before = BL.get_lstm_path()
    try:
        yield BL.set_lstm_path
    finally:
        BL.set_lstm_path(before)


# ------------------------------------------------------------------------------------------------ 1. the cell kernels alone
def _run_cell(t, off=0):
    """Forward (saving the gates) and backward of row inputs ``t`` with every result inside guard bands; operands ``off`` fp32 elements
    past a 16-byte boundary -> (dict h, c, act, dz, dc_prev; the two launches' kernel names)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    H, rows = t["H"], t["rows"]
    put = lambda v: None if v is None else G.place(v.cuda(), off)
    a, b, cp, gh, gc = (put(t[k]) for k in ("a", "b", "c_prev", "grad_h", "grad_c"))
    slab = t["special"] == "slab"
    if slab:      # slab t = 1 of a [4, 3, 64] sequence buffer: row stride 192
        hb, cb = (G.place_result((rows, 3, H), off, device="cuda", tag=n) for n in ("h slab", "c slab"))
        h_out, c_out = hb.view[:, 1, :], cb.view[:, 1, :]
        assert h_out.stride(0) == 3 * H
    else:
        hb, cb = (G.place_result((rows, H), off, device="cuda", tag=n) for n in ("h", "c"))
        h_out, c_out = hb.view, cb.view
    with G.guarded_allocations(off) as log:
        h, c, act = F.lstm_cell_fwd(a, b, cp, h_out=h_out, c_out=c_out, want_act=True)
        k_fwd = _lib.lib().bt_last_kernel_name().decode()
        dz, dcp = F.lstm_cell_bwd(act, cp, c, gh, gc)
        k_bwd = _lib.lib().bt_last_kernel_name().decode()
    torch.cuda.synchronize()
    assert h.data_ptr() == h_out.data_ptr() and c.data_ptr() == c_out.data_ptr() and len(log) == 3
    G.check_all(log)                       # act, dz, dc_prev: bands intact, every element written
    for buf in (hb, cb):
        G.check(buf, body=not slab)
        if slab:                           # the written slab holds no pattern word, the other time slabs of every row still hold it
            words = buf.words[buf.start:buf.start + buf.n_words].view(rows, 3, H)
            pat = G._i32(G.PATTERN)
            assert bool((words[:, 1] != pat).all()) and bool((words[:, 0] == pat).all()) and bool((words[:, 2] == pat).all())
    return dict(h=h.clone(), c=c.clone(), act=act, dz=dz, dc_prev=dcp), (k_fwd, k_bwd)


@pytest.mark.parametrize("row", range(len(LC.CELL_ROWS)), ids=LC.CELL_IDS)
def test_cell_kernels_match_fp64_gate_arithmetic(row):
    from bayesian_torch_amd import functional as F
    r = LC.cell_row(row)
    t = r["inputs"]
    H = t["H"]
    got, names = _run_cell(t)
    form = "vec4" if H % 4 == 0 else "elem"
    assert names == ("lstm_cell_fwd_kernel<%s,act=1>" % form, "lstm_cell_bwd_kernel<%s>" % form)
    err = {k: LC.metric(got[k], r["ref64"][k]) for k in LC.OUTPUTS}
    for k in LC.OUTPUTS:
        print(f"cell {LC.CELL_IDS[row]:>14} {k:>7}: fp32 reference {r['ref32_err'][k]:.2e}  limit {r['limit'][k]:.2e}  kernel {err[k]:.2e}")
    for k in LC.OUTPUTS + ("act",):
        assert torch.isfinite(got[k]).all(), f"{k}: non-finite where the float64 reference is finite"
    if t["special"] == "pm90":      # saturated gates land on the limits, exactly
        act = got["act"].cpu()
        assert torch.equal(act[0], torch.ones(4 * H))
        assert torch.equal(act[1], torch.cat([torch.zeros(2 * H), -torch.ones(H), torch.zeros(H)]))
        assert torch.equal(got["dz"][:2].cpu(), torch.zeros(2, 4 * H))
    for k in LC.OUTPUTS:
        assert err[k] <= r["limit"][k], f"{LC.CELL_IDS[row]} {k}: {err[k]:.3e} > {r['limit'][k]:.3e}"
    # the inference launch (no act) gives the same bits
    h2, c2, none = F.lstm_cell_fwd(_cuda(t["a"]), _cuda(t["b"]), _cuda(t["c_prev"]))
    assert none is None and torch.equal(h2, got["h"].reshape(h2.shape)) and torch.equal(c2, got["c"].reshape(c2.shape))
    # operands 4 bytes off a 16-byte boundary: the element-wise form, the same values
    got1, names1 = _run_cell(t, off=1)
    assert names1 == ("lstm_cell_fwd_kernel<elem,act=1>", "lstm_cell_bwd_kernel<elem>")
    for k in LC.OUTPUTS + ("act",):
        assert torch.equal(got1[k], got[k]), k


# ------------------------------------------------------------------------------------------------ 2. goldens under "fused"
def _golden_lstm(name):
    import bayesian_torch_amd.layers as L
    g = load_golden(name)
    lstm = (L.LSTMFlipout if "flipout" in name else L.LSTMReparameterization)(7, 5).cuda()
    with torch.no_grad():
        for nm in ("ih", "hh"):
            lin = getattr(lstm, nm)
            lin.mu_weight.copy_(g[nm + "_mu_w"]), lin.rho_weight.copy_(g[nm + "_rho_w"]), lin.mu_bias.copy_(g[nm + "_mu_b"]), lin.rho_bias.copy_(g[nm + "_rho_b"])
            lin.inject_draw = GC.lstm_inject_lists(g, nm, "cuda")
    return g, lstm


@pytest.mark.parametrize("name", ["lstm_reparam_7x5", "lstm_flipout_7x5"])
def test_goldens_under_fused(name, lstm_path):
    lstm_path("fused")
    g, lstm = _golden_lstm(name)
    with torch.no_grad():
        hs, (h2, cs), kl = lstm(g["x"].cuda())
        assert h2 is hs
        assert_close(hs.cpu(), g["hidden_seq"], RTOL, ATOL, "hidden_seq")
        assert_close(cs.cpu(), g["c_ts"], RTOL, ATOL, "c_ts")
        assert_close(kl.cpu(), g["kl"], 1e-5, 0, "kl")
        assert_close(lstm.kl_loss().cpu(), g["kl_loss"], 1e-5, 0, "kl_loss")
    assert lstm.ih.inject_draw == [] and lstm.hh.inject_draw == []      # every step consumed its own draw
    assert hs.is_contiguous() and cs.is_contiguous() and tuple(hs.shape) == tuple(g["hidden_seq"].shape)


# ------------------------------------------------------------------------------------------------ 3. gradients through time
@pytest.mark.parametrize("impl", ["hip", "aten"])
@pytest.mark.parametrize("name", ["lstm_reparam_7x5", "lstm_flipout_7x5"])
def test_gradients_through_time_under_fused(name, impl, lstm_path):
    """test_gpu_grad_oracle.py's LSTM test with the cell on its kernels (and, "aten", the cell's and the Linear launches' ATen checkers)."""
    from bayesian_torch_amd import autograd
    lstm_path("fused")
    g, lstm = _golden_lstm(name)
    lstm.train()
    x = g["x"].cuda().requires_grad_()
    before, autograd.BACKWARD_IMPL = autograd.BACKWARD_IMPL, impl
    try:
        hs, (_, cs), kl = lstm(x)
        g1, g2 = GC.lstm_upstream(hs.shape)
        ((hs * g1.cuda()).sum() + (cs * g2.cuda()).sum()).backward()
    finally:
        autograd.BACKWARD_IMPL = before
    assert lstm.ih.inject_draw == [] and lstm.hh.inject_draw == []
    assert_close(kl.detach().cpu(), g["kl"], 1e-5, 0, "kl")
    hr, cr, xr, pr = GC.lstm_ref_run(name, torch.float64)
    ((hr * g1).sum() + (cr * g2).sum()).backward()
    assert_close(hs, hr, 1e-4, 1e-5, name + " hidden_seq")
    assert_close(cs, cr, 1e-4, 1e-5, name + " c_ts")
    assert_close(x.grad, xr.grad, 1e-4, 1e-5, name + " dL/dx")
    for nm in ("ih", "hh"):
        lin = getattr(lstm, nm)
        for k, p in (("mu_w", lin.mu_weight), ("rho_w", lin.rho_weight), ("mu_b", lin.mu_bias), ("rho_b", lin.rho_bias)):
            assert_close(p.grad, pr[f"{nm}_{k}"].grad, 2e-4, 2e-5, f"{name} dL/d{nm}.{k}")


# ------------------------------------------------------------------------------------------------ 4. MC batching
S, B, T, NIN, HID = 3, 3, 4, 7, 5


def _mc_layer(cls):
    import bayesian_torch_amd.layers as L
    torch.manual_seed(11)
    return LC.spread_rho(getattr(L, cls)(NIN, HID)).cuda()


def _mc_run(lstm, x, call0, hidden=None, hooks=True):
    """One forward inside mc_samples(S, B) at call coordinate ``call0`` -> (hidden_seq, c_ts, per-call draws of ih / hh, step 0's a)."""
    from bayesian_torch_amd import mc, rng
    draws, first_a, handles = {"ih": [], "hh": []}, [], []
    if hooks:
        for nm in ("ih", "hh"):
            handles.append(getattr(lstm, nm).register_forward_hook(lambda m, i, o, nm=nm: draws[nm].append(m.materialize_last_draw())))
        handles.append(lstm.ih.register_forward_hook(lambda m, i, o: first_a.append((o[0] if isinstance(o, tuple) else o).clone())))
    rng.set_call(call0)
    try:
        with torch.no_grad(), mc.mc_samples(S, B):
            hs, (_, cs), _ = lstm(x, hidden)
    finally:
        for h in handles:
            h.remove()
    assert rng.peek_call() == call0 + 2 * T      # every step and every map drew once
    return hs, cs, draws, (first_a[0] if first_a else None)


def _oracle_sample(lstm, x_s, draws, s):
    """float64 O.lstm_ref of sample s on its own draws."""
    from oracle import bt_oracle as O
    flip = "Flipout" in type(lstm).__name__
    d64 = lambda v: v.detach().double().cpu()

    def step(nm):
        lin = getattr(lstm, nm)

        def f(t, v):
            d = draws[nm][t]
            w = (d64(lin.mu_weight), d64(lin.rho_weight), d64(d["eps_w"][s]))
            bb = (d64(lin.mu_bias), d64(lin.rho_bias), d64(d["eps_b"][s]))
            if flip:
                return O.flipout_fwd_ref(v.double(), *w, d64(d["sign_in"][s]), d64(d["sign_out"][s]), *bb)
            return O.reparam_fwd_ref(v.double(), *w, *bb)
        return f
    return O.lstm_ref(d64(x_s), step("ih"), step("hh"), HID)


@pytest.mark.parametrize("stacked", [False, True], ids=["shared-x", "stacked-x"])
@pytest.mark.parametrize("path", ["torch", "fused"])
@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_mc_batched_lstm_matches_the_oracle_per_sample(cls, path, stacked, lstm_path):
    from bayesian_torch_amd import rng
    lstm_path(path)
    rng.set_mode("philox")
    rng.manual_seed(31)
    lstm = _mc_layer(cls)
    x = LC.mc_x(S, B, T, NIN, stacked).cuda()
    hs, cs, draws, _ = _mc_run(lstm, x, 40)
    assert tuple(hs.shape) == tuple(cs.shape) == (S * B, T, HID) and len(draws["ih"]) == len(draws["hh"]) == T
    for s in range(S):
        x_s = x[s * B:(s + 1) * B] if stacked else x
        hr, cr = _oracle_sample(lstm, x_s, draws, s)
        assert_close(hs[s * B:(s + 1) * B], hr, 1e-4, 1e-5, f"{cls} {path} sample {s} hidden_seq")
        assert_close(cs[s * B:(s + 1) * B], cr, 1e-4, 1e-5, f"{cls} {path} sample {s} c_ts")
    assert not torch.equal(hs[:B], hs[B:2 * B]) or stacked      # (shared x: the samples differ by their draws alone)


@pytest.mark.parametrize("path", ["torch", "fused"])
@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_mc_batched_lstm_initial_states(cls, path, lstm_path):
    """A supplied state of B rows is shared by the samples, one of S * B rows is per sample; both give what the other gives when the
    per-sample one repeats the shared one. Any other row count is refused by name."""
    from bayesian_torch_amd import mc, rng
    lstm_path(path)
    rng.set_mode("philox")
    rng.manual_seed(32)
    lstm = _mc_layer(cls)
    x = LC.mc_x(S, B, T, NIN, False).cuda()
    gen = torch.Generator().manual_seed(9)
    h0, c0 = torch.randn(B, HID, generator=gen).cuda(), torch.randn(B, HID, generator=gen).cuda()
    zero = torch.zeros(B, HID, device="cuda")
    d_hs, d_cs, _, _ = _mc_run(lstm, x, 50, hooks=False)
    z_hs, z_cs, _, _ = _mc_run(lstm, x, 50, hidden=(zero, zero), hooks=False)
    assert torch.equal(d_hs, z_hs) and torch.equal(d_cs, z_cs)
    s_hs, s_cs, _, _ = _mc_run(lstm, x, 50, hidden=(h0, c0), hooks=False)
    p_hs, p_cs, _, _ = _mc_run(lstm, x, 50, hidden=(h0.repeat(S, 1), c0.repeat(S, 1)), hooks=False)
    assert not torch.equal(s_hs, d_hs)
    assert_close(p_hs, s_hs, 1e-5, 1e-6, "per-sample vs shared state: hidden_seq")
    assert_close(p_cs, s_cs, 1e-5, 1e-6, "per-sample vs shared state: c_ts")
    m_hs, _, _, _ = _mc_run(lstm, x, 50, hidden=(h0, c0.repeat(S, 1)), hooks=False)      # mixed: h shared, c per sample
    assert_close(m_hs, s_hs, 1e-5, 1e-6, "mixed state")
    bad = torch.zeros(B + 1, HID, device="cuda")
    c_before = rng.peek_call()
    with pytest.raises(RuntimeError, match=r"hidden_states h must be \[3, 5\] or \[9, 5\], got \(4, 5\)"):
        with torch.no_grad(), mc.mc_samples(S, B):
            lstm(x, (bad, bad))
    assert rng.peek_call() == c_before      # a refused call consumed no draw


@pytest.mark.parametrize("stacked", [False, True], ids=["shared-x", "stacked-x"])
@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_fused_against_torch_path_at_the_same_call_coordinates(cls, stacked, lstm_path):
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    rng.manual_seed(33)
    lstm = _mc_layer(cls)
    x = LC.mc_x(S, B, T, NIN, stacked).cuda()
    lstm_path("torch")
    t_hs, t_cs, _, t_a = _mc_run(lstm, x, 60)
    lstm_path("fused")
    f_hs, f_cs, _, f_a = _mc_run(lstm, x, 60)
    assert torch.equal(t_a, f_a)      # step 0's input-to-hidden launch is the same launch
    assert_close(f_hs, t_hs, 0, 1e-5, "hidden_seq fused vs torch")      # within 1e-5 * max: the transcendentals differ
    assert_close(f_cs, t_cs, 0, 1e-5, "c_ts fused vs torch")


# ------------------------------------------------------------------------------------------------ 5. a converted model
def _model(seed=2):
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(seed)
    net = LC.LSTMHead(NIN, HID, 3)
    dnn_to_bnn(net, PRIOR)
    LC.spread_rho(net.lstm)
    return net.cuda().eval()


@pytest.mark.parametrize("path", ["torch", "fused"])
def test_converted_model_mc_forward_and_graph(path, lstm_path):
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import McGraph, mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    lstm_path(path)
    rng.set_mode("philox")
    rng.manual_seed(34)
    net = _model()
    assert isinstance(net.lstm, L.LSTMReparameterization) and net.lstm.dnn_to_bnn_flag
    Bm = 6
    x = LC.mc_x(1, Bm, T, NIN, False).cuda()
    logits, kl = mc_forward(net, x, 4)
    assert tuple(logits.shape) == (4, Bm, 3) and torch.isfinite(logits).all()
    with torch.no_grad():
        assert_close(kl.cpu(), get_kl_loss(net).cpu(), 1e-5, 0, "mc_forward kl vs get_kl_loss")
    g = McGraph(net, x, 4)
    assert g.calls_per_run == 2 * T + 1
    seen = []
    for _ in range(2):
        c = rng.peek_call()
        l, gkl, _ = g.replay()
        l, gkl = l.clone(), gkl.clone()
        assert rng.peek_call() == c + 2 * T + 1
        rng.set_call(c)
        e, ekl = mc_forward(net, x, 4)      # eager at the same coordinates
        assert torch.equal(e, l)
        assert_close(gkl.cpu(), ekl.cpu(), 1e-6, 0, "graph kl")
        seen.append(l)
    assert not torch.equal(seen[0], seen[1])


# ------------------------------------------------------------------------------------------------ 6. eager training
def test_eager_training_under_fused(lstm_path):
    """Three SGD steps reduce the loss (measured on the first step's draws), and one step moves the parameters where the "torch" path
    moves them: the two paths differ by the cell's transcendentals alone (1e-7 relative in h, c and their gradients), far inside 1e-4."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    rng.set_mode("philox")
    rng.manual_seed(35)
    Bm = 16
    x = LC.mc_x(1, Bm, T, NIN, False, seed=6).cuda()
    y = (x[:, :, 0].sum(1) > 0).long()
    nets = {p: _model(seed=4).train() for p in ("torch", "fused")}

    def loss_at(net, call):
        rng.set_call(call)
        return torch.nn.functional.cross_entropy(net(x), y) + get_kl_loss(net) / 1000.0

    after_one = {}
    for path, net in nets.items():
        lstm_path(path)
        opt = torch.optim.SGD(net.parameters(), lr=0.5)
        losses = []
        for step in range(3):
            opt.zero_grad()
            loss = loss_at(net, 100 + 20 * step)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            if step == 0:
                after_one[path] = [p.detach().clone() for p in net.parameters()]
        with torch.no_grad():
            final = float(loss_at(net, 100))
        print(f"{path}: losses {losses}, on step 0's draws after three steps {final:.6f}")
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
        assert final < losses[0], (path, losses, final)
    for (n, _), pf, pt in zip(nets["fused"].named_parameters(), after_one["fused"], after_one["torch"]):
        assert_close(pf, pt, 1e-4, 1e-5, f"{n} after one SGD step, fused vs torch")
