"""GPU: grouped and depthwise convolutions on every kernel path (rows and inputs: tests/_group_cases.py).

Every launch with at most four input channels per group runs the stem ("quad") kernel whatever ``groups`` is, so that kernel is the
depthwise path: its group-dependent indices (the x offset and channel mask, the weight row and row mask, the pack offset, the Philox
block, the hashed sign indices, the per-channel output stage) are held here to the fp64 oracle at ``groups`` up to 70, next to the
general split kernel at 8 groups of one octet and the fp32 kernels.  Every test asserts the kernel it is there to reach against the
table (tests/test_grouped_plan_host.py holds the same table to the host dispatch without a GPU).

A forward vs the C oracle + the (K + 8) * 2^-24 bound   B launch-split independence   C injected draws   D fused output stage
F guard bands   G backward vs fp64 autograd   H Conv1d / ConvTranspose2d / Conv3d   I a converted model   J a grouped fuzz
(E, the bf16 mode, is rows dw3 and cog70 of tests/test_gpu_bf16_mode.py.)"""
import copy
import ctypes as C
import random

import pytest
import torch

import _grad_cases as GRC
import _group_cases as GC
import _guard as G
from conftest import assert_close

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
SEED, CALL, LAYER, SAMPLE0 = 77, 2, 9, 5
PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "moped_enable": False, "moped_delta": 0.5}
FLIP_IDS = ["reparam", "flipout"]


@pytest.fixture(autouse=True)
def _restore_switches():
    import bayesian_torch_amd.autograd as AG
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import _lib, rng
    rng.seed()
    saved = {k: getattr(rng._state, k, None) for k in ("seed", "pinned", "call")}
    paths = L.get_transpose_path(), L.get_conv3d_path()
    yield
    for k, v in saved.items():
        setattr(rng._state, k, v)
    rng.set_inject_path("general")
    rng.set_mode("philox")
    AG.BACKWARD_IMPL = "hip"
    L.set_transpose_path(paths[0]), L.set_conv3d_path(paths[1])
    C.CDLL(_lib.LIB_PATH).bt_debug_bwd_pair(1)
    _lib.lib().bt_set_contraction(0)


# ----------------------------------------------------------------------------------------------------------------- launches
_DEV, _PACKS, _DRAWS, _REFS = {}, {}, {}, {}


def _c(t):
    """One device copy per host tensor (GC.inputs builds a row's tensors once)."""
    if t is None:
        return None
    k = id(t)
    if k not in _DEV or _DEV[k][0] is not t:
        _DEV[k] = (t, t.cuda())
    return _DEV[k][1]


def _packed(t):
    from bayesian_torch_amd import functional as F
    k = id(t["mu"])
    if k not in _PACKS:
        _PACKS[k] = F.pack_params(_c(t["mu"]), _c(t["rho"]))
    return _PACKS[k]


def _launch(t, flip, S, shared, mode=0, sample0=SAMPLE0, x=None, **kw):
    """One forward of the row's tensors ``t`` over x[:B] (shared) or x[:S * B] (stacked) -> (out, kernel name)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    L = _lib.lib()
    if x is None:
        x = _c(t["x"])[:t["B"] if shared else S * t["B"]]
    _lib.check(L.bt_set_contraction(mode))
    try:
        out, _ = F.fused_forward(x, _c(t["mu"]), _c(t["rho"]), _c(t["mb"]), _c(t["rb"]), flip=flip, conv=t["conv"], S=S, shared_x=shared,
                                 seed=SEED, call=CALL, layer_id=LAYER, sample0=sample0, packed=_packed(t), **kw)
        name = L.bt_last_kernel_name().decode()
    finally:
        L.bt_set_contraction(0)
    return out, name


def _draws(rid, flip, S=3, sample0=SAMPLE0):
    """The on-chip draws of the launches above, replayed on the host: eps_w, eps_b[, sign_in, sign_out], each [S, ...]."""
    key = (rid, flip, S, sample0)
    if key not in _DRAWS:
        from bayesian_torch_amd import functional as F
        r, dev = GC.ROWS[rid], torch.device("cuda")
        Ho, Wo = GC.out_hw(r)
        wshape = (r["Co"], r["Ci"] // r["groups"]) + r["k"]
        d = dict(eps_w=F.rng_fill_normal(SEED, CALL, LAYER, sample0, 0, S, wshape, dev).cpu(),
                 eps_b=F.rng_fill_normal(SEED, CALL, LAYER, sample0, 1, S, (r["Co"],), dev).cpu())
        if flip:
            d["sign_in"] = F.rng_fill_sign(SEED, CALL, LAYER, sample0, 2, S, (r["B"], r["Ci"], r["H"], r["W"]), dev).cpu()
            d["sign_out"] = F.rng_fill_sign(SEED, CALL, LAYER, sample0, 3, S, (r["B"], r["Co"], Ho, Wo), dev).cpu()
        _DRAWS[key] = d
    return _DRAWS[key]


def _ref(rid, flip, shared, s):
    """Sample s of the row over the shared x[:B] or its own batch of the stacked x -> (C oracle: fp32 element-wise steps, fp64
    accumulation; the fp64 oracle; the magnitude conv(|x|, |W_s|) + |b_s|).  Computed once, shared, never modified."""
    key = (rid, flip, shared or s == 0, s)      # (the first stacked batch IS the shared one)
    if key not in _REFS:
        from oracle import c_oracle as CO
        t, d, B = GC.inputs(rid), _draws(rid, flip), GC.ROWS[rid]["B"]
        xs = t["x"][:B] if shared else t["x"][s * B:(s + 1) * B]
        if flip:
            cref = CO.flipout_fwd(xs, t["mu"], t["rho"], d["eps_w"][s], d["sign_in"][s], d["sign_out"][s], t["mb"], t["rb"], d["eps_b"][s], t["conv"])
        else:
            cref = CO.reparam_fwd(xs, t["mu"], t["rho"], d["eps_w"][s], t["mb"], t["rb"], d["eps_b"][s], t["conv"])
        _REFS[key] = (cref, GC.oracle64(flip, t, xs, d, s), GC.oracle64(flip, t, xs, d, s, absolute=True))
    return _REFS[key]


def _want(rid, flip, name, mode=0):
    want = GC.want_family(rid, flip, mode)
    assert GC.family(name) == want, f"{rid} {'flipout' if flip else 'reparam'} mode {mode}: ran {name}, the table says {want}"
    return want


# ----------------------------------------------------------------------------------------------------------------- A. forward
@pytest.mark.parametrize("flip", [False, True], ids=FLIP_IDS)
@pytest.mark.parametrize("rid", list(GC.ROWS))
def test_forward_on_chip_draws_vs_c_oracle(rid, flip):
    """S = 1 and S = 3, shared and stacked x, automatic and f32 mode on the same draws: the C oracle at the project's tolerance, and
    on the bf16x3 kernels |out - ref64| <= (K + 8) * 2^-24 * (conv(|x|, |W_s|) + |b_s|) per element, K = Cig * kh * kw: K for the fp32
    accumulation, 3 for the dropped piece products, 5 for forming W_s, sigma and the bias in fp32.  A lost low piece or a
    lost product term is 2^-16 of the magnitude."""
    t, r = GC.inputs(rid), GC.ROWS[rid]
    B, K = r["B"], GC.k_len(r)
    worst, over = 0.0, []
    for S in (1, 3):
        for shared in (True, False):
            out, name = _launch(t, flip, S, shared)
            want = _want(rid, flip, name)
            out32, name32 = _launch(t, flip, S, shared, mode=1)
            _want(rid, flip, name32, 1)
            o, o32 = out.reshape((S, B) + tuple(out.shape[1:])).cpu(), out32.reshape((S, B) + tuple(out.shape[1:])).cpu()
            for s in range(S):
                cref, ref64, mag = _ref(rid, flip, shared, s)
                tag = f"{rid} {FLIP_IDS[flip]} S={S} {'shared' if shared else 'stacked'} x, sample {s}"
                assert_close(o[s], cref, RTOL, ATOL, f"{tag}: {name} vs C oracle")
                assert_close(o32[s], cref, RTOL, ATOL, f"{tag}: {name32} vs C oracle")
                if want in GC.SPLIT_FAMILIES:
                    frac = float(((o[s].double() - ref64).abs() / ((K + 8) * 2.0 ** -24 * mag)).max())
                    worst = max(worst, frac)
                    if not frac <= 1.0:
                        over.append((tag, frac))
    if GC.want_family(rid, flip) in GC.SPLIT_FAMILIES:
        print(f"{rid} {FLIP_IDS[flip]} ({name}): worst |out - ref64| = {worst:.3f} of the (K + 8) * 2^-24 bound, K = {K}")
    assert not over, over


# ----------------------------------------------------------------------------------------------------------------- B. launch split
SPLIT_ROWS = [(rid, flip) for rid in ("dw3", "cig4", "oct-g8", "cog70") for flip in (False, True) if GC.want_family(rid, flip) in GC.SPLIT_FAMILIES]


@pytest.mark.parametrize("rid,flip", SPLIT_ROWS, ids=[f"{r}-{FLIP_IDS[f]}" for r, f in SPLIT_ROWS])
def test_launch_split_independence(rid, flip):
    """The same global samples in one launch of four or in two launches of two, over a shared x or the same x stacked: the same bits."""
    t = GC.inputs(rid, 4)
    B = t["B"]
    xs = _c(t["x"])
    full, name = _launch(t, flip, 4, True)
    _want(rid, flip, name)
    a, na = _launch(t, flip, 2, True)
    b, nb = _launch(t, flip, 2, True, sample0=SAMPLE0 + 2)
    _want(rid, flip, na), _want(rid, flip, nb)
    assert torch.equal(torch.cat([a, b]), full)
    stacked, ns = _launch(t, flip, 4, False, x=xs[:B].repeat(4, 1, 1, 1))
    _want(rid, flip, ns)
    assert torch.equal(stacked, full)
    # four batches of their own, in one launch and in two
    full, _ = _launch(t, flip, 4, False)
    a, _ = _launch(t, flip, 2, False, x=xs[:2 * B])
    b, _ = _launch(t, flip, 2, False, x=xs[2 * B:], sample0=SAMPLE0 + 2)
    assert torch.equal(torch.cat([a, b]), full)


# ----------------------------------------------------------------------------------------------------------------- C. injected draws
INJ_ROWS = [(rid, False) for rid in ("dw3", "dwx2s2", "cig4", "cog70", "oct-g8")] + [(rid, True) for rid in ("dw3", "cig2k5", "oct-g8")]


@pytest.mark.parametrize("shared", [True, False], ids=["shared-x", "stacked-x"])
@pytest.mark.parametrize("rid,flip", INJ_ROWS, ids=[f"{r}-{FLIP_IDS[f]}" for r, f in INJ_ROWS])
def test_injected_draws_reach_the_twin_and_reproduce_the_on_chip_launch(rid, flip, shared):
    """A replayed on-chip draw on the path "split" runs the ``,inj>`` twin and gives the on-chip launch's bits (the criterion of
    test_gpu_inject_split.py); through the general path it matches the oracle at the forward tolerance."""
    t, S, B = GC.inputs(rid), 3, GC.ROWS[rid]["B"]
    out0, k0 = _launch(t, flip, S, shared)
    assert _want(rid, flip, k0) in GC.SPLIT_FAMILIES and k0.endswith(">")
    kw = {k: _c(v) for k, v in _draws(rid, flip).items()}
    out1, k1 = _launch(t, flip, S, shared, inject_path="split", eps_pack_state={}, **kw)
    assert k1 == k0[:-1] + ",inj>", (k0, k1)
    assert torch.equal(out1, out0), f"{rid}: {k1} differs from {k0} at {int((out1 != out0).sum())} of {out0.numel()} elements"
    out2, k2 = _launch(t, flip, S, shared, inject_path="general", **kw)
    assert "split" not in k2 and "inj=1" in k2, k2
    o2 = out2.reshape((S, B) + tuple(out2.shape[1:])).cpu()
    for s in range(S):
        assert_close(o2[s], _ref(rid, flip, shared, s)[0], RTOL, ATOL, f"{rid} general path sample {s} ({k2})")


# ----------------------------------------------------------------------------------------------------------------- D. output stage
@pytest.mark.parametrize("residual", [False, True], ids=["bn-relu", "bn-residual-relu"])
@pytest.mark.parametrize("flip", [False, True], ids=FLIP_IDS)
@pytest.mark.parametrize("rid", ["dw3", "cig4", "cog70", "oct-g8"])
def test_fused_output_stage(rid, flip, residual):
    """Folded BatchNorm scale / shift (a third of the scales negative, a shift of its own per channel) [+ residual] + ReLU behind the
    contraction == the same stage applied in fp64 to the oracle's output."""
    t, S, B = GC.inputs(rid), 3, GC.ROWS[rid]["B"]
    kw = dict(post_scale=_c(t["sc"]), post_shift=_c(t["sh"]), relu=True)
    if residual:
        kw["residual"] = _c(t["res"])
    out, name = _launch(t, flip, S, False, **kw)
    _want(rid, flip, name)
    o = out.reshape((S, B) + tuple(out.shape[1:])).cpu()
    assert (o >= 0).all() and (o == 0).any() and (o > 0).any()
    sc, sh = t["sc"].double().view(1, -1, 1, 1), t["sh"].double().view(1, -1, 1, 1)
    for s in range(S):
        ref = _ref(rid, flip, False, s)[1] * sc + sh
        if residual:
            ref = ref + t["res"][s * B:(s + 1) * B].double()
        assert_close(o[s], torch.relu(ref), RTOL, ATOL, f"{rid} {FLIP_IDS[flip]} sample {s} ({name})")


# ----------------------------------------------------------------------------------------------------------------- F. guard bands
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("flip", [False, True], ids=FLIP_IDS)
@pytest.mark.parametrize("rid", GC.GUARD_ROWS)
def test_guard_bands(rid, flip, off):
    """x, the parameters and the result as interior views of NaN- / pattern-banded buffers, ``off`` fp32 elements past a 16-byte
    boundary: nothing written outside the result, every element of it written, no read outside an operand that is used.  At off 1
    no vector access is left and the fp32 fast kernel takes the launch (the host test plans the same)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    t, r, S = GC.inputs(rid), GC.ROWS[rid], 3
    B = r["B"]
    base, name0 = _launch(t, flip, S, True)
    _want(rid, flip, name0)
    dev = torch.device("cuda", torch.cuda.current_device())
    x, mu, rho, mb, rb = (G.place(_c(v).contiguous(), off) for v in (t["x"][:B], t["mu"], t["rho"], t["mb"], t["rb"]))
    geom = _lib.bt_conv2d_geom(B, r["Ci"], r["H"], r["W"], r["Co"], *r["k"], *r["st"], *r["pd"], *r["dl"], r["groups"])
    scratch = int(_lib.lib().bt_fused_scratch_bytes(C.byref(geom), S))
    packed = _packed(t)
    with G.seated_workspace("functional", dev, scratch) as ws, G.guarded_allocations(off) as log:
        out, _ = F.fused_forward(x, mu, rho, mb, rb, flip=flip, conv=t["conv"], S=S, shared_x=True, seed=SEED, call=CALL, layer_id=LAYER,
                                 sample0=SAMPLE0, packed=packed)
        name = _lib.lib().bt_last_kernel_name().decode()
        torch.cuda.synchronize()
        assert any(g.view.data_ptr() == out.data_ptr() for g in log) and out.data_ptr() % 16 == 4 * off
        G.check_all(log)
        assert _lib._ws[("functional", dev.index)] is ws.view
        G.check_workspace(ws)
    assert GC.family(name) == (GC.want_family(rid, flip) if off == 0 else GC.GUARD_OFF1), (rid, flip, off, name)
    assert torch.isfinite(out).all()
    if name == name0:
        assert torch.equal(out, base), f"{rid} @{off}: {name} differs from the unguarded launch"
    else:
        assert off == 1
        assert_close(out.cpu(), base.cpu(), RTOL, ATOL, f"{rid} @{off}: {name} vs the unguarded {name0}")
    o = out.reshape((S, B) + tuple(out.shape[1:])).cpu()
    for s in range(S):
        assert_close(o[s], _ref(rid, flip, True, s)[0], RTOL, ATOL, f"{rid} @{off} sample {s} ({name}) vs C oracle")


# ----------------------------------------------------------------------------------------------------------------- G. backward
GRAD_ROWS = ("dw3", "dwx2s2", "cig4", "cig2k5", "cig3rect", "oct-g8", "dw70")


def _layer(rid, flip):
    """The row as a drop-in layer with the row's parameters, in training mode."""
    import bayesian_torch_amd.layers as L
    r, t = GC.ROWS[rid], GC.inputs(rid)
    kw = dict(in_channels=r["Ci"], out_channels=r["Co"], kernel_size=r["k"], stride=r["st"], padding=r["pd"], dilation=r["dl"], groups=r["groups"], bias=True)
    if not flip:
        kw["prior_type"] = "normal"
    layer = (L.Conv2dFlipout if flip else L.Conv2dReparameterization)(**kw)
    with torch.no_grad():
        layer.mu_kernel.copy_(t["mu"]), layer.rho_kernel.copy_(t["rho"]), layer.mu_bias.copy_(t["mb"]), layer.rho_bias.copy_(t["rb"])
    return layer.cuda().train()


def _params(layer):
    return dict(mu_w=layer.mu_kernel, rho_w=layer.rho_kernel, mu_b=layer.mu_bias, rho_b=layer.rho_bias)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("flip", [False, True], ids=FLIP_IDS)
@pytest.mark.parametrize("rid", GRAD_ROWS)
def test_backward_vs_fp64_autograd_of_the_oracle(rid, flip, S):
    """out, dL/dx and the four parameter gradients of L = (out * gout).sum() + 3 * kl against float64 autograd of the oracle on the
    draws the forward made (materialize_last_draw), at the tolerances of test_gpu_autograd.py."""
    from oracle import bt_oracle as O
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    rng.manual_seed(11)
    layer, B = _layer(rid, flip), GC.ROWS[rid]["B"]
    x = _c(GC.inputs(rid)["x"])[:B].clone().requires_grad_(True)
    if S == 1:
        out, kl = layer(x)
    else:
        with mc.mc_samples(S, B):
            out, kl = layer(x)
    _want(rid, flip, layer._last["kernel"])
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).cuda()
    ((out * gout).sum() + 3.0 * kl).backward()
    params = _params(layer)
    o_ref, gx_ref, gp_ref = GRC.oracle_grads(flip, params, x, layer.materialize_last_draw(), layer._conv_desc(), gout, S, True)
    p64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in params.items()}
    pri = [v.double().cpu() for v in (layer.prior_weight_mu, layer.prior_weight_sigma, layer.prior_bias_mu, layer.prior_bias_sigma)]
    O.kl_layer_ref(p64["mu_w"], p64["rho_w"], pri[0], pri[1], p64["mu_b"], p64["rho_b"], pri[2], pri[3]).backward()
    tag = f"{rid} {FLIP_IDS[flip]} S={S} ({layer._last['kernel']})"
    assert_close(out, o_ref, 1e-4, 1e-5, tag + " out")
    assert_close(x.grad, gx_ref, 1e-4, 1e-5, tag + " dL/dx")
    for k, v in params.items():
        assert_close(v.grad, gp_ref[k] + 3.0 * p64[k].grad, 2e-4, 2e-5, f"{tag} dL/d{k}")


def _step(layer, x0, S, B, gout=None):
    """One forward + backward of L = (out * gout).sum() -> (out, gout, [dx, dmu_w, drho_w, dmu_b, drho_b])."""
    from bayesian_torch_amd import mc
    for p in layer.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    with mc.mc_samples(S, B):
        out = layer(x, return_kl=False)
    if gout is None:
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).cuda()
    (out * gout).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), gout, [x.grad] + [p.grad for p in _params(layer).values()]


GRAD_NAMES = ("dx", "dmu_w", "drho_w", "dmu_b", "drho_b")


def _same_bits(tag, a, b):
    for nm, u, v in zip(GRAD_NAMES, a, b):
        assert u is not None and v is not None, (tag, nm)
        assert torch.equal(u, v), f"{tag}: {nm} differs, max abs {float((u - v).abs().max()):.3e} at {int((u != v).sum())} of {u.numel()} elements"


@pytest.mark.parametrize("flip", [False, True], ids=FLIP_IDS)
@pytest.mark.parametrize("rid", ["dw3", "cig4"])
def test_backward_supplied_draws_unpaired_launches_and_the_aten_checker(rid, flip):
    """The methods of test_gpu_grad_oracle.py and test_gpu_autograd.py on a depthwise and a four-channel-group row: the draws an
    on-chip step made, handed back through inject_draw, give the same gradient bits; dgrad / wgrad and their finishing passes as four
    launches (bt_debug_bwd_pair(0)) give the paired launch's bits; BACKWARD_IMPL = "aten" agrees with "hip"."""
    import bayesian_torch_amd.autograd as AG
    from bayesian_torch_amd import _lib, rng
    hooks = C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
    rng.set_mode("philox")
    rng.manual_seed(11)
    S, B = 2, GC.ROWS[rid]["B"]
    layer = _layer(rid, flip)
    x0 = _c(GC.inputs(rid)["x"])[:B]
    out1, gout, g1 = _step(layer, x0, S, B)
    _want(rid, flip, layer._last["kernel"])
    draws = layer.materialize_last_draw()
    layer.inject_draw = draws
    out2, _, g2 = _step(layer, x0, S, B, gout)
    assert layer._last["draw"] is not None
    _same_bits(f"{rid}: supplied vs on-chip draws", g2, g1)
    try:
        hooks.bt_debug_bwd_pair(0)
        _, _, unpaired = _step(layer, x0, S, B, gout)
    finally:
        hooks.bt_debug_bwd_pair(1)
    _same_bits(f"{rid}: unpaired vs paired", unpaired, g2)
    try:
        AG.BACKWARD_IMPL = "aten"
        _, _, aten = _step(layer, x0, S, B, gout)
    finally:
        AG.BACKWARD_IMPL = "hip"
    for nm, a, b in zip(GRAD_NAMES, g2, aten):
        assert_close(a, b, 2e-4, 2e-5, f"{rid} {FLIP_IDS[flip]}: hip vs aten {nm}")
    o_ref, gx_ref, gp_ref = GRC.oracle_grads(flip, _params(layer), x0, draws, layer._conv_desc(), gout, S, True)
    assert_close(out2, o_ref, 1e-4, 1e-5, f"{rid} out")
    assert_close(g2[0], gx_ref, 1e-4, 1e-5, f"{rid} dL/dx")
    for g, (k, ref) in zip(g2[1:], gp_ref.items()):
        assert_close(g, ref, 2e-4, 2e-5, f"{rid} dL/d{k}")


# ----------------------------------------------------------------------------------------------------------------- H. family layers
R3 = dict(prior_mean=0.0, prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0)
# (id, class, constructor, x shape, flavour of the default path's launch, the path switch to flip to "native" or None)
FAMILY_ROWS = [
    ("c1r_dw", "Conv1dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=5, padding=2, groups=8), (8, 8, 64), "quad", None),
    ("t2r_dw", "ConvTranspose2dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=3, stride=2, padding=1, output_padding=1, groups=8),
     (8, 8, 8, 8), "quad", "set_transpose_path"),
    ("c3f_dw", "Conv3dFlipout", dict(in_channels=6, out_channels=6, kernel_size=3, padding=1, groups=6), (4, 6, 4, 8, 8), "quad", "set_conv3d_path"),
]


def _native_oracle(layer, x, draws, S):
    """The native-path launch of a family layer over a shared x, in the reference's layouts (its Flipout signs are per REAL element)."""
    import test_gpu_family_parity as FP
    from oracle import bt_oracle as O
    p, conv = FP._params64(layer), FP._native_conv(layer)
    t = lambda v: v.detach().double().cpu()
    outs = []
    for s in range(S):
        eb = t(draws["eps_b"][s]) if "eps_b" in draws else None
        if layer._flip:
            outs.append(O.flipout_fwd_ref(x, p["mu_w"], p["rho_w"], t(draws["eps_w"][s]), t(draws["sign_in"][s]), t(draws["sign_out"][s]),
                                          p["mu_b"], p["rho_b"], eb, conv))
        else:
            outs.append(O.reparam_fwd_ref(x, p["mu_w"], p["rho_w"], t(draws["eps_w"][s]), p["mu_b"], p["rho_b"], eb, conv))
    return torch.cat(outs)


@pytest.mark.parametrize("rid,cls,ctor,xshape,want,switch", FAMILY_ROWS, ids=[r[0] for r in FAMILY_ROWS])
def test_depthwise_family_layers_forward_and_gradients(rid, cls, ctor, xshape, want, switch):
    """A depthwise Conv1d, ConvTranspose2d and Conv3d, as test_gpu_family_parity.py holds its rows: on-chip draws against the fp64
    oracle on the draws the layer reports (S = 1, S = 3), the gradients of out * gout + 3 * KL against fp64 autograd of the oracle,
    and -- where the class has one -- the "native" x path, whose launch record must say the path it took."""
    import test_gpu_family_parity as FP
    import bayesian_torch_amd.layers as L
    from oracle import bt_oracle as O
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    rng.manual_seed(1234)
    layer = FP._make(cls, ctor, 7)
    B = xshape[0]
    scale = (1 + torch.arange(xshape[1], dtype=torch.float32) / 4).view((1, -1) + (1,) * (len(xshape) - 2))
    x = (torch.randn(xshape, generator=torch.Generator().manual_seed(3)) * scale).cuda()
    with torch.no_grad():
        out = layer(x, return_kl=False)
        FP._check_run(layer, out, x, 1, True, want, f"{rid} S=1")
        assert "x_path" not in layer._last      # the default setting's launch record
        with mc.mc_samples(3, B, sample0=5):
            out = layer(x, return_kl=False)
        FP._check_run(layer, out, x, 3, True, want, f"{rid} S=3 shared")
        if switch is not None:
            prev = getattr(L, switch)("native")
            try:
                with mc.mc_samples(3, B, sample0=2):
                    out = layer(x, return_kl=False)
            finally:
                getattr(L, switch)(prev)
            kn = layer._last["kernel"]
            assert layer._last["x_path"] == "native", (rid, layer._last)
            assert kn.startswith(("fused_fwd_kernel<", "fused_split_kernel<")), kn      # the stem kernel never takes the virtual fetch
            ref = _native_oracle(layer, x.cpu().double(), layer.materialize_last_draw(), 3)
            assert_close(out.cpu(), ref, 1e-4, 1e-5, f"{rid} native path ({kn})")
    # gradients (the training path always materialises)
    rng.manual_seed(11)
    xg = x.clone().requires_grad_(True)
    with mc.mc_samples(2, B):
        out, kl = layer(xg)
    assert FP.flavour(layer._last["kernel"]) == want and layer._last.get("x_path", "materialised") != "native", layer._last
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).cuda()
    ((out * gout).sum() + 3.0 * kl).backward()
    p = FP._params64(layer, grad=True)
    xc = x.detach().cpu().double().requires_grad_(True)
    ref = FP._oracle(layer, xc, p, layer.materialize_last_draw(), 2, True)
    prior = lambda v: None if v is None else v.cpu().double()
    klr = O.kl_layer_ref(p["mu_w"], p["rho_w"], prior(layer.prior_weight_mu), prior(layer.prior_weight_sigma), p["mu_b"], p["rho_b"],
                         prior(layer.prior_bias_mu), prior(layer.prior_bias_sigma))
    ((ref * gout.cpu().double()).sum() + 3.0 * klr).backward()
    assert_close(out.detach().cpu(), ref.detach(), 1e-4, 1e-5, f"{rid} out")
    assert_close(xg.grad.cpu(), xc.grad, 1e-4, 1e-5, f"{rid} dL/dx")
    for k, v in (("mu_w", layer.mu_kernel), ("rho_w", layer.rho_kernel), ("mu_b", layer.mu_bias), ("rho_b", layer.rho_bias)):
        assert_close(v.grad.cpu(), p[k].grad, 2e-4, 2e-5, f"{rid} dL/d{k}")


# ----------------------------------------------------------------------------------------------------------------- I. a converted model
def _mobile_block():
    """Stem -> depthwise 3x3 -> pointwise 1x1 -> head, BatchNorm constants of their own per channel."""
    nn = torch.nn
    torch.manual_seed(4)
    net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), nn.BatchNorm2d(16), nn.ReLU(), nn.Conv2d(16, 16, 3, padding=1, groups=16), nn.BatchNorm2d(16),
                        nn.ReLU(), nn.Conv2d(16, 32, 1), nn.BatchNorm2d(32), nn.ReLU(), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(32, 10))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.3), m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.weight.copy_((torch.rand(n, generator=g) + 0.5) * torch.where(torch.arange(n) % 3 == 1, -1.0, 1.0))
                m.bias.copy_(torch.randn(n, generator=g) * 0.2)
    return net


def _converted(btype):
    from oracle import bt_oracle as O
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    ref, net = _mobile_block(), _mobile_block()
    O.ref_dnn_to_bnn(ref, btype)
    dnn_to_bnn(net, dict(PRIOR, type=btype))
    H.fill_bayes_params(ref, 6), H.fill_bayes_params(net, 6)
    assert net[3].groups == 16 and tuple(net[3].mu_kernel.shape) == (16, 1, 3, 3)
    x = torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(7)) * torch.tensor([1.0, 1.25, 1.5]).view(1, 3, 1, 1)
    return ref.eval(), net.cuda().eval(), x


@pytest.mark.parametrize("btype", ["Reparameterization", "Flipout"])
def test_converted_depthwise_model_inference(btype):
    """dnn_to_bnn passes ``groups`` through: mc_forward at S = 4 against the oracle model per sample on the materialised draws;
    fold_batchnorm + eval against the unfolded model on the same draws; a McGraph replay against the eager call."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.fuse import fold_batchnorm
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import McGraph, mc_forward
    ref, net, x = _converted(btype)
    S, xd = 4, x.cuda()
    rng.set_mode("philox")
    rng.manual_seed(5)
    c0 = rng.peek_call()
    logits, kl = mc_forward(net, xd, S)
    kernels = [m._last["kernel"] for _, m in H.bayes_layers(net)]
    print(btype, "kernels:", kernels)
    assert kernels[0].startswith("fused_split_quad_kernel<") and kernels[1].startswith("fused_split_quad_kernel<"), kernels      # stem, depthwise
    assert ("flip" in kernels[1]) == (btype == "Flipout")
    draws = [m.materialize_last_draw() for _, m in H.bayes_layers(net)]
    with torch.no_grad():
        for s in range(S):
            for (_, rm), d in zip(H.bayes_layers(ref), draws):
                rm.inject = {k: v[s].cpu() for k, v in d.items()}
            assert_close(logits[s].cpu(), ref(x), RTOL, ATOL, f"{btype} sample {s}")
    folded = copy.deepcopy(net)
    assert fold_batchnorm(folded) == 3
    for (_, a), (_, b) in zip(H.bayes_layers(net), H.bayes_layers(folded)):
        b._layer_id = a._layer_id                  # the unfolded model's RNG coordinates
    rng.set_call(c0)
    got, kl1 = mc_forward(folded, xd, S)
    assert folded[3].post_scale is not None and [m._last["kernel"] for _, m in H.bayes_layers(folded)][1].startswith("fused_split_quad_kernel<")
    assert_close(got.cpu(), logits.cpu(), 1e-5, 1e-6, "fold_batchnorm vs unfolded")
    assert torch.equal(kl, kl1)
    g = McGraph(net, xd, S)
    c = rng.peek_call()
    l, gkl, _ = g.replay()
    l, gkl = l.clone(), gkl.clone()
    rng.set_call(c)
    e, ekl = mc_forward(net, xd, S)
    assert torch.equal(e, l)
    assert_close(ekl.cpu(), gkl.cpu(), 1e-6, 0, "kl")


@pytest.mark.parametrize("btype", ["Reparameterization", "Flipout"])
def test_converted_depthwise_model_train_graph_step(btype):
    """One TrainGraph(fused=True) step == the eager step from the same RNG position (the criterion of
    test_train_graph_replays_the_eager_training_loop): the parameters bit for bit, the loss value to 1e-6."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import TrainGraph
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    _, net, x = _converted(btype)
    net = net.train()
    twin = copy.deepcopy(net)
    xd = x.cuda()
    y = torch.randint(0, 10, (8,), generator=torch.Generator().manual_seed(2)).cuda()
    loss_fn = lambda m, out, yy: torch.nn.functional.cross_entropy(out, yy) + get_kl_loss(m) / 8
    n_warm = 3
    rng.set_mode("philox")
    rng.manual_seed(11)
    opt_r = torch.optim.SGD(twin.parameters(), lr=0.01, momentum=0.9)
    for _ in range(n_warm + 1):
        opt_r.zero_grad(set_to_none=True)
        loss = loss_fn(twin, twin(xd), y)
        loss.backward()
        opt_r.step()
    rng.manual_seed(11)
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
    tg = TrainGraph(net, opt, loss_fn, xd, y, warmup=n_warm, fused=True)
    got = float(tg.step())
    assert abs(got - float(loss)) <= 1e-6 * abs(float(loss)), (got, float(loss))
    for (k, a), (_, b) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), k


# ----------------------------------------------------------------------------------------------------------------- J. a grouped fuzz
def _rand_grouped(r):
    """A random grouped geometry: groups in {2, 3, 4, 8, Ci}, Cig in {1, 2, 3, 4, 8, 12, 16}, Cog in {1, 2, 5, 8, 70}, 1 to 25 taps,
    strides and dilations in {1, 2}, 2- to 16-pixel maps, B in {2, 8, 32}."""
    Cig = r.choice([1, 2, 3, 4, 8, 12, 16])
    groups = r.choice([2, 3, 4, 8, "Ci"])
    if groups == "Ci":      # depthwise: as many groups as input channels
        Cig, groups = 1, r.choice([6, 12, 24, 40])
    Cog = r.choice([1, 2, 5, 8, 70])
    kh, kw = r.randint(1, 5), r.randint(1, 5)
    st, dl = (r.choice([1, 1, 2]), r.choice([1, 1, 2])), (r.choice([1, 1, 2]), r.choice([1, 1, 2]))
    pd = (r.randint(0, (kh - 1) * dl[0]), r.randint(0, (kw - 1) * dl[1]))
    H, W = r.choice([2, 3, 4, 7, 8, 12, 16]), r.choice([2, 3, 4, 7, 8, 12, 16])
    H, W = max(H, (kh - 1) * dl[0] + 1 - 2 * pd[0]), max(W, (kw - 1) * dl[1] + 1 - 2 * pd[1])
    return dict(Ci=Cig * groups, Co=Cog * groups, groups=groups, k=(kh, kw), st=st, pd=pd, dl=dl, H=H, W=W, B=r.choice([2, 8, 32]),
                S=r.choice([1, 2, 3]), bias=r.random() < 0.5, flip=r.random() < 0.5)


# (a seed whose 40 draws the host dispatch plans onto 3 quad Reparameterization, 3 quad Flipout and 6 general split launches with groups > 2)
FUZZ_SEED, FUZZ_CASES = 20261082, 40


def test_random_grouped_geometries_agree_with_the_fp32_kernels_and_the_oracle():
    """40 random grouped geometries, each launched in automatic mode behind NaN-poisoned LDS and in f32 mode: finite and equal within
    the contraction's rounding (test_gpu_split.py's criterion: < 2e-5 of max); every third case sample 0 against the C oracle."""
    from oracle import c_oracle as CO
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [C.c_void_p, C.c_void_p]
    L.bt_debug_poison_lds.restype = C.c_int
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    r = random.Random(FUZZ_SEED)
    dev = torch.device("cuda")
    taken = []
    for case in range(FUZZ_CASES):
        g = _rand_grouped(r)
        gen = torch.Generator().manual_seed(case)
        wshape = (g["Co"], g["Ci"] // g["groups"]) + g["k"]
        mu, rho = (torch.randn(wshape, generator=gen) * 0.1).cuda(), (torch.randn(wshape, generator=gen) * 0.1 - 3).cuda()
        mb = (torch.randn(g["Co"], generator=gen) * 0.1).cuda() if g["bias"] else None
        rb = (torch.randn(g["Co"], generator=gen) * 0.1 - 3).cuda() if g["bias"] else None
        x = (torch.randn(g["S"] * g["B"], g["Ci"], g["H"], g["W"], generator=gen) * (1 + torch.arange(g["Ci"]) / 4.0).view(1, -1, 1, 1)).cuda()
        conv = GC.conv_of(g)
        kw = dict(flip=g["flip"], conv=conv, S=g["S"], shared_x=False, seed=5, call=case, layer_id=3, packed=F.pack_params(mu, rho))
        outs = {}
        for mode in (0, 1):
            _lib.check(L.bt_set_contraction(mode))
            try:
                assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0
                outs[mode], _ = F.fused_forward(x, mu, rho, mb, rb, **kw)
                if mode == 0:
                    kn = L.bt_last_kernel_name().decode()
                    taken.append((kn, g["groups"], g["flip"]))
            finally:
                L.bt_set_contraction(0)
        a, b = outs[0], outs[1]
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (case, g, kn)
        if case % 3 == 0:
            Bq, S_, cm = g["B"], g["S"], (lambda t: None if t is None else t.cpu())
            eps_w = F.rng_fill_normal(5, case, 3, 0, 0, S_, mu.shape, dev).cpu()
            eps_b = F.rng_fill_normal(5, case, 3, 0, 1, S_, (g["Co"],), dev).cpu() if g["bias"] else None
            xs = x[:Bq].cpu()
            if g["flip"]:
                s_in = F.rng_fill_sign(5, case, 3, 0, 2, S_, (Bq,) + tuple(x.shape[1:]), dev).cpu()
                s_out = F.rng_fill_sign(5, case, 3, 0, 3, S_, (Bq,) + tuple(a.shape[1:]), dev).cpu()
                ref = CO.flipout_fwd(xs, mu.cpu(), rho.cpu(), eps_w[0], s_in[0], s_out[0], cm(mb), cm(rb), None if eps_b is None else eps_b[0], conv)
            else:
                ref = CO.reparam_fwd(xs, mu.cpu(), rho.cpu(), eps_w[0], cm(mb), cm(rb), None if eps_b is None else eps_b[0], conv)
            assert_close(a[:Bq].cpu(), ref, RTOL, ATOL, f"grouped fuzz case {case} {g} {kn} vs C oracle")
        err = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)
        assert err < 2e-5, (case, g, kn, err)
    counts = {}
    for kn, groups, flip in taken:
        key = kn.split("<")[0] + ("/flip" if flip else "") + ("/groups>2" if groups > 2 else "")
        counts[key] = counts.get(key, 0) + 1
    print("kernels taken in automatic mode:", counts)
    quad_r = sum(kn.startswith("fused_split_quad_kernel<") and not flip and groups > 2 for kn, groups, flip in taken)
    quad_f = sum(kn.startswith("fused_split_quad_kernel<") and flip and groups > 2 for kn, groups, flip in taken)
    general = sum(kn.startswith("fused_split_kernel<") and groups > 2 for kn, groups, flip in taken)
    assert quad_r >= 1 and quad_f >= 1 and general >= 1, counts
