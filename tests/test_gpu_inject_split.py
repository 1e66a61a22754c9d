"""GPU: supplied draws on the split-precision (bf16x3) kernels -- ``rng.set_inject_path("split")``.

``bt_pack_eps`` re-lays a draw into the packed parameters' layout and the injected (``inj``) instantiations of the general,
stem (quad), direct and split-K (skinny) kernels read it where their on-chip twins run Philox; everything behind the draw is the
same code, so a replayed on-chip draw must reproduce the on-chip launch BIT FOR BIT.  Every row asserts the kernel name it is
there to reach, so a dispatch change cannot quietly turn a split-kernel test into a general-kernel test."""
import ctypes

import pytest
import torch

from conftest import assert_close, golden_names, layer_tensors, load_golden

pytestmark = pytest.mark.gpu
PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "moped_enable": False, "moped_delta": 0.5}


@pytest.fixture(autouse=True)
def _restore_switches():
    from bayesian_torch_amd import _lib, rng
    rng.seed()
    saved = {k: getattr(rng._state, k, None) for k in ("seed", "pinned", "call")}
    yield
    for k, v in saved.items():
        setattr(rng._state, k, v)
    rng.set_inject_path("general")
    rng.set_mode("philox")
    L = _lib.lib()
    L.bt_debug_force_bn32(-1)
    L.bt_set_contraction(0)


def check_twins(got, onchip):
    """Layer by layer: a split kernel's replay is its injected twin; a layer on the fp32 kernels replays on the general kernel."""
    assert len(got) == len(onchip)
    for q, k in zip(got, onchip):
        assert (q == inj_name(k)) if "bf16x3" in k else ("fused_fwd_kernel" in q and "inj=1" in q), (got, onchip)


def inj_name(onchip):
    """The injected twin of an on-chip split kernel name."""
    assert onchip.endswith(">") and "bf16x3" in onchip, onchip
    return onchip[:-1] + ",inj>"


# ------------------------------------------------------------------------------------------------------------------ 1. bt_pack_eps
@pytest.mark.parametrize("Cig", [3, 8, 20, 64])
@pytest.mark.parametrize("T", [1, 9, 49])
@pytest.mark.parametrize("S", [1, 3])
def test_pack_eps_is_the_torch_permutation(Cig, T, S):
    from bayesian_torch_amd import _lib
    Co = 37
    eps = torch.randn(S, Co, Cig, T, generator=torch.Generator().manual_seed(Cig * 100 + T)).cuda()
    C4 = (Cig + 3) // 4 * 4
    out = torch.full((S, Co, T, C4), float("nan"), device="cuda")
    _lib.check(_lib.lib().bt_pack_eps(eps.data_ptr(), S, Co, Cig, T, out.data_ptr(), _lib.stream_ptr(eps.device)))
    want = torch.zeros(S, Co, T, C4, device="cuda")
    want[..., :Cig] = eps.view(S, Co, Cig, T).permute(0, 1, 3, 2)
    assert torch.equal(out, want)


@pytest.mark.parametrize("shape", [(40, 24, 3, 3), (64, 3, 7, 7), (10, 512), (96, 130, 1, 1)])
def test_pack_eps_of_mu_is_mu_packed(shape):
    """Packing the parameters themselves with bt_pack_eps reproduces bt_pack_params' mu_packed bit for bit: one layout."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    mu = torch.randn(*shape, generator=torch.Generator().manual_seed(3)).cuda()
    mp, _ = F.pack_params(mu, torch.zeros_like(mu))
    Co, Ci = shape[0], shape[1]
    T = mu[0, 0].numel()
    out = torch.empty_like(mp)
    _lib.check(_lib.lib().bt_pack_eps(mu.data_ptr(), 1, Co, Ci, T, out.data_ptr(), _lib.stream_ptr(mu.device)))
    assert torch.equal(out, mp)


# ------------------------------------------------------------------------------------------------ 2. bit-identical replay, per flavour
# label: (kind, Ci, Co, k, stride, pad, H, W, B, bias, bn32 (None: automatic), pool, on-chip kernel name at S = 3)
ROWS = {
    "general 512-wide, row pieces (64->256 k3 p1 on 8x8, b512)": ("conv", 64, 256, 3, 1, 1, 8, 8, 512, False, None, False,
                                                                  "fused_split_kernel<64,512,bf16x3,6 terms,npw=4,xm=3>"),
    "512-wide, every second column (24->64 1x1 s2 on 16x16, b512)": ("conv", 24, 64, 1, 2, 0, 16, 16, 512, True, None, False,
                                                                     "fused_split_kernel<64,512,bf16x3,6 terms,npw=4,xm=4>"),
    "256-wide row tiles (256->256 k3 p1 on 2x2, b1024)": ("conv", 256, 256, 3, 1, 1, 2, 2, 1024, False, None, False,
                                                          "fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=2>"),
    "256-wide whole-image stride-2 (128->256 k3 s2 p1 on 4x4, b1024)": ("conv", 128, 256, 3, 2, 1, 4, 4, 1024, True, None, False,
                                                                        "fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=3>"),
    "128-wide whole-image stride-2 (128->256 k3 s2 p1 on 4x4, b128)": ("conv", 128, 256, 3, 2, 1, 4, 4, 128, True, None, False,
                                                                       "fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=0>"),
    "128-wide (512->512 k3 p1 on 1x1 maps), 64-channel tiles": ("conv", 512, 512, 3, 1, 1, 1, 1, 128, False, 0, False,
                                                                "fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=1>"),
    "128-wide row tiles (256->256 k3 p1 on 2x2, b128)": ("conv", 256, 256, 3, 1, 1, 2, 2, 128, False, None, False,
                                                         "fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=2>"),
    "128-wide Linear 3072->512, 64-channel tiles": ("linear", 3072, 512, 1, 1, 0, 1, 1, 256, True, 0, False,
                                                    "fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=1>"),
    "128-wide Linear 3072->512, bn32": ("linear", 3072, 512, 1, 1, 0, 1, 1, 256, True, 1, False,
                                        "fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=1>"),
    "ragged (24->40 k3 p1 on 8x8), bias": ("conv", 24, 40, 3, 1, 1, 8, 8, 64, True, None, False,
                                           "fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=0>"),
    "ragged (24->40 k3 p1 on 8x8), no bias, 64-channel tiles": ("conv", 24, 40, 3, 1, 1, 8, 8, 64, False, 0, False,
                                                                "fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>"),
    "quad: CIFAR stem 3->64 k7 s2 p3": ("conv", 3, 64, 7, 2, 3, 32, 32, 32, False, None, False,
                                        "fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0>"),
    "quad: CIFAR stem 3->64 k7 s2 p3 + max-pool": ("conv", 3, 64, 7, 2, 3, 32, 32, 32, False, None, True,
                                                   "fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1>"),
    "quad: 3->16 k3": ("conv", 3, 16, 3, 1, 1, 16, 16, 16, True, None, False,
                       "fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0>"),
    "direct resident (64->256 1x1 on 16x16)": ("conv", 64, 256, 1, 1, 0, 16, 16, 32, False, None, False,
                                               "fused_split_direct_kernel<64,8x64,bf16x3,6 terms,resident W>"),
    "direct strided (128->256 1x1 s2 on 8x8)": ("conv", 128, 256, 1, 2, 0, 8, 8, 64, True, None, False,
                                                "fused_split_direct_kernel<64,8x64,bf16x3,6 terms,resident W>"),
    "direct streamed (512->128 1x1 on 8x8)": ("conv", 512, 128, 1, 1, 0, 8, 8, 64, False, None, False,
                                              "fused_split_direct_kernel<64,8x64,bf16x3,6 terms,streamed W>"),
    "skinny (512->10 Linear)": ("linear", 512, 10, 1, 1, 0, 1, 1, 128, True, None, False,
                                "fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 128>"),
}
# a pooled stem over a shared input walks several samples per workgroup on chip; its replay runs the one-sample pooled kernel
WALK = "fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1,walk>"


def _layer(row, seed):
    import bayesian_torch_amd.layers as L
    kind, Ci, Co, k, st, pd, H, W, B, bias, bn32, pool, name = row
    torch.manual_seed(seed)
    if kind == "linear":
        m = L.LinearReparameterization(Ci, Co, bias=bias)
    else:
        m = L.Conv2dReparameterization(Ci, Co, k, stride=st, padding=pd, bias=bias)
    m = m.cuda().eval()
    m.post_pool = pool
    return m


def _x(row, S, seed):
    kind, Ci, Co, k, st, pd, H, W, B = row[:9]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(S * B, Ci, generator=g) if kind == "linear" else torch.randn(S * B, Ci, H, W, generator=g)).cuda()


def _replay_row(label, shared, stage, poison=None):
    """on-chip launch -> materialised draw -> injected launch on the path "split": equal bits, twin kernel, same KL."""
    from bayesian_torch_amd import _lib, rng
    from bayesian_torch_amd.mc import mc_samples
    row = ROWS[label]
    kind, Ci, Co, k, st, pd, H, W, B, bias, bn32, pool, want = row
    S = 3
    Lb = _lib.lib()
    Lb.bt_debug_force_bn32(-1 if bn32 is None else bn32)
    m = _layer(row, 11)
    xs = _x(row, S, 5)
    x = xs[:B].contiguous() if shared else xs
    res = None
    if stage:      # folded output stage: scale / shift (+ residual) + ReLU
        g = torch.Generator().manual_seed(9)
        m.post_scale = (torch.rand(Co, generator=g) + 0.5).cuda()
        m.post_shift = torch.randn(Co, generator=g).cuda()
        m.post_relu = True
    rng.manual_seed(1234)

    def run():
        nonlocal res
        if poison is not None:
            poison()
        with torch.no_grad(), mc_samples(S, B):
            if stage and not pool and res is None:
                probe, _ = m(x, True)
                res = torch.randn(probe.shape, generator=torch.Generator().manual_seed(4)).cuda()
                if poison is not None:
                    poison()
            out, kl = m(x, True, res) if res is not None else m(x, True)
        return out, kl, m._last["kernel"]

    out0, kl0, k0 = run()
    walked = pool and shared and k0 == WALK
    assert k0 == want or walked, (label, k0)
    draw = m.materialize_last_draw()
    assert draw["eps_w"].shape == (S,) + tuple(m._w("mu").shape)
    m.inject_draw = draw
    rng.set_inject_path("split")
    out1, kl1, k1 = run()
    assert k1 == inj_name(want), (label, k1)
    assert torch.equal(out1, out0), (label, float((out1 - out0).abs().max()))
    assert_close(kl1.cpu(), kl0.cpu(), 1e-5, 0, label + ": KL")
    d2 = m.materialize_last_draw()      # still the natural-layout tensors the caller supplied
    assert d2["eps_w"].data_ptr() == draw["eps_w"].data_ptr() and torch.equal(d2["eps_w"], draw["eps_w"])
    # the default path is untouched: the fp32 general kernel (it refuses the fused max-pool: pooled separately), close but not equal bits
    rng.set_inject_path("general")
    out2, _, k2 = run()
    assert "split" not in k2 and "inj=1" in k2, (label, k2)
    assert_close(out2.cpu(), out0.cpu(), 1e-4, 1e-5, label + ": general path")


@pytest.mark.parametrize("stage", [False, True], ids=["plain", "folded-stage"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared-x", "stacked-x"])
@pytest.mark.parametrize("label", list(ROWS))
def test_replay_is_bit_identical(label, shared, stage):
    _replay_row(label, shared, stage)


@pytest.mark.parametrize("label", ["general 512-wide, row pieces (64->256 k3 p1 on 8x8, b512)", "256-wide row tiles (256->256 k3 p1 on 2x2, b1024)",
                                   "128-wide (512->512 k3 p1 on 1x1 maps), 64-channel tiles",
                                   "quad: CIFAR stem 3->64 k7 s2 p3 + max-pool", "direct resident (64->256 1x1 on 16x16)",
                                   "direct streamed (512->128 1x1 on 8x8)", "skinny (512->10 Linear)"])
def test_replay_behind_poisoned_lds(label):
    """LDS survives from kernel to kernel: fill it with NaN patterns before every launch -- the same bits come out."""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(4, dtype=torch.int32, device="cuda")

    def poison():
        assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0

    _replay_row(label, True, True, poison)


def test_declined_launches_fall_back_and_are_remembered():
    """A layer no split flavour takes (5 input channels per group: not whole octets) runs the general kernel under "split" as well,
    and does not pack its draw again on the next call; a forced fp32 contraction declines every layer."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import _lib, rng
    torch.manual_seed(2)
    m = L.Conv2dReparameterization(5, 7, 3, padding=1).cuda().eval()
    x = torch.randn(4, 5, 6, 6).cuda()
    with torch.no_grad():
        out0, _ = m(x)
        m.inject_draw = m.materialize_last_draw()
        rng.set_inject_path("split")
        out1, _ = m(x)
        assert "split" not in m._last["kernel"] and "inj=1" in m._last["kernel"]
        assert len(m._eps_pack["declined"]) == 1
        m._eps_pack["buf"] = None
        out2, _ = m(x)
        assert m._eps_pack["buf"] is None and torch.equal(out1, out2)      # no second pack
        rng.set_inject_path("general")
        out3, _ = m(x)
    assert torch.equal(out1, out3)
    assert_close(out1.cpu(), out0.cpu(), 1e-4, 1e-5, "fallback")
    # forced fp32 contraction: refused before any launch, with the reason
    row = ROWS["ragged (24->40 k3 p1 on 8x8), bias"]
    m = _layer(row, 1)
    x = _x(row, 1, 1)
    with torch.no_grad():
        m(x)
        assert "bf16x3" in m._last["kernel"]
        m.inject_draw = m.materialize_last_draw()
        rng.set_inject_path("split")
        _lib.check(_lib.lib().bt_set_contraction(1))
        m(x)
        assert "fused_fwd_kernel" in m._last["kernel"] and "inj=1" in m._last["kernel"]
        assert b"contraction" in _lib.lib().bt_last_error_string()


# ------------------------------------------------------------------------------------------------ 3. reference goldens on the timed kernels
def _nets(name, meta):
    from oracle import bt_oracle as O
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    mk = (lambda: H.mlp((3072, 512, 10))) if len(meta["x_shape"]) == 2 else (lambda: H.resnet18(10, 8 if "w8" in name else 64))
    torch.manual_seed(meta["seed"])
    ref = mk()
    O.ref_dnn_to_bnn(ref, meta["btype"])
    H.fill_bayes_params(ref, meta["seed"])
    net = mk()
    dnn_to_bnn(net, dict(PRIOR, type=meta["btype"]))
    H.fill_bayes_params(net, meta["seed"])
    return ref.eval(), net.cuda().eval()


def _replay_reference_draws(ref, x, meta):
    from bayesian_torch_amd.harness import resnet as H
    layers = [m for _, m in H.bayes_layers(ref)]
    logits, draws = [], [dict(eps_w=[], eps_b=[]) for _ in layers]
    with torch.no_grad():
        for s in range(meta["S"]):
            torch.manual_seed(meta["seed"] * 100 + s)
            logits.append(ref(x))
            for m, d in zip(layers, draws):
                d["eps_w"].append(getattr(m, "eps_" + m._wn).clone())
                if m.mu_bias is not None:
                    d["eps_b"].append(m.eps_bias.clone())
    stack = lambda lst: torch.stack(lst).cuda() if lst else None
    return torch.stack(logits), [{k: stack(v) for k, v in d.items()} for d in draws]


# model_r18_reparam (unfused, the golden's S and batch), on-chip draws: layers that report a bf16x3 kernel, of 21. Measured on an
# MI355X at the commit before the injected instantiations existed: 21 of 21, no exceptions (stem: quad kernel; 3 downsamples: direct
# kernel, resident W; head: split-K 128; the 16 others: 32-channel 128-wide tiles, x fetch modes 0 / 2 / 1 for layer1-2 / layer3 / layer4).
R18_BF16X3_LAYERS = 21


@pytest.mark.parametrize("name", ["model_r18w8_reparam", "model_mlp_reparam", "model_r18_reparam"])
def test_model_goldens_on_the_split_kernels(name):
    """test_gpu_model.test_model_matches_reference_golden with the reference's draws read by the kernels the benchmark times:
    every layer's kernel is the one the same model reports with on-chip draws at the same S and batch, plus the marker.
    model_r18_reparam: 21 of its 21 layers report bf16x3 with on-chip draws (R18_BF16X3_LAYERS, measured at the parent commit; asserted
    here on the on-chip run), so all 21 replay on an injected split kernel."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    g = load_golden(name)
    meta = g["meta"]
    ref, net = _nets(name, meta)
    x = torch.randn(*meta["x_shape"], generator=torch.Generator().manual_seed(meta["seed"] + 7))
    ref_logits, draws = _replay_reference_draws(ref, x, meta)
    assert_close(ref_logits, g["logits"], 1e-4, 1e-5, name + ": oracle vs golden")
    layers = [m for _, m in H.bayes_layers(net)]
    S = meta["S"]
    mc_forward(net, x.cuda(), S)      # on-chip draws: the kernels this model runs at this S and batch
    onchip = [m._last["kernel"] for m in layers]
    print(name, "on-chip kernels:", onchip)
    n_split = sum("bf16x3" in k for k in onchip)
    if name == "model_r18_reparam":
        assert len(onchip) == 21 and n_split == R18_BF16X3_LAYERS, onchip
    assert n_split > 0
    with torch.no_grad():
        net(x.cuda())
    onchip1 = [m._last["kernel"] for m in layers]      # ... and one sample at a time
    for m, d in zip(layers, draws):
        m.inject_draw = d
    rng.set_inject_path("split")
    logits, kl = mc_forward(net, x.cuda(), S)
    got = [m._last["kernel"] for m in layers]
    check_twins(got, onchip)
    assert_close(logits.cpu(), g["logits"], 1e-4, 1e-5, name + ": split kernels (MC-batched) vs golden")
    assert_close(kl.cpu(), g["kl"], 1e-5, 0, name + ": fused KL vs golden")
    assert_close(get_kl_loss(net).cpu(), g["kl"], 1e-5, 0, name + ": get_kl_loss vs golden")
    with torch.no_grad():
        for s in range(S):
            for m, d in zip(layers, draws):
                m.inject_draw = {k: (v[s:s + 1] if v is not None else None) for k, v in d.items()}
            assert_close(net(x.cuda()).cpu(), g["logits"][s], 1e-4, 1e-5, f"{name}: sequential sample {s}")
            check_twins([m._last["kernel"] for m in layers], onchip1)


# the layer fixtures through the switch: where each lands (split kernel, or declined -> the general kernel, as under "general")
FIXTURE_LANDS = {
    "conv2d_reparam_c16x32k1s2nb": "general",
    "conv2d_reparam_c3x16k7s2": "split",
    "conv2d_reparam_c3x8k3": "general",
    "conv2d_reparam_c4x4k3d2": "general",
    "conv2d_reparam_c64x64k3hw1": "split",
    "conv2d_reparam_c6x10k3x2": "general",
    "conv2d_reparam_c8x12g2": "general",
    "conv2d_reparam_c8x16k3s2": "general",
    "linear_reparam_cfg1": "general",
    "linear_reparam_k500": "general",
    "linear_reparam_nobias": "general",
    "linear_reparam_rprior": "general",
}


def test_fixture_table_is_complete():
    assert sorted(FIXTURE_LANDS) == sorted(golden_names("linear_reparam_") + golden_names("conv2d_reparam_"))


@pytest.mark.parametrize("name", sorted(FIXTURE_LANDS))
def test_layer_fixtures_through_the_switch(name):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    g = layer_tensors(load_golden(name))
    c = lambda t: None if t is None else t.cuda()
    st = lambda t: None if t is None else t.cuda().unsqueeze(0)
    mu, rho = c(g["mu_w"]), c(g["rho_w"])
    state = {}
    out, kl = F.fused_forward(c(g["x"]), mu, rho, c(g["mu_b"]), c(g["rho_b"]), conv=g["conv"], S=1, want_kl=True,
                              priors=tuple(c(g[k]) for k in ("prior_mu_w", "prior_sigma_w", "prior_mu_b", "prior_sigma_b")),
                              eps_w=st(g["eps_w"]), eps_b=st(g["eps_b"]), packed=F.pack_params(mu, rho), inject_path="split", eps_pack_state=state)
    kn = _lib.lib().bt_last_kernel_name().decode()
    print(name, "->", kn)
    assert_close(out.cpu(), g["out"], 1e-4, 1e-5, name + ".out")
    assert_close(kl.cpu(), g["kl"], 1e-5, 0, name + ".kl")
    if FIXTURE_LANDS[name] == "split":
        assert "bf16x3" in kn and kn.endswith(",inj>") and not state["declined"], kn
    else:
        assert "fused_fwd_kernel" in kn and "inj=1" in kn and len(state["declined"]) == 1, kn


# ------------------------------------------------------------------------------------------------ 4. fused model replay
def test_fused_model_replays_its_own_draws():
    """resnet18 converted and fuse_inference'd (folded BatchNorm / ReLU / residual adds, the stem's max-pool in its launch):
    on-chip -> materialise every layer's draw -> inject on the path "split" -> the same logits, bit for bit."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(3)
    net = H.resnet18(10, 64)
    dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
    H.fill_bayes_params(net, 3)
    net = net.cuda().eval()
    H.fuse_inference(net)
    x = torch.randn(128, 3, 32, 32, generator=torch.Generator().manual_seed(8)).cuda()
    rng.manual_seed(99)
    logits, kl = mc_forward(net, x, 4)
    assert logits.shape == (4, 128, 10)
    layers = [m for _, m in H.bayes_layers(net)]
    onchip = [m._last["kernel"] for m in layers]
    assert all("bf16x3" in k for k in onchip), onchip
    for m in layers:
        m.inject_draw = m.materialize_last_draw()
    rng.set_inject_path("split")
    logits1, kl1 = mc_forward(net, x, 4)
    got = [m._last["kernel"] for m in layers]
    want = [inj_name("fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1>" if k.endswith("walk>") else k) for k in onchip]
    assert got == want, (got, want)
    assert torch.equal(logits1, logits)
    assert_close(kl1.cpu(), kl.cpu(), 1e-5, 0, "KL")
    # the default path as it has always been (it does not raise: the general kernel refuses the fused max-pool with BT_ERR_UNSUPPORTED
    # and fused_forward pools the stem in a separate pass) -- the fp32 kernels, close to the on-chip logits, not equal to them
    rng.set_inject_path("general")
    logits2, _ = mc_forward(net, x, 4)
    assert all("inj=1" in m._last["kernel"] for m in layers)
    assert_close(logits2.cpu(), logits.cpu(), 1e-4, 1e-5, "general path")


# ------------------------------------------------------------------------------------------------ 5. "torch" mode
@pytest.mark.parametrize("which", ["r18w8", "mlp"])
def test_torch_mode_through_the_switch(which):
    """rng.set_mode("torch"): the same torch.manual_seed gives the same draws on either path; the two paths are different
    arithmetic (fp32 MFMA chain vs exact bf16x3 split in another K order) -- close, NOT bit-identical -- and the layers' eps_*
    buffers hold what the general path leaves in them."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(6)
    net = H.resnet18(10, 8) if which == "r18w8" else H.mlp((3072, 512, 10))
    dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
    H.fill_bayes_params(net, 6)
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(128, 3, 32, 32, generator=g) if which == "r18w8" else torch.randn(128, 3072, generator=g)).cuda()
    layers = [m for _, m in H.bayes_layers(net)]
    rng.set_mode("torch")
    res = {}
    for path in ("general", "split"):
        rng.set_inject_path(path)
        torch.manual_seed(41)
        with torch.no_grad():
            out = net(x)
        res[path] = (out, [m._last["kernel"] for m in layers], [getattr(m, "eps_" + m._wname).clone() for m in layers],
                     [None if m.mu_bias is None else m.eps_bias.clone() for m in layers])
    assert all("inj=1" in k for k in res["general"][1]), res["general"][1]
    n_split = sum("bf16x3" in k and k.endswith(",inj>") for k in res["split"][1])
    print(which, "split path kernels:", res["split"][1])
    assert n_split >= (2 if which == "mlp" else 1), res["split"][1]
    assert all(("bf16x3" in k and k.endswith(",inj>")) or "inj=1" in k for k in res["split"][1])
    assert_close(res["split"][0].cpu(), res["general"][0].cpu(), 1e-4, 1e-5, which + ": split vs general")
    for a, b in zip(res["general"][2], res["split"][2]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    for a, b in zip(res["general"][3], res["split"][3]):
        assert (a is None and b is None) or torch.equal(a, b)
