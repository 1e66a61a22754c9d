"""GPU: supplied Flipout draws AND signs on the split-precision (bf16x3) kernels -- ``rng.set_inject_path("split")``.

``bt_pack_eps`` re-lays the weight draw, ``bt_pack_signs`` turns the two sign tensors into byte images, and the ``flip,...,inj``
instantiations of the general and stem (quad) kernels read all of it where their on-chip twins run Philox and the sign hash;
everything behind the three read sites is the same code, so a replayed on-chip draw must reproduce the on-chip launch BIT FOR BIT.
Every row asserts the kernel name it is there to reach -- what launch_split_flip_one selects for the row's geometry with on-chip
draws; that host code is the commit's before these instantiations existed, unchanged -- so a dispatch change cannot quietly turn a
split-kernel test into a general-kernel test."""
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
    _lib.lib().bt_set_contraction(0)


def inj_name(onchip):
    """The injected twin of an on-chip split kernel name."""
    assert onchip.endswith(">") and "bf16x3" in onchip and "flip" in onchip, onchip
    return onchip[:-1] + ",inj>"


def is_general_inj(k):
    return "fused_fwd_kernel" in k and "flip" in k and "inj=1" in k


def check_twins(got, onchip):
    """Layer by layer: a split kernel's replay is its injected twin; a layer on the fp32 kernels replays on the general kernel."""
    assert len(got) == len(onchip)
    for q, k in zip(got, onchip):
        assert (q == inj_name(k)) if "bf16x3" in k else is_general_inj(q), (got, onchip)


def sign_counts(state):
    return [int(v) for v in state["sign_count"].cpu()]


# ------------------------------------------------------------------------------------------------------------------ 1. bt_pack_signs
def _pack_signs(t):
    from bayesian_torch_amd import _lib
    S, n = t.shape
    stride = _lib.signs_packed_stride(n)
    out = torch.full((S, stride), 0x55, dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), 12345, dtype=torch.int32, device="cuda")      # set by the call, not accumulated
    _lib.check(_lib.lib().bt_pack_signs(t.data_ptr(), S, n, out.data_ptr(), cnt.data_ptr(), _lib.stream_ptr(t.device)))
    return out, int(cnt.cpu()), stride


@pytest.mark.parametrize("n", [1, 15, 16, 4097])
@pytest.mark.parametrize("S", [1, 3])
def test_pack_signs_is_the_byte_map(n, S):
    g = torch.Generator().manual_seed(n * 10 + S)
    t = (torch.randint(0, 2, (S, n), generator=g).float() * 2 - 1).cuda()
    out, cnt, stride = _pack_signs(t)
    assert stride == (n + 15) // 16 * 16 and stride % 16 == 0
    want = torch.zeros(S, stride, dtype=torch.uint8, device="cuda")
    want[:, :n] = (t < 0).to(torch.uint8) * 0x80
    assert torch.equal(out, want) and cnt == 0
    # k zeros and one NaN: counted, the zeros read as +1
    k = min(3, n - 1) if n > 1 else 0
    pos = torch.randperm(S * n, generator=g)[:k + 1]
    flat = t.clone().view(-1)
    flat[pos[:k].cuda()] = 0.0
    flat[pos[k:].cuda()] = float("nan")
    out2, cnt2, _ = _pack_signs(flat.view(S, n))
    assert cnt2 == k + 1
    rows, cols = (pos[:k] // n).cuda(), (pos[:k] % n).cuda()
    assert bool((out2[rows, cols] == 0).all())
    keep = torch.ones(S * n, dtype=torch.bool, device="cuda")
    keep[pos.cuda()] = False
    assert torch.equal(out2[:, :n].reshape(-1)[keep], want[:, :n].reshape(-1)[keep]) and bool((out2[:, n:] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. bit-identical replay, per instantiation
# label: (kind, Ci, Co, k, stride, pad, dilation, groups, H, W, B, S, bias, pool, on-chip kernel name). The geometries are FLIP_GEOMS and
# FLIP_STEMS of tests/test_gpu_split.py (with their batch and sample counts) plus the pooled CIFAR stem; a row whose on-chip launch
# is an fp32 kernel (GENERAL) replays on the general kernel.
GENERAL = "fp32"
N256_3 = "fused_split_kernel<64,256,bf16x3,2x6 terms,flip,npw=4,xm=3>"
N256_0 = "fused_split_kernel<64,256,bf16x3,2x6 terms,flip,npw=4,xm=0>"
N128_0 = "fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=0>"
N128_1 = "fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=1>"
N128_2 = "fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=2>"
Q0 = "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0>"
Q1 = "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=1>"
ROWS = {
    "flip layer1 64x64 3x3 8x8 (row pieces, xm=3)": ("conv", 64, 64, 3, 1, 1, 1, 1, 8, 8, 128, 2, True, False, N128_0),
    "flip layer2 128x128 3x3 4x4": ("conv", 128, 128, 3, 1, 1, 1, 1, 4, 4, 128, 2, False, False, N128_0),
    "flip 1x1 bottleneck 64->256 8x8 (one tap: octet pairs)": ("conv", 64, 256, 1, 1, 0, 1, 1, 8, 8, 64, 2, True, False, N128_0),
    "flip row bands 16x32 3x3 28x28, ragged channels": ("conv", 16, 40, 3, 1, 1, 1, 1, 28, 28, 4, 1, True, False, N128_0),
    "flip W % 4 != 0 (generic fetch) 24x64 3x3 6x6": ("conv", 24, 64, 3, 1, 1, 1, 1, 6, 6, 64, 2, True, False, N128_0),
    "flip layer3 256x256 3x3 on 2x2 maps (128 tile of whole images)": ("conv", 256, 256, 3, 1, 1, 1, 1, 2, 2, 128, 2, False, False, N128_0),
    "flip layer4 512x512 3x3 on 1x1 maps (128 tile, one tap, xm=1)": ("conv", 512, 512, 3, 1, 1, 1, 1, 1, 1, 128, 2, True, False, N128_1),
    "flip layer3.0.conv1 128->256 3x3 s2 4x4->2x2 (pixel-major, generic fetch)": ("conv", 128, 256, 3, 2, 1, 1, 1, 4, 4, 128, 2, True, False, GENERAL),
    "flip layer4.0.downsample 256->512 1x1 s2 2x2->1x1 (one tap)": ("conv", 256, 512, 1, 2, 0, 1, 1, 2, 2, 128, 2, False, False, N128_0),
    "flip small batch 64x64 3x3 4x4, B = 16 (128 tile of whole images)": ("conv", 64, 64, 3, 1, 1, 1, 1, 4, 4, 16, 8, True, False, N128_0),
    "flip groups 2, dilation 2": ("conv", 32, 64, 3, 1, 2, 2, 2, 8, 8, 32, 1, True, False, N128_0),
    "flip CIFAR stem 3->64 7x7 s2 on 32x32 (one image per 256 tile)": ("conv", 3, 64, 7, 2, 3, 1, 1, 32, 32, 12, 2, True, False, Q0),
    "flip 1 channel 3x3 on 16x16": ("conv", 1, 64, 3, 1, 1, 1, 1, 16, 16, 6, 2, False, False, Q0),
    "flip 3 channels 5x5 s1 on 24x24 (bands of 10 rows), 40 output channels": ("conv", 3, 40, 5, 1, 2, 1, 1, 24, 24, 4, 1, True, False, Q0),
    "flip pooled CIFAR stem 3->64 k7 s2 p3 on 32x32": ("conv", 3, 64, 7, 2, 3, 1, 1, 32, 32, 10, 3, False, True, Q1),
    # added: the smallest geometries that reach the 256-wide tiles (the cost model takes them once the 128-wide grid needs a second
    # round of 256 workgroups: 256 workgroups of 256 columns here against 512 of 128), and a Linear layer
    "flip 256-wide row pieces 16->64 3x3 8x8, B = 512": ("conv", 16, 64, 3, 1, 1, 1, 1, 8, 8, 512, 2, True, False, N256_3),
    "flip 256-wide generic fetch (W % 4 != 0) 8->64 3x3 6x6, B = 256, S = 4": ("conv", 8, 64, 3, 1, 1, 1, 1, 6, 6, 256, 4, False, False, N256_0),
    "flip Linear 512->256 (xm=1)": ("linear", 512, 256, 1, 1, 0, 1, 1, 1, 1, 128, 2, True, False, N128_1),
}
MAY_BE_GENERAL = ("one tap", "3x3 s2")       # the rows the existing suite allows to be ineligible for the split Flipout
# All six instantiations can be launched. A seventh, <64,128,xm=2> (whole 2x2 planes, as Reparameterization has it), is NOT
# instantiated: it would serve only PIXEL-MAJOR 128-wide tiles of 2x2 maps, and such a tile holds >= 112 images x the 4 patch pixels
# of a plane = 448 pixels, more than the 301 the two weight images leave in LDS: split_geometry declines, the launch falls to
# whole-image tiles (xm=0). DESIGN.md section 4.0c says so; the name stays here so that nothing starts to report it.
REACHABLE = {N256_3, N256_0, N128_0, N128_1, Q0, Q1}


def test_rows_reach_every_instantiation():
    names = [r[-1] for r in ROWS.values()]
    assert REACHABLE <= set(names) and N128_2 not in names, REACHABLE - set(names)
    general = [lb for lb, r in ROWS.items() if r[-1] == GENERAL]
    assert len(general) <= 3 and all(any(t in lb for t in MAY_BE_GENERAL) for lb in general), general


def _layer(row, seed):
    import bayesian_torch_amd.layers as L
    kind, Ci, Co, k, st, pd, dl, grp, H, W, B, S, bias, pool, name = row
    torch.manual_seed(seed)
    if kind == "linear":
        m = L.LinearFlipout(Ci, Co, bias=bias)
    else:
        m = L.Conv2dFlipout(Ci, Co, k, stride=st, padding=pd, dilation=dl, groups=grp, bias=bias)
    m = m.cuda().eval()
    m.post_pool = pool
    return m


def _x(row, seed):
    kind, Ci, Co, k, st, pd, dl, grp, H, W, B, S = row[:12]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(S * B, Ci, generator=g) if kind == "linear" else torch.randn(S * B, Ci, H, W, generator=g)).cuda()


def _replay_row(label, shared, stage, poison=None, zero_rule=False):
    """on-chip launch -> materialised draw -> injected launch on the path "split": equal bits, twin kernel, same KL, no sign counted."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import mc_samples
    row = ROWS[label]
    kind, Ci, Co, k, st, pd, dl, grp, H, W, B, S, bias, pool, want = row
    m = _layer(row, 11)
    xs = _x(row, 5)
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
    print(label, "| on-chip:", k0)
    if want == GENERAL:
        assert "split" not in k0 and "flip" in k0, (label, k0)
    else:
        assert k0 == want, (label, k0)
    draw = m.materialize_last_draw()
    assert draw["eps_w"].shape == (S,) + tuple(m._w("mu").shape)
    assert draw["sign_in"].numel() == S * x.numel() // (1 if shared else S) and draw["sign_out"].shape[0] == S
    if zero_rule:
        return m, x, draw, run
    m.inject_draw = draw
    rng.set_inject_path("split")
    out1, kl1, k1 = run()
    if want == GENERAL:      # on the fp32 kernels on chip: the replay stays on the general kernel (declined, remembered)
        assert is_general_inj(k1) and len(m._eps_pack["declined"]) == 1, (label, k1)
        assert_close(out1.cpu(), out0.cpu(), 1e-4, 1e-5, label + ": declined -> general")
    else:
        assert k1 == inj_name(want), (label, k1)
        assert torch.equal(out1, out0), (label, float((out1 - out0).abs().max()))
        assert sign_counts(m._eps_pack) == [0, 0], label
    assert_close(kl1.cpu(), kl0.cpu(), 1e-5, 0, label + ": KL")
    d2 = m.materialize_last_draw()      # still the natural-layout tensors the caller supplied
    for key in ("eps_w", "sign_in", "sign_out"):
        assert d2[key].data_ptr() == draw[key].data_ptr() and torch.equal(d2[key], draw[key])
    # the default path is untouched: the fp32 general kernel (it refuses the fused max-pool: pooled separately), close but not equal bits
    rng.set_inject_path("general")
    out2, _, k2 = run()
    assert is_general_inj(k2), (label, k2)
    assert_close(out2.cpu(), out0.cpu(), 1e-4, 1e-5, label + ": general path")


@pytest.mark.parametrize("stage", [False, True], ids=["plain", "folded-stage"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared-x", "stacked-x"])
@pytest.mark.parametrize("label", list(ROWS))
def test_replay_is_bit_identical(label, shared, stage):
    _replay_row(label, shared, stage)


# ------------------------------------------------------------------------------------------------ 3. poisoned LDS
@pytest.mark.parametrize("label", ["flip 256-wide row pieces 16->64 3x3 8x8, B = 512", "flip layer4 512x512 3x3 on 1x1 maps (128 tile, one tap, xm=1)",
                                   "flip pooled CIFAR stem 3->64 k7 s2 p3 on 32x32"])
def test_replay_behind_poisoned_lds(label):
    """LDS survives from kernel to kernel: fill it with NaN patterns before every launch -- the same bits come out."""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(4, dtype=torch.int32, device="cuda")

    def poison():
        assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0

    assert ROWS[label][-1] in (N256_3, N128_1, Q1)      # one 256-wide row, one 128-wide row, the pooled stem
    _replay_row(label, True, True, poison)


# ------------------------------------------------------------------------------------------------ 4. the zero rule
@pytest.mark.parametrize("label", ["flip layer1 64x64 3x3 8x8 (row pieces, xm=3)", "flip CIFAR stem 3->64 7x7 s2 on 32x32 (one image per 256 tile)"])
def test_an_exact_zero_sign_reads_as_plus_one_and_is_counted(label):
    """A byte image has no third value: on the path "split" a supplied 0.0 sign is +1.0, and the packing pass counts it."""
    from bayesian_torch_amd import rng
    m, x, draw, run = _replay_row(label, False, False, zero_rule=True)
    want = ROWS[label][-1]
    i_in, i_out = draw["sign_in"].numel() // 3 + 1, draw["sign_out"].numel() // 2 + 3
    plus, zero = dict(draw), dict(draw)
    for d, v in ((plus, 1.0), (zero, 0.0)):
        d["sign_in"], d["sign_out"] = draw["sign_in"].clone(), draw["sign_out"].clone()
        d["sign_in"].view(-1)[i_in] = v
        d["sign_out"].view(-1)[i_out] = v
    rng.set_inject_path("split")
    m.inject_draw = plus
    out_p, _, k_p = run()
    assert k_p == inj_name(want) and sign_counts(m._eps_pack) == [0, 0]
    m.inject_draw = zero
    out_z, _, k_z = run()
    assert k_z == inj_name(want)
    assert sign_counts(m._eps_pack) == [1, 1]
    assert torch.equal(out_z, out_p)
    # (the default path multiplies by the value it is given: a zero there removes the term)
    rng.set_inject_path("general")
    out_g, _, _ = run()
    assert not torch.equal(out_g, out_p)


# ------------------------------------------------------------------------------------------------ 5. reference goldens on the timed kernels
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
    """Run the oracle modules with the golden's per-sample seeds; collect logits and every layer's draws (CPU tensors)."""
    from bayesian_torch_amd.harness import resnet as H
    layers = [m for _, m in H.bayes_layers(ref)]
    logits, draws = [], [dict(eps_w=[], eps_b=[], sign_in=[], sign_out=[]) for _ in layers]
    with torch.no_grad():
        for s in range(meta["S"]):
            torch.manual_seed(meta["seed"] * 100 + s)
            logits.append(ref(x))
            for m, d in zip(layers, draws):
                d["eps_w"].append(getattr(m, "eps_" + m._wn).clone())
                if m.mu_bias is not None:
                    d["eps_b"].append(m.eps_bias.clone())
                d["sign_in"].append(m.last["sign_in"])
                d["sign_out"].append(m.last["sign_out"])
    stack = lambda lst: torch.stack(lst) if lst else None
    return torch.stack(logits), [{k: stack(v) for k, v in d.items()} for d in draws]


# model_r18_flipout (unfused, the golden's S = 1 and batch 128), on-chip draws: layers that report a bf16x3 kernel, of 21 -- what the
# on-chip dispatch of the commit before the injected Flipout instantiations existed selects (it is unchanged here): every layer but
# the three stride-2 3x3 ones, layer{2,3,4}.0.conv1. Asserted on the on-chip run below.
R18_FLIP_BF16X3_LAYERS = 18
# sign elements of the reference's draws (both tensors, all layers and samples): none of them is an exact zero
SIGN_ELEMENTS = {"model_r18_flipout": 12256512, "model_r18w8_flipout": 175992}


@pytest.mark.parametrize("name", ["model_r18w8_flipout", "model_r18_flipout"])
def test_model_goldens_on_the_split_kernels(name):
    """test_gpu_model.test_model_matches_reference_golden with the reference's draws and signs read by the kernels cfg4 is timed on:
    every layer's kernel is the twin of the one the same model reports with on-chip draws at the same S and batch; a layer on an
    fp32 kernel on chip replays on the general kernel."""
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
    n_sign = n_zero = 0
    for d in draws:      # the contract of the path: +-1 only
        for key in ("sign_in", "sign_out"):
            n_sign += d[key].numel()
            n_zero += int((d[key] == 0).sum())
            assert bool((d[key].abs() == 1).all()), (name, key)
    print(name, "sign elements:", n_sign, "zeros:", n_zero)
    assert n_zero == 0 and n_sign == SIGN_ELEMENTS[name], (n_sign, n_zero)
    draws = [{k: (None if v is None else v.cuda()) for k, v in d.items()} for d in draws]
    layers = [m for _, m in H.bayes_layers(net)]
    S = meta["S"]
    mc_forward(net, x.cuda(), S)      # on-chip draws: the kernels this model runs at this S and batch
    onchip = [m._last["kernel"] for m in layers]
    print(name, "on-chip kernels:", onchip)
    n_split = sum("bf16x3" in k for k in onchip)
    if name == "model_r18_flipout":
        assert len(onchip) == 21 and n_split == R18_FLIP_BF16X3_LAYERS, (n_split, onchip)
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
    assert all(sign_counts(m._eps_pack) == [0, 0] for m, k in zip(layers, got) if k.endswith(",inj>"))
    assert_close(logits.cpu(), g["logits"], 1e-4, 1e-5, name + ": split kernels (MC-batched) vs golden")
    assert_close(kl.cpu(), g["kl"], 1e-5, 0, name + ": fused KL vs golden")
    assert_close(get_kl_loss(net).cpu(), g["kl"], 1e-5, 0, name + ": get_kl_loss vs golden")
    with torch.no_grad():
        for s in range(S):
            for m, d in zip(layers, draws):
                m.inject_draw = {k: (v[s:s + 1] if v is not None else None) for k, v in d.items()}
            assert_close(net(x.cuda()).cpu(), g["logits"][s], 1e-4, 1e-5, f"{name}: sequential sample {s}")
            check_twins([m._last["kernel"] for m in layers], onchip1)


# the layer fixtures through the switch: where each lands (split kernel, or declined -> the general kernel, as under "general"); each
# entry is what the on-chip launch of that geometry reports (asserted below)
FIXTURE_LANDS = {
    "conv2d_flipout_c16x32k1s2nb": "general",
    "conv2d_flipout_c3x16k7s2": "split",
    "conv2d_flipout_c3x8k3": "general",
    "conv2d_flipout_c4x4k3d2": "general",
    "conv2d_flipout_c64x64k3hw1": "general",
    "conv2d_flipout_c6x10k3x2": "general",
    "conv2d_flipout_c8x12g2": "general",
    "conv2d_flipout_c8x16k3s2": "general",
    "linear_flipout_cfg1": "general",
    "linear_flipout_k500": "general",
    "linear_flipout_nobias": "general",
    "linear_flipout_rprior": "general",
}


def test_fixture_table_is_complete():
    assert sorted(FIXTURE_LANDS) == sorted(golden_names("linear_flipout_") + golden_names("conv2d_flipout_"))


@pytest.mark.parametrize("name", sorted(FIXTURE_LANDS))
def test_layer_fixtures_through_the_switch(name):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    g = layer_tensors(load_golden(name))
    c = lambda t: None if t is None else t.cuda()
    st = lambda t: None if t is None else t.cuda().unsqueeze(0)
    mu, rho = c(g["mu_w"]), c(g["rho_w"])
    assert bool((g["sign_in"].abs() == 1).all()) and bool((g["sign_out"].abs() == 1).all())
    packed = F.pack_params(mu, rho)
    F.fused_forward(c(g["x"]), mu, rho, c(g["mu_b"]), c(g["rho_b"]), flip=True, conv=g["conv"], S=1, packed=packed)
    onchip = _lib.lib().bt_last_kernel_name().decode()
    state = {}
    out, kl = F.fused_forward(c(g["x"]), mu, rho, c(g["mu_b"]), c(g["rho_b"]), flip=True, conv=g["conv"], S=1, want_kl=True,
                              priors=tuple(c(g[k]) for k in ("prior_mu_w", "prior_sigma_w", "prior_mu_b", "prior_sigma_b")),
                              eps_w=st(g["eps_w"]), eps_b=st(g["eps_b"]), sign_in=st(g["sign_in"]), sign_out=st(g["sign_out"]),
                              packed=packed, inject_path="split", eps_pack_state=state)
    kn = _lib.lib().bt_last_kernel_name().decode()
    print(name, "| on-chip:", onchip, "| split path:", kn)
    assert_close(out.cpu(), g["out"], 1e-4, 1e-5, name + ".out")
    assert_close(kl.cpu(), g["kl"], 1e-5, 0, name + ".kl")
    assert FIXTURE_LANDS[name] == ("split" if "bf16x3" in onchip else "general"), onchip
    if FIXTURE_LANDS[name] == "split":
        assert kn == inj_name(onchip) and not state["declined"] and sign_counts(state) == [0, 0], kn
    else:
        assert is_general_inj(kn) and len(state["declined"]) == 1, kn


# ------------------------------------------------------------------------------------------------ 6. fused model replay
def test_fused_model_replays_its_own_draws():
    """Flipout resnet18 converted and fuse_inference'd (folded BatchNorm / ReLU / residual adds, the stem's max-pool in its launch):
    on-chip -> materialise every layer's draw -> inject on the path "split"."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(3)
    net = H.resnet18(10, 64)
    dnn_to_bnn(net, dict(PRIOR, type="Flipout"))
    H.fill_bayes_params(net, 3)
    net = net.cuda().eval()
    H.fuse_inference(net)
    x = torch.randn(128, 3, 32, 32, generator=torch.Generator().manual_seed(8)).cuda()
    rng.manual_seed(99)
    logits, kl = mc_forward(net, x, 4)
    assert logits.shape == (4, 128, 10)
    named = list(H.bayes_layers(net))
    layers = [m for _, m in named]
    onchip = [m._last["kernel"] for m in layers]
    for m in layers:
        m.inject_draw = m.materialize_last_draw()
    rng.set_inject_path("split")
    logits1, kl1 = mc_forward(net, x, 4)
    got = [m._last["kernel"] for m in layers]
    check_twins(got, onchip)
    assert got[0] == "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=1,inj>", got[0]
    assert all(sign_counts(m._eps_pack) == [0, 0] for m, k in zip(layers, got) if k.endswith(",inj>"))
    rest = [(n, k) for (n, m), k in zip(named, onchip) if "bf16x3" not in k]
    if not rest:
        assert torch.equal(logits1, logits)
    else:      # the stride-2 3x3 layers stay on the fp32 kernels on chip, and their replay on the general kernel
        print("layers not on a split kernel on chip:", rest)
        for n, _ in rest:
            m = dict(named)[n]
            pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
            assert pair(m.kernel_size) == (3, 3) and pair(m.stride) == (2, 2), rest
        assert_close(logits1.cpu(), logits.cpu(), 1e-4, 1e-5, "split path")
    assert_close(kl1.cpu(), kl.cpu(), 1e-5, 0, "KL")


# ------------------------------------------------------------------------------------------------ 7. "torch" mode
@pytest.mark.parametrize("which", ["r18w8", "mlp"])
def test_torch_mode_through_the_switch(which):
    """rng.set_mode("torch"): the same torch.manual_seed gives the same draws on either path; the two paths are different arithmetic
    -- close, NOT bit-identical -- and the layers' eps_* buffers hold what the general path leaves in them."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(6)
    net = H.resnet18(10, 8) if which == "r18w8" else H.mlp((3072, 512, 10))
    dnn_to_bnn(net, dict(PRIOR, type="Flipout"))
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
    assert all(is_general_inj(k) for k in res["general"][1]), res["general"][1]
    split = [("bf16x3" in k and "flip" in k and k.endswith(",inj>")) for k in res["split"][1]]
    print(which, "split path kernels:", res["split"][1])
    assert sum(split) >= 1, res["split"][1]
    assert all(s or is_general_inj(k) for s, k in zip(split, res["split"][1]))
    counts = [sign_counts(m._eps_pack) for m, s in zip(layers, split) if s]
    assert all(c == [0, 0] for c in counts), f"a drawn sign was an exact zero ({counts}): pick another torch.manual_seed for this test"
    assert_close(res["split"][0].cpu(), res["general"][0].cpu(), 1e-4, 1e-5, which + ": split vs general")
    for a, b in zip(res["general"][2], res["split"][2]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    for a, b in zip(res["general"][3], res["split"][3]):
        assert (a is None and b is None) or torch.equal(a, b)
