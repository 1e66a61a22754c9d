"""GPU checks of the opt-in bf16 contraction mode (bt_set_contraction(3) / precision.contraction("bf16"); bt_fused_split_bf16.hip):
every operand value rounded ONCE to bf16 (nearest even), one MFMA term per K16 step, fp32 accumulate -- on the Reparameterization
launches that the automatic mode gives to the general split, stem or direct kernel, with the same plan.

The oracle is the project's fp64 C oracle evaluated on operands rounded on the host (torch's ``.bfloat16().float()`` is round to
nearest even): bf16 x bf16 products are exact in fp32 and the accumulation is the exact split's fp32 chain, so what remains is
fp32-accumulation error and the UNCHANGED tolerance (rtol 1e-4, atol 1e-5 max|ref|) holds. A truncating or double-rounding kernel
misses it by orders of magnitude. The sampled weight W_s = mu + sigma * eps is formed on the host in fp32 in the kernel's operation
order from the sigma = softplus(rho) the kernels read (the packed tensor of pack_params, held here to the host's fp32 softplus within
two ulps): with a softplus that differs in the last bit, about one weight in 2^16 lands on the other side of a bf16 rounding boundary,
and ONE such weight moves a whole output channel by a bf16 ulp of its products (~2^-8 |x w|, measured 1e-4 .. 2e-4 of max|ref| with
the host's own softplus) -- past the tolerance, although the kernel is right. Against the UNROUNDED oracle the distance is bounded per
element by 1.01 * 2^-8 * (|x| conv |W_s|) + atol, because (1 + 2^-9)^2 - 1 < 1.01 * 2^-8.

That last constant takes 2^-9 for the relative error of one rounding. It is the typical size, not the worst case: bf16 carries an 8-bit
significand, so round-to-nearest is off by up to 2^-8 of the value and a product of two rounded operands by up to
(1 + 2^-8)^2 - 1 < 1.01 * 2^-7. Over the K >= 24 products of the rows this file started with the errors average and the tighter constant
holds; they keep it. The depthwise row (SHORT_K: nine products per output, one input channel) has no such averaging: a correct kernel,
8.2e-8 of max|ref| from the oracle on rounded operands, exceeded the 2^-8 form at 10 of 12288 elements, by up to 8.0e-4 (MI355X). That
row is held to the worst-case constant; the check on rounded operands, which is what catches a truncating or double-rounding kernel, is
the same for every row."""
import ctypes
import zlib

import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
SEED, CALL, LAYER, SAMPLE0 = 77, 2, 9, 5

# Ci, Co, (kh, kw), stride, pad, dil, groups, H, W, B, S, bias -- rows of GEOMS in test_gpu_split.py
GENERAL = {
    "layer1 64x64 3x3 8x8 (512 tile, 9 taps)": (64, 64, (3, 3), 1, 1, 1, 1, 8, 8, 128, 2, False),
    "layer2 128x128 3x3 4x4 (256 tile)": (128, 128, (3, 3), 1, 1, 1, 1, 4, 4, 128, 2, False),
    "9 octets, partial channel tile, bias": (72, 40, (3, 3), 1, 1, 1, 1, 8, 8, 64, 1, True),
    "odd octet count, one tap": (24, 64, (1, 1), 1, 0, 1, 1, 8, 8, 16, 2, False),
    "layer4 512x512 3x3 on 1x1 maps (128 tile, 1 of 9 taps, xm=1)": (512, 512, (3, 3), 1, 1, 1, 1, 1, 1, 128, 2, False),
    "layer3 256x256 3x3 on 2x2 maps (row tiles, 6 of 9 taps, xm=2)": (256, 256, (3, 3), 1, 1, 1, 1, 2, 2, 128, 2, False),
    "14x14 maps 3x3 (W % 4 != 0: whole planes fetched flat)": (64, 64, (3, 3), 1, 1, 1, 1, 14, 14, 16, 2, True),
    "28x28 -> 14x14 1x1 s2 (every second column, XM 4)": (64, 128, (1, 1), 2, 0, 1, 1, 28, 28, 8, 2, True),
    "28x28 -> 14x14 3x3 s2 (strided window: row quads)": (32, 64, (3, 3), 2, 1, 1, 1, 28, 28, 8, 2, False),
    "groups 2, 3x2 kernel, stride (2,1)": (32, 48, (3, 2), (2, 1), (1, 0), 1, 2, 16, 9, 8, 1, True),
    # rows dw3 and cog70 of tests/_group_cases.py: grouped launches on the stem kernel (one live row of 64; a partial second channel tile)
    "depthwise 12 groups 3x3 8x8 (stem kernel, Cig 1, Cog 1)": (12, 12, (3, 3), 1, 1, 1, 12, 8, 8, 8, 2, True),
    "groups 2, 8->140 3x3 8x8 (stem kernel, Cig 4, Cog 70)": (8, 140, (3, 3), 1, 1, 1, 2, 8, 8, 8, 2, True),
}
# rows of DIRECT in test_gpu_round3.py (there: Ci, Co, groups, H, W, B, S, bias, extras[, stride]) in the layout above; EXTRAS below
DIRECT = {
    "K=256 -> 96 (partial channel tile), 7x7 (odd plane), b200, M % 64 != 0": (256, 96, (1, 1), 1, 0, 1, 1, 7, 7, 200, 1, True),
    "streamed W: K=1024 -> 96 (partial tile), 7x7, b180, ragged tiles": (1024, 96, (1, 1), 1, 0, 1, 1, 7, 7, 180, 1, False),
    "CIFAR downsample 64 -> 128, 1x1 s2, 8x8 -> 4x4, b128 (few pixels: one sub-tile per wave)": (64, 128, (1, 1), 2, 0, 1, 1, 8, 8, 128, 2, False),
}
# the stems: shared x (a model's input); the second one with the fused max-pool
STEMS = {
    "CIFAR stem 3->64 k7 s2 p3 on 32x32, B = 12, S = 2": (3, 64, (7, 7), 2, 3, 1, 1, 32, 32, 12, 2, False),
    "CIFAR stem 3->64 k7 s2 p3 on 32x32, B = 10, S = 3, shared x, pool": (3, 64, (7, 7), 2, 3, 1, 1, 32, 32, 10, 3, False),
}
ROWS = {**GENERAL, **DIRECT, **STEMS}
SHORT_K = {"depthwise 12 groups 3x3 8x8 (stem kernel, Cig 1, Cog 1)"}      # held to the worst-case rounding constant (module docstring)
EXTRAS = {"K=256 -> 96 (partial channel tile), 7x7 (odd plane), b200, M % 64 != 0", "streamed W: K=1024 -> 96 (partial tile), 7x7, b180, ragged tiles",
          "CIFAR downsample 64 -> 128, 1x1 s2, 8x8 -> 4x4, b128 (few pixels: one sub-tile per wave)"}      # DIRECT's rows carry an output stage there
FLIP_ROW = ("flip layer1 64x64 3x3 8x8 (row pieces, xm=3)", (64, 64, (3, 3), 1, 1, 1, 1, 8, 8, 128, 2, True))      # FLIP_GEOMS, test_gpu_split.py


_gpu = {}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _case(name, row=None):
    Ci, Co, k, st, pd, dl, grp, H, W, B, S, bias = row or ROWS[name]
    _gpu.clear()
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    mu = torch.randn(Co, Ci // grp, *k, generator=g) * 0.1
    rho = torch.randn(Co, Ci // grp, *k, generator=g) * 0.1 - 3
    mb = torch.randn(Co, generator=g) * 0.1 if bias else None
    rb = torch.randn(Co, generator=g) * 0.1 - 3 if bias else None
    shared = name in STEMS
    x = torch.randn(B if shared else S * B, Ci, H, W, generator=g)
    conv = dict(stride=_pair(st), padding=_pair(pd), dilation=_pair(dl), groups=grp)
    return dict(mu=mu, rho=rho, mb=mb, rb=rb, x=x, conv=conv, B=B, S=S, shared=shared, pool="pool" in name)


def _c(t):
    """One device copy per host tensor (cases are built once per test)."""
    if t is None:
        return None
    k = id(t)
    if k not in _gpu or _gpu[k][0] is not t:
        _gpu[k] = (t, t.cuda())
    return _gpu[k][1]


def _run(c, mode, S=None, x=None, shared=None, sample0=SAMPLE0, flip=False, **kw):
    """One launch of the case under contraction ``mode``: (out, kl, kernel name)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    L = _lib.lib()
    _lib.check(L.bt_set_contraction(mode))
    try:
        assert L.bt_get_contraction() == mode
        r = F._fused_forward(_c(c["x"] if x is None else x), _c(c["mu"]), _c(c["rho"]), _c(c["mb"]), _c(c["rb"]), flip=flip, conv=c["conv"],
                             S=c["S"] if S is None else S, shared_x=c["shared"] if shared is None else shared, seed=SEED, call=CALL, layer_id=LAYER,
                             sample0=sample0, packed=F.pack_params(_c(c["mu"]), _c(c["rho"])), pool=c["pool"], **kw)
        assert r is not None, "the fused max-pool was declined"
        return r[0], r[1], L.bt_last_kernel_name().decode()
    finally:
        L.bt_set_contraction(0)


def _draws(c):
    from bayesian_torch_amd import functional as F
    dev = torch.device("cuda")
    eps_w = F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 0, c["S"], c["mu"].shape, dev).cpu()
    eps_b = F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 1, c["S"], (c["mu"].shape[0],), dev).cpu() if c["mb"] is not None else None
    # sigma as the kernels read it: pack_params' [Co, taps, Ci padded to 4] back in the natural layout, anchored to the host's softplus
    Co, Ci = c["mu"].shape[:2]
    sig = F.pack_params(_c(c["mu"]), _c(c["rho"]))[1].cpu().reshape(Co, -1, (Ci + 3) // 4 * 4)[:, :, :Ci].permute(0, 2, 1).reshape(c["mu"].shape)
    host = torch.log1p(torch.exp(c["rho"]))
    assert float(((sig - host).abs() / host).max()) <= 5e-7, "packed sigma is not the fp32 softplus(rho)"
    return eps_w, eps_b, sig.contiguous()


def _bf16(t):
    return t.bfloat16().float()      # round to nearest even


def _images(B):
    """The images the CPU oracle evaluates: the first and the last 16 of the batch (the ragged last tile included)."""
    return sorted(set(range(min(B, 16))) | set(range(max(0, B - 16), B)))


def _oracles(c, s, eps_w, eps_b, sig, stage=None):
    """fp64 C oracle of sample s on the chosen images: (on rounded operands, on unrounded operands, on absolute values without bias).
    ``stage(ref64, image indices, s)`` applies an output stage in fp64."""
    from oracle import c_oracle as CO
    idx = _images(c["B"])
    xs = (c["x"] if c["shared"] else c["x"][s * c["B"]:(s + 1) * c["B"]])[idx]
    w_s = c["mu"] + sig * eps_w[s]      # fp32, the kernel's operation order: the product rounded, then the sum
    zero = torch.zeros_like(w_s)
    eb = None if eps_b is None else eps_b[s]
    rounded = CO.reparam_fwd(_bf16(xs), _bf16(w_s), c["rho"], zero, c["mb"], c["rb"], eb, c["conv"]).double()
    exact = CO.reparam_fwd(xs, c["mu"], c["rho"], eps_w[s], c["mb"], c["rb"], eb, c["conv"]).double()
    mag = CO.reparam_fwd(xs.abs(), w_s.abs(), c["rho"], zero, None, None, None, c["conv"]).double()
    if stage is not None:
        rounded, exact = stage(rounded, idx, s), stage(exact, idx, s)
    if c["pool"]:
        mp = lambda t: torch.nn.functional.max_pool2d(t, 3, 2, 1)
        rounded, exact, mag = mp(rounded), mp(exact), mp(mag)      # |max a - max b| <= max |a - b|: the bound pools with the window
    return idx, rounded, exact, mag


def _output_stage(c, seed, shift_scale):
    """BatchNorm constants, a residual and ReLU for the case: (launch keywords, the same stage in fp64, its effect on the error bound)."""
    g = torch.Generator().manual_seed(seed)
    Co, B = c["mu"].shape[0], c["B"]
    cv = c["conv"]
    Ho = (c["x"].shape[2] + 2 * cv["padding"][0] - cv["dilation"][0] * (c["mu"].shape[2] - 1) - 1) // cv["stride"][0] + 1
    Wo = (c["x"].shape[3] + 2 * cv["padding"][1] - cv["dilation"][1] * (c["mu"].shape[3] - 1) - 1) // cv["stride"][1] + 1
    sc, sh = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * shift_scale
    res = torch.randn(c["S"] * B, Co, Ho, Wo, generator=g)
    kw = dict(post_scale=sc.cuda(), post_shift=sh.cuda(), residual=res.cuda(), relu=True)
    sc64, sh64 = sc.double().view(1, -1, 1, 1), sh.double().view(1, -1, 1, 1)

    def stage(t, idx, s):
        return torch.relu(t * sc64 + sh64 + res[s * B:(s + 1) * B][idx].double())
    return kw, stage, lambda m: m * sc64      # |relu(a) - relu(b)| <= |a - b|, and the scale multiplies the distance


def _check_against_oracles(name, c, out3, stage=None, scale_mag=None):
    eps_w, eps_b, sig = _draws(c)
    o = out3.reshape((c["S"], c["B"]) + tuple(out3.shape[1:])).cpu()
    for s in range(c["S"]):
        idx, rounded, exact, mag = _oracles(c, s, eps_w, eps_b, sig, stage)
        got = o[s][idx]
        print(f"{name}[s={s}]: max |out - rounded oracle| / max|ref| = {float((got.double() - rounded).abs().max() / rounded.abs().max()):.3e}, "
              f"max |out - exact oracle| / max|ref| = {float((got.double() - exact).abs().max() / exact.abs().max()):.3e}")
        assert_close(got, rounded, RTOL, ATOL, f"{name}[s={s}] bf16 mode vs the oracle on rounded operands")
        if scale_mag is not None:
            mag = scale_mag(mag)
        lg = -7 if name in SHORT_K else -8
        bound = 1.01 * 2.0 ** lg * mag + ATOL * float(exact.abs().max())
        over = (got.double() - exact).abs() - bound
        assert float(over.max()) <= 0.0, f"{name}[s={s}]: {int((over > 0).sum())} elements past 1.01 * 2^{lg} * (|x| conv |W|) + atol, worst by {float(over.max()):.3e}"


# ------------------------------------------------------------------------------------------------ 1. rounded-operand oracle
@pytest.mark.parametrize("name", list(ROWS))
def test_bf16_mode_vs_oracle_on_rounded_operands(name):
    c = _case(name)
    kw = {}
    stage = scale_mag = None
    if name in EXTRAS:      # the direct rows' output stage (test_gpu_round3.py): BatchNorm constants, residual, ReLU
        kw, stage, scale_mag = _output_stage(c, 11, 0.1)
    out0, _, kn0 = _run(c, 0, **kw)
    out3, _, kn3 = _run(c, 3, **kw)
    assert "bf16x1" in kn3 and "1 terms" in kn3, (kn3, kn0)
    assert kn3.split("<")[0] == kn0.split("<")[0], (kn3, kn0)
    assert torch.isfinite(out3).all() and not torch.equal(out3, out0)
    _check_against_oracles(name, c, out3, stage, scale_mag)


# ------------------------------------------------------------------------------------------------ 2. canonical K order
def test_bf16_mode_is_independent_of_tiling_and_launch_split():
    """The scenario of test_split_kernel_is_independent_of_tiling_and_launch_split (test_gpu_split.py) in mode 3: a launch's plan is
    the automatic mode's, the K order canonical -- bit for bit the same numbers however the samples, the batch or x are split."""
    c = _case("layer1 64x64 3x3 8x8 (512 tile, 9 taps)")
    B = c["B"]
    x1 = c["x"][:B].contiguous()
    full, _, kn = _run(c, 3, S=16, x=x1, shared=True)
    assert "<64,512" in kn and "bf16x1" in kn, kn
    parts = []
    for s0 in range(0, 16, 2):
        o, _, kn2 = _run(c, 3, S=2, x=x1, shared=True, sample0=SAMPLE0 + s0)
        assert "fused_split_kernel" in kn2 and "<64,512" not in kn2 and "bf16x1" in kn2, kn2
        parts.append(o)
    assert torch.equal(torch.cat(parts), full)
    stacked, _, _ = _run(c, 3, S=2, x=torch.cat([x1, x1]), shared=False)
    assert torch.equal(stacked, full[:2 * B])
    part, _, kn3 = _run(c, 3, S=2, x=x1[:4].contiguous(), shared=True)
    assert "bf16x1" in kn3, kn3
    assert torch.equal(part.reshape(2, 4, -1), full.reshape(16, B, -1)[:2, :4])


# ------------------------------------------------------------------------------------------------ 3. direct == general
@pytest.mark.parametrize("name", ["K=256 -> 96 (partial channel tile), 7x7 (odd plane), b200, M % 64 != 0",
                                  "streamed W: K=1024 -> 96 (partial tile), 7x7, b180, ragged tiles"])
def test_bf16_direct_kernel_is_the_general_kernels_bits(name):
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    c = _case(name)
    out, _, kn = _run(c, 3)
    assert kn.startswith("fused_split_direct_kernel<") and "bf16x1" in kn and ("streamed" in kn) == (c["mu"].shape[1] > 256), kn
    L.bt_debug_disable_direct(1)
    try:
        ref, _, kn0 = _run(c, 3)
    finally:
        L.bt_debug_disable_direct(0)
    assert kn0.startswith("fused_split_kernel<") and "bf16x1" in kn0, kn0
    assert torch.equal(out, ref), f"{name}: {kn} differs from {kn0}: max abs {float((out - ref).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ 4. LDS hygiene
@pytest.mark.parametrize("name", ["9 octets, partial channel tile, bias", "CIFAR stem 3->64 k7 s2 p3 on 32x32, B = 10, S = 3, shared x, pool",
                                  "K=256 -> 96 (partial channel tile), 7x7 (odd plane), b200, M % 64 != 0"])
def test_bf16_kernels_never_read_lds_they_did_not_write(name):
    """LDS survives from kernel to kernel: NaN patterns in all of it right before the launch -- finite, and the same bits."""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(4, dtype=torch.int32, device="cuda")
    c = _case(name)
    clean, _, kn = _run(c, 3)
    assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0
    dirty, _, kn2 = _run(c, 3)
    assert "bf16x1" in kn and kn2 == kn, (kn, kn2)
    assert torch.isfinite(dirty).all() and torch.equal(clean, dirty), (name, kn)


# ------------------------------------------------------------------------------------------------ 5. KL and output stage
def test_bf16_mode_keeps_kl_and_output_stage():
    name = "layer1 64x64 3x3 8x8 (512 tile, 9 taps)"
    c = _case(name)
    kw, stage, scale_mag = _output_stage(c, 3, 1.0)
    pri = (torch.zeros_like(c["mu"]).cuda(), torch.ones_like(c["mu"]).cuda(), None, None)
    kw.update(priors=pri, want_kl=True, workspace_owner="t_bf16")
    out0, kl0, kn0 = _run(c, 0, **kw)
    out3, kl3, kn3 = _run(c, 3, **kw)
    assert "bf16x3" in kn0 and "bf16x1" in kn3, (kn0, kn3)
    assert torch.equal(kl3, kl0) and float(kl3) > 0
    assert (out3 >= 0).all() and (out3 == 0).any() and not torch.equal(out3, out0)
    _check_against_oracles(name, c, out3, stage, scale_mag)


# ------------------------------------------------------------------------------------------------ 6. what must not change
def test_bf16_mode_leaves_flipout_and_injected_draws_alone():
    from bayesian_torch_amd import functional as F
    c = _case(*FLIP_ROW)
    out0, _, kn0 = _run(c, 0, flip=True)
    out3, _, kn3 = _run(c, 3, flip=True)
    assert "fused_split_kernel" in kn0 and "flip" in kn0 and kn3 == kn0, (kn0, kn3)
    assert torch.equal(out3, out0)
    # natural-layout injected draws: the fp32 general kernel, as in the automatic mode
    c = _case("layer1 64x64 3x3 8x8 (512 tile, 9 taps)")
    eps = F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 0, c["S"], c["mu"].shape, torch.device("cuda"))
    outs = {}
    for mode in (0, 3):
        outs[mode], _, kn = _run(c, mode, eps_w=eps, inject_path="general")
        assert kn.startswith("fused_fwd_kernel<") and "inj=1" in kn, (mode, kn)
    assert torch.equal(outs[3], outs[0])


# ------------------------------------------------------------------------------------------------ 7. a model through the Python API
def test_bf16_mode_on_a_fused_model_through_the_python_api():
    from bayesian_torch_amd import precision, rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "moped_enable": False, "moped_delta": 0.5}
    torch.manual_seed(1)
    net = H.resnet18(10, 64)
    dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
    H.fill_bayes_params(net, 5)
    net = net.cuda().eval()
    H.fuse_inference(net)
    x = torch.randn(64, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    rng.set_mode("philox")
    rng.manual_seed(11)
    c0 = rng.peek_call()
    layers = [m for _, m in H.bayes_layers(net)]

    def run():
        rng.set_call(c0)
        logits, kl = mc_forward(net, x, 2)
        return logits, kl, [m._last["kernel"] for m in layers]
    assert precision.get_contraction() == "auto"
    l0, kl0, k0 = run()
    with precision.contraction("bf16"):
        assert precision.get_contraction() == "bf16"
        l3, kl3, k3 = run()
    assert precision.get_contraction() == "auto"
    served = {"fused_split_kernel", "fused_split_quad_kernel", "fused_split_direct_kernel"}
    want = {i for i, k in enumerate(k0) if k.split("<")[0] in served}
    got = {i for i, k in enumerate(k3) if "bf16x1" in k}
    assert want and got == want, ([k0[i] for i in sorted(want ^ got)], [k3[i] for i in sorted(want ^ got)])
    # (a launch the automatic mode gives the split-K kernel has no bf16 twin: it runs on whatever else takes it, here fp32 MFMA)
    assert all(k3[i] == k0[i] for i in range(len(k0)) if i not in want and "skinny" not in k0[i])
    assert torch.isfinite(l3).all() and l3.shape == l0.shape
    assert torch.equal(kl3, kl0)
    l0b, kl0b, k0b = run()
    assert torch.equal(l0b, l0) and torch.equal(kl0b, kl0) and k0b == k0      # the mode leaves no state behind
    print(f"resnet18(10, 64) b64 S=2, {len(want)} of {len(k0)} layers in the bf16 mode: max|dlogit| / max|logit| = "
          f"{float((l3 - l0).abs().max() / l0.abs().max()):.3e}")
