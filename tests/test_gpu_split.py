"""GPU parity of the split-precision flavour (bt_fused_split.h: fp32 operands as exact bf16x3 pieces, 6 product terms on
the bf16 matrix pipe, fp32 accumulate): on-chip draws replayed through the plain-C oracle (fp64 accumulation) at the
UNCHANGED tolerances, its error next to the fp32-MFMA kernel's on the same draws, and its independence of tile choice,
launch split and batch size (canonical K order)."""
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5

# Ci, Co, (kh, kw), stride, pad, dil, groups, H, W, B, S, bias
GEOMS = {
    "layer1 64x64 3x3 8x8 (512 tile, 9 taps)": (64, 64, (3, 3), 1, 1, 1, 1, 8, 8, 128, 2, False),
    "layer2 128x128 3x3 4x4 (256 tile)": (128, 128, (3, 3), 1, 1, 1, 1, 4, 4, 128, 2, False),
    "layer2.0 64->128 3x3 s2": (64, 128, (3, 3), 2, 1, 1, 1, 8, 8, 128, 2, False),
    "downsample 64->128 1x1 s2 (one tap: octet pairs)": (64, 128, (1, 1), 2, 0, 1, 1, 8, 8, 128, 2, False),
    "bottleneck 256->64 1x1 16x16": (256, 64, (1, 1), 1, 0, 1, 1, 16, 16, 8, 1, True),
    "row bands 64x64 3x3 56x56": (64, 64, (3, 3), 1, 1, 1, 1, 56, 56, 2, 1, True),
    "9 octets, partial channel tile, bias": (72, 40, (3, 3), 1, 1, 1, 1, 8, 8, 64, 1, True),
    "odd octet count, one tap": (24, 64, (1, 1), 1, 0, 1, 1, 8, 8, 16, 2, False),
    "dilation 2": (16, 32, (3, 3), 1, 2, 2, 1, 16, 16, 8, 1, True),
    "groups 2, 3x2 kernel, stride (2,1)": (32, 48, (3, 2), (2, 1), (1, 0), 1, 2, 16, 9, 8, 1, True),
    "K = 4608 (512x512 3x3 on 4x4)": (512, 64, (3, 3), 1, 1, 1, 1, 4, 4, 32, 1, False),
    "layer4 512x512 3x3 on 1x1 maps (128 tile, 1 of 9 taps, xm=1)": (512, 512, (3, 3), 1, 1, 1, 1, 1, 1, 128, 2, False),
    "layer3 256x256 3x3 on 2x2 maps (row tiles, 6 of 9 taps, xm=2)": (256, 256, (3, 3), 1, 1, 1, 1, 2, 2, 128, 2, False),
    "layer3.0.conv1 128->256 3x3 s2 4x4->2x2 (pixel-major, generic fetch)": (128, 256, (3, 3), 2, 1, 1, 1, 4, 4, 128, 2, True),
    "layer4.0.downsample 256->512 1x1 s2 2x2->1x1": (256, 512, (1, 1), 2, 0, 1, 1, 2, 2, 128, 2, False),
    "1x1 maps, partial batch tile (B = 120)": (64, 96, (3, 3), 1, 1, 1, 1, 1, 1, 120, 1, True),
    "14x14 maps 3x3 (W % 4 != 0: whole planes fetched flat)": (64, 64, (3, 3), 1, 1, 1, 1, 14, 14, 16, 2, True),
    "14x14 maps 1x1 256->64 (flat planes, one tap)": (256, 64, (1, 1), 1, 0, 1, 1, 14, 14, 8, 2, False),
    "28x28 -> 14x14 1x1 s2 (every second column, XM 4)": (64, 128, (1, 1), 2, 0, 1, 1, 28, 28, 8, 2, True),
    "28x28 -> 14x14 3x3 s2 (strided window: row quads)": (32, 64, (3, 3), 2, 1, 1, 1, 28, 28, 8, 2, False),
}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


# the tile a case's label names, as bt_last_launch_info reports its automatic-mode launch (2x2 maps: row tiles for
# Reparameterization; Flipout's pixel-major patch of 128 images does not fit, so whole images)
LABELLED_TILES = {"layer3 256x256 3x3 on 2x2 maps (row tiles, 6 of 9 taps, xm=2)": dict(row_tiles=1, pixel_major=0),
                  "flip layer3 256x256 3x3 on 2x2 maps (128 tile of whole images)": dict(row_tiles=0, pixel_major=0, t_R=2, t_Wt=2)}


def _check_labelled_tile(name, kn):
    from bayesian_torch_amd import _lib
    want = LABELLED_TILES.get(name, {})
    li = _lib.last_launch_info()
    assert {k: li[k] for k in want} == want, (name, kn, li)


def _case(name):
    Ci, Co, k, st, pd, dl, grp, H, W, B, S, bias = GEOMS[name]
    g = torch.Generator().manual_seed(abs(hash(name)) % (1 << 31))
    mu = torch.randn(Co, Ci // grp, *k, generator=g) * 0.1
    rho = torch.randn(Co, Ci // grp, *k, generator=g) * 0.1 - 3
    mb = torch.randn(Co, generator=g) * 0.1 if bias else None
    rb = torch.randn(Co, generator=g) * 0.1 - 3 if bias else None
    x = torch.randn(S * B, Ci, H, W, generator=g)
    conv = dict(stride=_pair(st), padding=_pair(pd), dilation=_pair(dl), groups=grp)
    return mu, rho, mb, rb, x, conv, B, S


def _run(mu, rho, mb, rb, x, conv, S, mode, sample0=5, shared=False):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    c = lambda t: None if t is None else t.cuda()
    _lib.check(_lib.lib().bt_set_contraction(mode))
    try:
        out, _ = F.fused_forward(c(x), c(mu), c(rho), c(mb), c(rb), conv=conv, S=S, shared_x=shared, seed=77, call=2, layer_id=9, sample0=sample0,
                                 packed=F.pack_params(c(mu), c(rho)))
        name = _lib.lib().bt_last_kernel_name().decode()
    finally:
        _lib.lib().bt_set_contraction(0)
    return out, name


@pytest.mark.parametrize("name", list(GEOMS))
def test_split_kernel_vs_c_oracle_and_fp32_kernel(name):
    from oracle import c_oracle as CO
    from bayesian_torch_amd import functional as F
    mu, rho, mb, rb, x, conv, B, S = _case(name)
    out, kn = _run(mu, rho, mb, rb, x, conv, S, 0)
    if "s2" in name and "3x3" in name:     # strided 3x3: the patch holds every input pixel (4x the outputs); small tiles stay on the fp32 kernel
        if "fused_split_kernel" not in kn:
            pytest.skip("not eligible for the split flavour at this size: " + kn)
    # (1x1 layers with K <= 256: the direct kernel; narrow one-pixel heads: the split-K kernel)
    assert ("fused_split_kernel" in kn or "fused_split_direct_kernel" in kn or "fused_split_skinny_kernel" in kn) and "6 terms" in kn, kn
    _check_labelled_tile(name, kn)
    out32, kn32 = _run(mu, rho, mb, rb, x, conv, S, 1)
    assert "split" not in kn32, kn32
    dev = torch.device("cuda")
    eps_w = F.rng_fill_normal(77, 2, 9, 5, 0, S, mu.shape, dev).cpu()
    eps_b = F.rng_fill_normal(77, 2, 9, 5, 1, S, (mu.shape[0],), dev).cpu() if mb is not None else None
    out, out32 = out.reshape((S, B) + tuple(out.shape[1:])).cpu(), out32.reshape((S, B) + tuple(out.shape[1:])).cpu()
    worst = 0.0
    for s in range(S):
        ref = CO.reparam_fwd(x[s * B:(s + 1) * B], mu, rho, eps_w[s], mb, rb, None if eps_b is None else eps_b[s], conv)
        assert_close(out[s], ref, RTOL, ATOL, f"{name}[s={s}] split vs C oracle")
        scale = float(ref.abs().max())
        e_split = float((out[s].double() - ref.double()).abs().max()) / scale
        e_f32 = float((out32[s].double() - ref.double()).abs().max()) / scale
        worst = max(worst, e_split / max(e_f32, 1e-9))
        # the exact split is fp32-grade: no worse than 4x the fp32-MFMA kernel's error on the same draws (+ one fp32 ulp of slack)
        assert e_split <= 4.0 * e_f32 + 1.2e-7, (name, s, e_split, e_f32)
    print(f"{name}: split/f32 error ratio {worst:.2f}")


def test_split_kernel_is_independent_of_tiling_and_launch_split():
    """Canonical K order: the same global samples in one launch (512-wide tiles) or in eight launches of two (narrower
    tiles: fewer workgroups), a whole batch or its first rows (another tile geometry), shared or stacked x -- bit for bit
    the same numbers."""
    mu, rho, mb, rb, x, conv, B, S = _case("layer1 64x64 3x3 8x8 (512 tile, 9 taps)")
    x1 = x[:B]                                          # one batch shared by all samples
    full, kn = _run(mu, rho, None, None, x1, conv, 16, 0, shared=True)
    assert "<64,512" in kn, kn
    parts = []
    for s0 in range(0, 16, 2):
        o, kn2 = _run(mu, rho, None, None, x1, conv, 2, 0, sample0=5 + s0, shared=True)
        assert "fused_split_kernel" in kn2 and "<64,512" not in kn2, kn2     # fewer workgroups: a narrower tile
        parts.append(o)
    assert torch.equal(torch.cat(parts), full)
    stacked, _ = _run(mu, rho, None, None, torch.cat([x1, x1]), conv, 2, 0)
    assert torch.equal(stacked, full[:2 * B])
    part, kn3 = _run(mu, rho, None, None, x1[:4].contiguous(), conv, 2, 0, shared=True)     # 4 images per sample
    assert "split" in kn3, kn3
    assert torch.equal(part.reshape(2, 4, -1), full.reshape(16, B, -1)[:2, :4])


def test_three_term_split_is_opt_in_and_coarser():
    from oracle import c_oracle as CO
    from bayesian_torch_amd import functional as F
    mu, rho, mb, rb, x, conv, B, S = _case("layer1 64x64 3x3 8x8 (512 tile, 9 taps)")
    out3, kn = _run(mu, rho, None, None, x, conv, S, 2)
    assert "3 terms" in kn
    eps_w = F.rng_fill_normal(77, 2, 9, 5, 0, S, mu.shape, torch.device("cuda")).cpu()
    ref = CO.reparam_fwd(x[:B], mu, rho, eps_w[0], None, None, None, conv)
    err = float((out3[:B].cpu().double() - ref.double()).abs().max() / ref.abs().max())
    assert 1e-7 < err < 2e-4, err      # documented: ~1e-5 relative; NOT held to the parity tolerance


def test_model_level_parity_with_split_kernels():
    """ResNet18 width 64 at CIFAR size (the bench's kernels): on-chip draws through the oracle, and split == fp32 path
    within the layer tolerance on the same draws."""
    from oracle import bt_oracle as O
    from bayesian_torch_amd import _lib, rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "moped_enable": False, "moped_delta": 0.5}
    torch.manual_seed(1)
    ref = H.resnet18(10, 64)
    O.ref_dnn_to_bnn(ref, "Reparameterization")
    H.fill_bayes_params(ref, 5)
    net = H.resnet18(10, 64)
    dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
    H.fill_bayes_params(net, 5)
    ref, net = ref.eval(), net.cuda().eval()
    x = torch.randn(64, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    rng.set_mode("philox")
    rng.manual_seed(11)
    c0 = rng.peek_call()
    logits, kl = mc_forward(net, x.cuda(), 2)
    used = {m._last["kernel"].split("<")[0] for _, m in H.bayes_layers(net)}
    assert "fused_split_kernel" in used, used
    draws = [m.materialize_last_draw() for _, m in H.bayes_layers(net)]
    with torch.no_grad():
        for s in range(2):
            for (_, rm), d in zip(H.bayes_layers(ref), draws):
                rm.inject = {k: v[s].cpu() for k, v in d.items()}
            assert_close(logits[s].cpu(), ref(x), RTOL, ATOL, f"split model sample {s}")
    _lib.lib().bt_set_contraction(1)
    try:
        rng.set_call(c0)
        l32, kl32 = mc_forward(net, x.cuda(), 2)
    finally:
        _lib.lib().bt_set_contraction(0)
    assert_close(logits.cpu(), l32.cpu(), RTOL, ATOL, "split vs fp32 kernels, same draws")
    assert float(kl) == float(kl32)


@pytest.mark.parametrize("In,Out,B,S,bias", [(512, 10, 128, 2, True), (3072, 512, 256, 1, True), (520, 40, 128, 1, False)])
def test_linear_layers_on_the_split_kernel(In, Out, B, S, bias):
    """LinearReparameterization == a 1x1 convolution over 1x1 images (cfg2's MLP, the ResNet heads)."""
    from oracle import c_oracle as CO
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    g = torch.Generator().manual_seed(In + Out)
    mu, rho = torch.randn(Out, In, generator=g) * 0.1, torch.randn(Out, In, generator=g) * 0.1 - 3
    mb = torch.randn(Out, generator=g) * 0.1 if bias else None
    rb = torch.randn(Out, generator=g) * 0.1 - 3 if bias else None
    x = torch.randn(B, In, generator=g)
    c = lambda t: None if t is None else t.cuda()
    out, _ = F.fused_forward(c(x), c(mu), c(rho), c(mb), c(rb), S=S, seed=3, call=1, layer_id=4, sample0=2, packed=F.pack_params(c(mu), c(rho)))
    kn = _lib.lib().bt_last_kernel_name().decode()
    assert "fused_split_kernel" in kn or "fused_split_direct_kernel" in kn or "fused_split_skinny_kernel" in kn, kn
    dev = torch.device("cuda")
    eps_w = F.rng_fill_normal(3, 1, 4, 2, 0, S, mu.shape, dev).cpu()
    eps_b = F.rng_fill_normal(3, 1, 4, 2, 1, S, (Out,), dev).cpu() if bias else None
    out = out.reshape(S, B, Out).cpu()
    for s in range(S):
        ref = CO.reparam_fwd(x, mu, rho, eps_w[s], mb, rb, None if eps_b is None else eps_b[s], None)
        assert_close(out[s], ref, RTOL, ATOL, f"linear {In}->{Out} sample {s}")


def test_fp32_kernel_repeatability_on_a_padded_channel_chunk():
    """24 input channels (a channel chunk padded to 32) on the fp32 kernels, interleaved with split-kernel launches on the
    same CUs: identical, finite results every time. Regression: the fp32 fast kernel left the K rows of channel quads past
    Cig4 unwritten, and stale LDS (a NaN pattern) times a zero activation is a NaN."""
    mu, rho, mb, rb, x, conv, B, S = _case("odd octet count, one tap")
    first = None
    for it in range(12):
        if it % 2 == 0:
            _run(mu, rho, mb, rb, x, conv, S, 0)      # leaves bf16 pieces (NaN patterns, read as fp32) behind in the CUs' LDS
        out, kn = _run(mu, rho, mb, rb, x, conv, S, 1)
        assert "split" not in kn
        assert torch.isfinite(out).all(), "non-finite output from " + kn
        first = out if first is None else first
        assert torch.equal(out, first)


STEMS = {
    "CIFAR ResNet stem 3->64 7x7 s2 on 32x32": (3, 64, (7, 7), 2, 3, 32, 32, 12, 2, False),
    "4 channels, 5x5 s1, bias, 40 output channels": (4, 40, (5, 5), 1, 2, 16, 16, 6, 1, True),
    "1 channel, 3x3": (1, 64, (3, 3), 1, 1, 16, 16, 4, 2, True),
    "2 channels, 7x7 s2 on 64x64 (one image per tile)": (2, 64, (7, 7), 2, 3, 32, 32, 3, 1, False),
    "ImageNet-style stem 3->64 7x7 s2 on 96x96 (bands of 10 rows of 48)": (3, 64, (7, 7), 2, 3, 96, 96, 2, 2, True),
    "3 channels, 3x3 s1 on 40x40 (bands of 12 rows, last band ragged)": (3, 32, (3, 3), 1, 1, 40, 40, 3, 1, False),
}


@pytest.mark.parametrize("name", list(STEMS))
def test_stem_kernel_vs_c_oracle(name):
    """<= 4 input channels: the quad flavour (bt_fused_split_quad.h: two taps per k-group, patch staged once, tap chunks)."""
    from oracle import c_oracle as CO
    from bayesian_torch_amd import functional as F
    Ci, Co, k, st, pd, H, W, B, S, bias = STEMS[name]
    g = torch.Generator().manual_seed(abs(hash(name)) % (1 << 31))
    mu, rho = torch.randn(Co, Ci, *k, generator=g) * 0.1, torch.randn(Co, Ci, *k, generator=g) * 0.1 - 3
    mb = torch.randn(Co, generator=g) * 0.1 if bias else None
    rb = torch.randn(Co, generator=g) * 0.1 - 3 if bias else None
    x = torch.randn(B, Ci, H, W, generator=g)                     # shared by the samples, like a model's input
    conv = dict(stride=(st, st), padding=(pd, pd), dilation=(1, 1), groups=1)
    out, kn = _run(mu, rho, mb, rb, x, conv, S, 0, shared=True)
    assert "fused_split_quad_kernel" in kn, kn
    out32, kn32 = _run(mu, rho, mb, rb, x, conv, S, 1, shared=True)
    assert "split" not in kn32
    dev = torch.device("cuda")
    eps_w = F.rng_fill_normal(77, 2, 9, 5, 0, S, mu.shape, dev).cpu()
    eps_b = F.rng_fill_normal(77, 2, 9, 5, 1, S, (Co,), dev).cpu() if bias else None
    out, out32 = out.reshape((S, B) + tuple(out.shape[1:])).cpu(), out32.reshape((S, B) + tuple(out.shape[1:])).cpu()
    for s in range(S):
        ref = CO.reparam_fwd(x, mu, rho, eps_w[s], mb, rb, None if eps_b is None else eps_b[s], conv)
        assert_close(out[s], ref, RTOL, ATOL, f"{name}[s={s}] quad vs C oracle")
        scale = float(ref.abs().max())
        e_split = float((out[s].double() - ref.double()).abs().max()) / scale
        e_f32 = float((out32[s].double() - ref.double()).abs().max()) / scale
        assert e_split <= 4.0 * e_f32 + 1.2e-7, (name, s, e_split, e_f32)
    # launch-split independence
    a, _ = _run(mu, rho, mb, rb, x, conv, 1, 0, sample0=5 + S - 1, shared=True)
    assert torch.equal(a.cpu().reshape(out[S - 1].shape), out[S - 1])


def test_stem_kernel_fused_maxpool():
    """conv -> scale/shift -> ReLU -> MaxPool2d(3, 2, 1) in the quad kernel's output stage == max_pool2d of its unpooled launch."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    g = torch.Generator().manual_seed(5)
    mu, rho = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).cuda(), (torch.randn(64, 3, 7, 7, generator=g) * 0.1 - 3).cuda()
    sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.3).cuda()
    x = torch.randn(10, 3, 32, 32, generator=g).cuda()
    conv = dict(stride=(2, 2), padding=(3, 3), dilation=(1, 1), groups=1)
    kw = dict(conv=conv, S=3, seed=5, call=1, layer_id=4, sample0=0, packed=F.pack_params(mu, rho), post_scale=sc, post_shift=sh, relu=True)
    pooled = F._fused_forward(x, mu, rho, pool=True, **kw)
    assert pooled is not None and "fused_split_quad_kernel" in _lib.lib().bt_last_kernel_name().decode() and "pool=1" in _lib.lib().bt_last_kernel_name().decode()
    full, _ = F.fused_forward(x, mu, rho, **kw)
    assert "pool=0" in _lib.lib().bt_last_kernel_name().decode()
    assert tuple(pooled[0].shape) == (30, 64, 8, 8)
    assert torch.equal(pooled[0], torch.nn.functional.max_pool2d(full, 3, 2, 1))


# ---------------------------------------------------------------------------------------------------------------- Flipout
# Flipout on the split flavour (FLIP = true: two weight images, sign masks next to the x pieces, 64 x 256 tile).
FLIP_GEOMS = {
    "flip layer1 64x64 3x3 8x8 (row pieces, xm=3)": (64, 64, (3, 3), 1, 1, 1, 1, 8, 8, 128, 2, True),
    "flip layer2 128x128 3x3 4x4": (128, 128, (3, 3), 1, 1, 1, 1, 4, 4, 128, 2, False),
    "flip 1x1 bottleneck 64->256 8x8 (one tap: octet pairs)": (64, 256, (1, 1), 1, 0, 1, 1, 8, 8, 64, 2, True),
    "flip row bands 16x32 3x3 28x28, ragged channels": (16, 40, (3, 3), 1, 1, 1, 1, 28, 28, 4, 1, True),
    "flip W % 4 != 0 (generic fetch) 24x64 3x3 6x6": (24, 64, (3, 3), 1, 1, 1, 1, 6, 6, 64, 2, True),
    "flip layer3 256x256 3x3 on 2x2 maps (128 tile of whole images)": (256, 256, (3, 3), 1, 1, 1, 1, 2, 2, 128, 2, False),
    "flip layer4 512x512 3x3 on 1x1 maps (128 tile, one tap, xm=1)": (512, 512, (3, 3), 1, 1, 1, 1, 1, 1, 128, 2, True),
    "flip layer3.0.conv1 128->256 3x3 s2 4x4->2x2 (pixel-major, generic fetch)": (128, 256, (3, 3), 2, 1, 1, 1, 4, 4, 128, 2, True),
    "flip layer4.0.downsample 256->512 1x1 s2 2x2->1x1 (one tap)": (256, 512, (1, 1), 2, 0, 1, 1, 2, 2, 128, 2, False),
    "flip small batch 64x64 3x3 4x4, B = 16 (128 tile of whole images)": (64, 64, (3, 3), 1, 1, 1, 1, 4, 4, 16, 8, True),
    "flip groups 2, dilation 2": (32, 64, (3, 3), 1, 2, 2, 2, 8, 8, 32, 1, True),
}


def _flip_case(name):
    GEOMS[name] = FLIP_GEOMS[name]
    try:
        return _case(name)
    finally:
        del GEOMS[name]


def _run_flip(mu, rho, mb, rb, x, conv, S, mode, sample0=5, **kw):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    c = lambda t: None if t is None else t.cuda()
    _lib.check(_lib.lib().bt_set_contraction(mode))
    try:
        out, kl = F.fused_forward(c(x), c(mu), c(rho), c(mb), c(rb), flip=True, conv=conv, S=S, shared_x=False, seed=77, call=2, layer_id=9,
                                  sample0=sample0, packed=F.pack_params(c(mu), c(rho)), **kw)
        name = _lib.lib().bt_last_kernel_name().decode()
    finally:
        _lib.lib().bt_set_contraction(0)
    return out, kl, name


@pytest.mark.parametrize("name", list(FLIP_GEOMS))
def test_split_flipout_vs_c_oracle_and_fp32_kernel(name):
    """On-chip draws and signs replayed through the plain-C oracle (fp64 accumulation) at the unchanged tolerances; the split
    kernel's error next to the fp32-MFMA Flipout kernel's on the same draws."""
    from oracle import c_oracle as CO
    from bayesian_torch_amd import functional as F
    mu, rho, mb, rb, x, conv, B, S = _flip_case(name)
    out, _, kn = _run_flip(mu, rho, mb, rb, x, conv, S, 0)
    if ("one tap" in name or "3x3 s2" in name) and "fused_split_kernel" not in kn:
        # a single tap pairs consecutive octets in one MFMA step: two octet planes per stage, 150 pixels each; a strided 3x3 reads
        # 4x the pixels it writes: such patches may not fit the 301 pixels the two weight images leave
        pytest.skip("not eligible for the split Flipout: " + kn)
    assert "fused_split_kernel" in kn and "flip" in kn, kn
    _check_labelled_tile(name, kn)
    out32, _, kn32 = _run_flip(mu, rho, mb, rb, x, conv, S, 1)
    assert "split" not in kn32 and "flip" in kn32, kn32
    dev = torch.device("cuda")
    eps_w = F.rng_fill_normal(77, 2, 9, 5, 0, S, mu.shape, dev).cpu()
    eps_b = F.rng_fill_normal(77, 2, 9, 5, 1, S, (mu.shape[0],), dev).cpu() if mb is not None else None
    oshape = tuple(out.shape[1:])
    s_in = F.rng_fill_sign(77, 2, 9, 5, 2, S, (B,) + tuple(x.shape[1:]), dev).cpu()
    s_out = F.rng_fill_sign(77, 2, 9, 5, 3, S, (B,) + oshape, dev).cpu()
    out, out32 = out.reshape((S, B) + oshape).cpu(), out32.reshape((S, B) + oshape).cpu()
    worst = 0.0
    for s in range(S):
        ref = CO.flipout_fwd(x[s * B:(s + 1) * B], mu, rho, eps_w[s], s_in[s], s_out[s], mb, rb, None if eps_b is None else eps_b[s], conv)
        assert_close(out[s], ref, RTOL, ATOL, f"{name}[s={s}] split flipout vs C oracle")
        scale = float(ref.abs().max())
        e_split = float((out[s].double() - ref.double()).abs().max()) / scale
        e_f32 = float((out32[s].double() - ref.double()).abs().max()) / scale
        worst = max(worst, e_split / max(e_f32, 1e-9))
        assert e_split <= 4.0 * e_f32 + 1.2e-7, (name, s, e_split, e_f32)
    print(f"{name}: split/f32 error ratio {worst:.2f}")


def test_split_flipout_output_stage_and_kl():
    """BatchNorm constants, residual and ReLU behind the sign-combined sum, KL in the same launch: equal to the fp32 Flipout
    kernel's (same order of operations) within the contraction's rounding, KL bit for bit."""
    mu, rho, mb, rb, x, conv, B, S = _flip_case("flip layer1 64x64 3x3 8x8 (row pieces, xm=3)")
    g = torch.Generator().manual_seed(3)
    sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), torch.randn(64, generator=g).cuda()
    res = torch.randn(S * B, 64, 8, 8, generator=g).cuda()
    pri = (torch.zeros_like(mu).cuda(), torch.ones_like(mu).cuda(), torch.zeros_like(mb).cuda(), torch.ones_like(mb).cuda())
    kw = dict(post_scale=sc, post_shift=sh, residual=res, relu=True, priors=pri, want_kl=True)
    out, kl, kn = _run_flip(mu, rho, mb, rb, x, conv, S, 0, **kw)
    assert "fused_split_kernel" in kn and "flip" in kn, kn
    out32, kl32, kn32 = _run_flip(mu, rho, mb, rb, x, conv, S, 1, **kw)
    assert "split" not in kn32
    assert torch.equal(kl, kl32)
    assert (out >= 0).all() and (out == 0).any()
    assert_close(out.cpu(), out32.cpu(), 1e-5, 1e-5, "split flipout vs fp32 flipout, fused output stage")


def test_split_flipout_is_independent_of_launch_split():
    mu, rho, mb, rb, x, conv, B, S = _flip_case("flip layer1 64x64 3x3 8x8 (row pieces, xm=3)")
    x4 = torch.cat([x, x])     # 4 samples' batches
    full, _, kn = _run_flip(mu, rho, mb, rb, x4, conv, 4, 0)
    assert "flip" in kn and "split" in kn, kn
    a, _, _ = _run_flip(mu, rho, mb, rb, x4[:2 * B], conv, 2, 0, sample0=5)
    b, _, _ = _run_flip(mu, rho, mb, rb, x4[2 * B:], conv, 2, 0, sample0=7)
    assert torch.equal(torch.cat([a, b]), full)


FLIP_STEMS = {
    "flip CIFAR stem 3->64 7x7 s2 on 32x32 (one image per 256 tile)": (3, 64, (7, 7), 2, 3, 32, 32, 12, 2, True),
    "flip 1 channel 3x3 on 16x16": (1, 64, (3, 3), 1, 1, 16, 16, 6, 2, False),
    "flip 3 channels 5x5 s1 on 24x24 (bands of 10 rows), 40 output channels": (3, 40, (5, 5), 1, 2, 24, 24, 4, 1, True),
}


@pytest.mark.parametrize("name", list(FLIP_STEMS))
def test_split_flipout_stem_vs_c_oracle(name):
    """Flipout with <= 3 input channels on the quad flavour (FLIP = true: the sign bits ride in the padding channel of the patch)."""
    from oracle import c_oracle as CO
    from bayesian_torch_amd import functional as F
    Ci, Co, k, st, pd, H, W, B, S, bias = FLIP_STEMS[name]
    g = torch.Generator().manual_seed(abs(hash(name)) % (1 << 31))
    mu, rho = torch.randn(Co, Ci, *k, generator=g) * 0.1, torch.randn(Co, Ci, *k, generator=g) * 0.1 - 3
    mb = torch.randn(Co, generator=g) * 0.1 if bias else None
    rb = torch.randn(Co, generator=g) * 0.1 - 3 if bias else None
    x = torch.randn(S * B, Ci, H, W, generator=g)
    conv = dict(stride=(st, st), padding=(pd, pd), dilation=(1, 1), groups=1)
    out, _, kn = _run_flip(mu, rho, mb, rb, x, conv, S, 0)
    assert "fused_split_quad_kernel" in kn and "flip" in kn, kn
    out32, _, kn32 = _run_flip(mu, rho, mb, rb, x, conv, S, 1)
    assert "split" not in kn32 and "flip" in kn32, kn32
    dev = torch.device("cuda")
    eps_w = F.rng_fill_normal(77, 2, 9, 5, 0, S, mu.shape, dev).cpu()
    eps_b = F.rng_fill_normal(77, 2, 9, 5, 1, S, (Co,), dev).cpu() if bias else None
    oshape = tuple(out.shape[1:])
    s_in = F.rng_fill_sign(77, 2, 9, 5, 2, S, (B, Ci, H, W), dev).cpu()
    s_out = F.rng_fill_sign(77, 2, 9, 5, 3, S, (B,) + oshape, dev).cpu()
    out, out32 = out.reshape((S, B) + oshape).cpu(), out32.reshape((S, B) + oshape).cpu()
    for s in range(S):
        ref = CO.flipout_fwd(x[s * B:(s + 1) * B], mu, rho, eps_w[s], s_in[s], s_out[s], mb, rb, None if eps_b is None else eps_b[s], conv)
        assert_close(out[s], ref, RTOL, ATOL, f"{name}[s={s}] split flipout stem vs C oracle")
        scale = float(ref.abs().max())
        e_split = float((out[s].double() - ref.double()).abs().max()) / scale
        e_f32 = float((out32[s].double() - ref.double()).abs().max()) / scale
        assert e_split <= 4.0 * e_f32 + 1.2e-7, (name, s, e_split, e_f32)


def test_split_flipout_stem_fused_maxpool():
    """Flipout stem -> scale/shift -> ReLU -> MaxPool2d(3, 2, 1) in the quad kernel's output stage == max_pool2d of its unpooled launch."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    g = torch.Generator().manual_seed(6)
    mu, rho = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).cuda(), (torch.randn(64, 3, 7, 7, generator=g) * 0.1 - 3).cuda()
    sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.3).cuda()
    x = torch.randn(10, 3, 32, 32, generator=g).cuda()
    conv = dict(stride=(2, 2), padding=(3, 3), dilation=(1, 1), groups=1)
    kw = dict(flip=True, conv=conv, S=3, seed=5, call=1, layer_id=4, sample0=0, packed=F.pack_params(mu, rho), post_scale=sc, post_shift=sh, relu=True)
    pooled = F._fused_forward(x, mu, rho, pool=True, **kw)
    kn = _lib.lib().bt_last_kernel_name().decode()
    assert pooled is not None and "fused_split_quad_kernel" in kn and "flip" in kn and "pool=1" in kn, kn
    full, _ = F.fused_forward(x, mu, rho, **kw)
    assert "pool=0" in _lib.lib().bt_last_kernel_name().decode()
    assert tuple(pooled[0].shape) == (30, 64, 8, 8)
    assert torch.equal(pooled[0], torch.nn.functional.max_pool2d(full, 3, 2, 1))


def test_tile_decode_without_host_reciprocals_is_bit_identical():
    """FwdArgs::inv_* are an optimisation only: with BT_NO_HOST_INV set (a fresh process: the knob is read once) every kernel
    divides instead, and a conv layer, a strided one-tap layer, a Flipout layer and a stem give the same bits."""
    import os, subprocess, sys, hashlib
    code = r'''
import hashlib, sys, torch
sys.path.insert(0, %r)
from bayesian_torch_amd import functional as F
def digest(flip, Ci, Co, k, st, pd, H, B, S):
    g = torch.Generator().manual_seed(Ci * 7 + k)
    mu = (torch.randn(Co, Ci, k, k, generator=g) * 0.1).cuda(); rho = (torch.randn(Co, Ci, k, k, generator=g) * 0.1 - 3).cuda()
    x = torch.randn(S * B, Ci, H, H, generator=g).cuda()
    conv = dict(stride=(st, st), padding=(pd, pd), dilation=(1, 1), groups=1)
    out, _ = F.fused_forward(x, mu, rho, flip=flip, conv=conv, S=S, shared_x=False, seed=3, call=1, layer_id=2, packed=F.pack_params(mu, rho))
    return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
print(digest(False, 64, 64, 3, 1, 1, 8, 128, 2), digest(False, 64, 128, 1, 2, 0, 8, 128, 2), digest(True, 64, 64, 3, 1, 1, 8, 128, 2), digest(False, 3, 64, 7, 2, 3, 32, 12, 2))
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    def run(extra):
        env = dict(os.environ, **extra)
        env.pop("BT_NO_HOST_INV", None) if not extra else None
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip().splitlines()[-1]
    assert run({}) == run({"BT_NO_HOST_INV": "1"})


POISON_CASES = ["layer1 64x64 3x3 8x8 (512 tile, 9 taps)", "odd octet count, one tap", "9 octets, partial channel tile, bias",
                "downsample 64->128 1x1 s2 (one tap: octet pairs)", "1x1 maps, partial batch tile (B = 120)", "groups 2, 3x2 kernel, stride (2,1)",
                "layer3 256x256 3x3 on 2x2 maps (row tiles, 6 of 9 taps, xm=2)", "14x14 maps 3x3 (W % 4 != 0: whole planes fetched flat)",
                "28x28 -> 14x14 1x1 s2 (every second column, XM 4)", "row bands 64x64 3x3 56x56"]


def test_split_kernels_never_read_lds_they_did_not_write():
    """The split kernels clear only their weight buffers and the shared zero pixels (bt_fused_split.h), the stem kernels nothing:
    every other LDS slot a consumer reads must have been written by a producer of the same workgroup. LDS survives from kernel
    to kernel, so fill all of it with NaN patterns (test hook bt_debug_poison_lds) right before each launch: Reparameterization,
    Flipout and stem launches over ragged geometries stay finite and bit-identical to the unpoisoned launch."""
    import ctypes
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(1, dtype=torch.int32, device="cuda")

    def poison():
        assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0

    for name in POISON_CASES:
        mu, rho, mb, rb, x, conv, B, S = _case(name)
        clean, kn = _run(mu, rho, mb, rb, x, conv, S, 0)
        poison()
        dirty, _ = _run(mu, rho, mb, rb, x, conv, S, 0)
        assert "split" in kn and torch.isfinite(dirty).all() and torch.equal(clean, dirty), (name, kn)
    for name in ("flip layer1 64x64 3x3 8x8 (row pieces, xm=3)", "flip W % 4 != 0 (generic fetch) 24x64 3x3 6x6",
                 "flip layer4 512x512 3x3 on 1x1 maps (128 tile, one tap, xm=1)", "flip small batch 64x64 3x3 4x4, B = 16 (128 tile of whole images)"):
        mu, rho, mb, rb, x, conv, B, S = _flip_case(name)
        clean, _, kn = _run_flip(mu, rho, mb, rb, x, conv, S, 0)
        poison()
        dirty, _, _ = _run_flip(mu, rho, mb, rb, x, conv, S, 0)
        assert "split" in kn and torch.isfinite(dirty).all() and torch.equal(clean, dirty), (name, kn)
    for name in ("9 octets, partial channel tile, bias", "odd octet count, one tap", "dilation 2", "layer2.0 64->128 3x3 s2"):   # the fp32-MFMA kernels too
        mu, rho, mb, rb, x, conv, B, S = _case(name)
        clean, kn = _run(mu, rho, mb, rb, x, conv, S, 1)
        poison()
        dirty, _ = _run(mu, rho, mb, rb, x, conv, S, 1)
        assert "split" not in kn and torch.isfinite(dirty).all() and torch.equal(clean, dirty), (name, kn)
    for flip in (False, True):     # stems (quad kernels: no clear at all), ragged channel count
        g = torch.Generator().manual_seed(9)
        mu, rho = torch.randn(40, 3, 7, 7, generator=g) * 0.1, torch.randn(40, 3, 7, 7, generator=g) * 0.1 - 3
        x = torch.randn(2 * 5, 3, 32, 32, generator=g)
        conv = dict(stride=(2, 2), padding=(3, 3), dilation=(1, 1), groups=1)
        clean = (_run_flip(mu, rho, None, None, x, conv, 2, 0) if flip else _run(mu, rho, None, None, x, conv, 2, 0))[0]
        assert "fused_split_quad_kernel" in L.bt_last_kernel_name().decode()
        poison()
        dirty = (_run_flip(mu, rho, None, None, x, conv, 2, 0) if flip else _run(mu, rho, None, None, x, conv, 2, 0))[0]
        assert torch.isfinite(dirty).all() and torch.equal(clean, dirty), ("stem", flip)


def _rand_geometry(r, big=False):
    """A random conv geometry the split flavour may or may not take (channels in octets or <= 4, <= 9 taps)."""
    stem = r.random() < 0.2
    groups = 1 if stem else r.choice([1, 1, 1, 2])
    Cig = r.choice([1, 2, 3, 4]) if stem else 8 * r.randint(1, 9)
    Co = groups * r.choice([8, 10, 24, 40, 64, 72, 96, 130])
    kh, kw = (r.choice([3, 5, 7]),) * 2 if stem else (r.randint(1, 3), r.randint(1, 3))
    st = (r.choice([1, 1, 2]), r.choice([1, 1, 2]))
    dl = (1, 1) if stem else (r.choice([1, 1, 2]), r.choice([1, 1, 2]))
    pd = (r.randint(0, (kh - 1) * dl[0]), r.randint(0, (kw - 1) * dl[1]))
    H, W = r.choice([1, 2, 3, 4, 6, 7, 8, 12, 14, 16, 20, 28]), r.choice([1, 2, 3, 4, 6, 7, 8, 12, 14, 16, 20, 28])
    if H + 2 * pd[0] < (kh - 1) * dl[0] + 1 or W + 2 * pd[1] < (kw - 1) * dl[1] + 1:
        H, W = max(H, kh * dl[0]), max(W, kw * dl[1])
    B = r.choice([1, 3, 8, 16, 33, 64, 128])
    S = r.choice([1, 2, 5])
    if big:      # chip-filling launches: the wide tiles (64 x 512 / 64 x 256) are only chosen when there are rounds of workgroups to save
        B, S = r.choice([64, 100, 128]), r.choice([8, 16, 32])
        if not stem:
            Cig = 8 * r.randint(1, 8)
        while S * B * H * W * Cig * groups > 1 << 25:
            S = max(1, S // 2)
    else:
        while B * H * W * Cig * groups > 1 << 21:
            B = max(1, B // 2)
    return dict(Ci=Cig * groups, Co=Co, k=(kh, kw), st=st, pd=pd, dl=dl, groups=groups, H=H, W=W, B=B, S=S,
                bias=r.random() < 0.5, flip=r.random() < 0.4)


def test_random_geometries_split_agrees_with_the_fp32_kernels():
    """120 random geometries (strides, dilations, groups, ragged channel counts, 1..28-pixel maps, stems, Flipout), each launched
    in automatic mode (split wherever eligible) behind NaN-poisoned LDS and in fp32 mode: finite and equal within the
    contraction's rounding. The fp32 kernels are held to the oracle elsewhere; this sweeps the tile / fetch-mode selection."""
    import ctypes, random
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    r = random.Random(20261004)
    taken = {}
    import os
    ncases = int(os.environ.get("BT_FUZZ_CASES", "120"))     # (one-off sweeps of up to 5000 cases were clean in round 2)
    for case in range(ncases):
        g = _rand_geometry(r, big=case % 4 == 3)
        linear = r.random() < 0.15       # Linear layers: [B, In] inputs, the fused kernels' 1x1 geometry
        if linear:
            g.update(Ci=r.choice([8, 40, 64, 100, 512, 784, 1000]), groups=1, k=(), H=1, W=1, B=r.choice([1, 7, 64, 128, 256]))
        gen = torch.Generator().manual_seed(case)
        wshape = (g["Co"], g["Ci"] // g["groups"]) + g["k"]
        mu, rho = (torch.randn(wshape, generator=gen) * 0.1).cuda(), (torch.randn(wshape, generator=gen) * 0.1 - 3).cuda()
        mb = (torch.randn(g["Co"], generator=gen) * 0.1).cuda() if g["bias"] else None
        rb = (torch.randn(g["Co"], generator=gen) * 0.1 - 3).cuda() if g["bias"] else None
        x = (torch.randn(g["S"] * g["B"], g["Ci"], generator=gen) if linear else torch.randn(g["S"] * g["B"], g["Ci"], g["H"], g["W"], generator=gen)).cuda()
        conv = None if linear else dict(stride=g["st"], padding=g["pd"], dilation=g["dl"], groups=g["groups"])
        kw = dict(flip=g["flip"], conv=conv, S=g["S"], shared_x=False, seed=5, call=case, layer_id=3, packed=F.pack_params(mu, rho))
        outs = {}
        for mode in (0, 1):
            _lib.check(L.bt_set_contraction(mode))
            try:
                assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0
                outs[mode], _ = F.fused_forward(x, mu, rho, mb, rb, **kw)
                if mode == 0:
                    kn = L.bt_last_kernel_name().decode()
                    key = kn.split("<")[0] + ("/" + kn.split(",")[1] if "split_kernel" in kn else "") + ("/flip" if g["flip"] else "")   # kernel / tile width
                    taken[key] = taken.get(key, 0) + 1
            finally:
                L.bt_set_contraction(0)
        a, b = outs[0], outs[1]
        if case % 3 == 0 and x.numel() <= 300000 and not linear:     # and sample 0 against the plain-C oracle on the replayed draws
            from oracle import c_oracle as CO
            dev = torch.device("cuda")
            Bq, S_ = g["B"], g["S"]
            eps_w = F.rng_fill_normal(5, case, 3, 0, 0, S_, mu.shape, dev).cpu()
            eps_b = F.rng_fill_normal(5, case, 3, 0, 1, S_, (g["Co"],), dev).cpu() if g["bias"] else None
            xs, cm = x[:Bq].cpu(), lambda t: None if t is None else t.cpu()
            if g["flip"]:
                s_in = F.rng_fill_sign(5, case, 3, 0, 2, S_, (Bq,) + tuple(x.shape[1:]), dev).cpu()
                s_out = F.rng_fill_sign(5, case, 3, 0, 3, S_, (Bq,) + tuple(a.shape[1:]), dev).cpu()
                ref = CO.flipout_fwd(xs, mu.cpu(), rho.cpu(), eps_w[0], s_in[0], s_out[0], cm(mb), cm(rb), None if eps_b is None else eps_b[0], conv)
            else:
                ref = CO.reparam_fwd(xs, mu.cpu(), rho.cpu(), eps_w[0], cm(mb), cm(rb), None if eps_b is None else eps_b[0], conv)
            assert_close(a[:Bq].cpu(), ref, RTOL, ATOL, f"fuzz case {case} {g} {kn} vs C oracle")
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (case, g, kn)
        scale = float(b.abs().max()) + 1e-30
        err = float((a - b).abs().max()) / scale
        assert err < 2e-5, (case, g, kn, err)
    print("kernels taken in automatic mode:", taken)
    assert sum(v for k, v in taken.items() if "split" in k) >= ncases // 3, taken
