"""GPU: Conv1d, Conv3d and ConvTranspose{1,2,3}d (both flavours) with ON-CHIP draws against an fp64 oracle on the draws the layers
report (materialize_last_draw), forward and gradients, with one geometry table that reaches every kernel flavour of the fused
Conv2d launch; the fold passes on these layers; the 128-tap limit of the pack check.

Reparameterization rows are compared with the native N-d convolution of the reference layout (bt_oracle._contract): that checks
the family's re-arrangements (zero-upsampling, channel transpose, spatial flip, depth unfold) independently. Flipout signs are
defined over the Conv2d launch's operands, so Flipout rows run the oracle on layer._x_eq / layer._w_eq (pinned
against the reference's goldens on CPU by test_layer_family.py) and map the result back; ConvTranspose1d/2d Flipout rows also gather
the reference-layout signs from the real positions of the upsampled input and check the native conv_transpose oracle agrees."""
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

# kernel flavour of a launch, from the name bt_last_kernel_name() reports (layer._last["kernel"])
_FLAVOUR_PREFIX = (("fused_split_quad_kernel", "quad"), ("fused_split_direct_kernel", "direct"), ("fused_split_skinny_kernel", "skinny"),
                   ("fused_split_kernel", "split"), ("fused_fast_kernel", "fast"), ("fused_fwd_kernel", "fwd"))
FLAVOURS = tuple(f for _, f in _FLAVOUR_PREFIX)


def flavour(kernel_name):
    for prefix, fl in _FLAVOUR_PREFIX:
        if kernel_name.startswith(prefix + "<"):
            return fl
    raise AssertionError(f"unknown kernel {kernel_name!r}")


R3 = dict(prior_mean=0.0, prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0)   # Conv3dReparameterization: no defaults

# (id, class, constructor, input shape, flavour the equivalent Conv2d launch was chosen for)
ROWS = [
    # Conv1d: 1-row images
    ("c1r_k3_oddW", "Conv1dReparameterization", dict(in_channels=16, out_channels=40, kernel_size=3, padding=1), (4, 16, 61), "split"),
    ("c1f_k9", "Conv1dFlipout", dict(in_channels=8, out_channels=24, kernel_size=9, padding=4), (4, 8, 64), "split"),
    ("c1r_k10", "Conv1dReparameterization", dict(in_channels=8, out_channels=16, kernel_size=10, padding=2, stride=2), (4, 8, 45), "fast"),
    ("c1f_k64", "Conv1dFlipout", dict(in_channels=4, out_channels=8, kernel_size=64), (2, 4, 100), "fast"),
    ("c1r_k65_nobias", "Conv1dReparameterization", dict(in_channels=2, out_channels=8, kernel_size=65, bias=False), (3, 2, 140), "fwd"),
    ("c1f_k128", "Conv1dFlipout", dict(in_channels=3, out_channels=5, kernel_size=128, stride=2, padding=3), (2, 3, 300), "fwd"),
    ("c1r_k1_direct", "Conv1dReparameterization", dict(in_channels=64, out_channels=48, kernel_size=1), (2, 64, 97), "direct"),
    ("c1r_stem", "Conv1dReparameterization", dict(in_channels=2, out_channels=16, kernel_size=7, padding=3), (16, 2, 128), "quad"),
    # Conv3d: (ci, kd) folded into the channel axis
    ("c3r_video_stem", "Conv3dReparameterization", dict(in_channels=1, out_channels=32, kernel_size=(3, 7, 7), stride=(1, 2, 2), padding=(1, 3, 3), **R3),
     (2, 1, 4, 32, 32), "quad"),
    ("c3r_stem_t64", "Conv3dReparameterization", dict(in_channels=1, out_channels=16, kernel_size=(2, 8, 8), **R3), (2, 1, 3, 27, 27), "quad"),
    ("c3f_stem_dstride_ddil", "Conv3dFlipout", dict(in_channels=1, out_channels=16, kernel_size=(3, 5, 5), stride=(2, 1, 1), padding=(2, 2, 2),
                                                    dilation=(2, 1, 1)), (2, 1, 7, 16, 16), "quad"),
    ("c3r_odd_cikd", "Conv3dReparameterization", dict(in_channels=3, out_channels=12, kernel_size=3, padding=1, **R3), (2, 3, 5, 9, 9), "fast"),
    ("c3f_split", "Conv3dFlipout", dict(in_channels=8, out_channels=20, kernel_size=(2, 3, 3), stride=(2, 1, 1), padding=(0, 1, 1)), (2, 8, 6, 10, 10), "split"),
    ("c3r_groups_ddil_nobias", "Conv3dReparameterization", dict(in_channels=4, out_channels=12, kernel_size=3, dilation=(2, 1, 1), padding=(2, 1, 1),
                                                                groups=2, bias=False, **R3), (2, 4, 5, 7, 7), "fast"),
    ("c3r_deepK_skinny", "Conv3dReparameterization", dict(in_channels=64, out_channels=40, kernel_size=(2, 3, 3), padding=(0, 1, 1), **R3),
     (3, 64, 2, 1, 1), "skinny"),
    # ConvTranspose: zero-upsampled, asymmetrically padded inputs, kernels transposed in their channel axes and flipped in space
    ("t2r_s2_outpad", "ConvTranspose2dReparameterization", dict(in_channels=16, out_channels=24, kernel_size=3, stride=2, padding=1, output_padding=1),
     (2, 16, 7, 7), "split"),
    ("t2f_groups", "ConvTranspose2dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, stride=2, padding=1, output_padding=1, groups=2),
     (2, 16, 6, 5), "split"),
    ("t2r_1x1_direct", "ConvTranspose2dReparameterization", dict(in_channels=64, out_channels=32, kernel_size=1), (2, 64, 8, 9), "direct"),
    ("t2f_crop", "ConvTranspose2dFlipout", dict(in_channels=6, out_channels=4, kernel_size=3, stride=2, padding=3, output_padding=1), (2, 6, 9, 8), "fast"),
    ("t2r_k11", "ConvTranspose2dReparameterization", dict(in_channels=4, out_channels=6, kernel_size=11, stride=3, padding=2), (2, 4, 5, 6), "fwd"),
    ("t1r_crop_outpad", "ConvTranspose1dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=5, stride=3, padding=6, output_padding=2),
     (2, 8, 44), "split"),
    ("t1f_dil", "ConvTranspose1dFlipout", dict(in_channels=6, out_channels=4, kernel_size=7, stride=2, dilation=3, padding=2, output_padding=1),
     (2, 6, 33), "fast"),
    ("t3r_stem", "ConvTranspose3dReparameterization", dict(in_channels=2, out_channels=4, kernel_size=(2, 3, 3), stride=(2, 1, 1), padding=(0, 1, 1)),
     (2, 2, 4, 8, 8), "quad"),
    ("t3f_outpad", "ConvTranspose3dFlipout", dict(in_channels=4, out_channels=8, kernel_size=3, stride=(1, 2, 2), padding=1, output_padding=(0, 1, 1),
                                                  bias=False), (2, 4, 3, 5, 5), "fast"),
]


def _native_conv(layer):
    """The reference layout's convolution arguments (bt_oracle._contract), whatever the class."""
    from bayesian_torch_amd.layers._family import FamilyConvLayer
    nd = layer._nd if isinstance(layer, FamilyConvLayer) else (1 if getattr(layer, "_one_d", False) else 2)
    tup = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * nd
    conv = dict(stride=tup(layer.stride), padding=tup(layer.padding), dilation=tup(layer.dilation), groups=layer.groups)
    if getattr(layer, "_transposed", False):
        conv.update(transposed=True, output_padding=tup(layer.output_padding))
    return conv


def _params64(layer, grad=False):
    """The layer's (mu, rho) in its own layout as fp64 CPU tensors (leaves that require grad when ``grad``)."""
    t = lambda v: None if v is None else v.detach().double().cpu().clone().requires_grad_(grad)
    return dict(mu_w=t(layer.mu_kernel), rho_w=t(layer.rho_kernel), mu_b=t(layer.mu_bias), rho_b=t(layer.rho_bias))


def _native_signs(layer, x, si_eq, so_eq, back):
    """ConvTranspose{1,2}d Flipout: the reference-layout sign tensors of one sample, gathered from the launch's operands -- sign_in at
    the real (non-inserted) positions of the zero-upsampled, padded x (1 where a real element was cropped away: it meets no tap),
    sign_out mapped back like the output."""
    s, p, d, _, ks = layer._geom()
    si = si_eq.squeeze(2) if layer._nd == 1 else si_eq
    keep = torch.ones((), dtype=torch.bool)
    for i in range(layer._nd):
        ax = 2 + i
        pos = d[i] * (ks[i] - 1) - p[i] + torch.arange(x.shape[ax]) * s[i]
        ok = (pos >= 0) & (pos < si.shape[ax])
        si = si.index_select(ax, pos.clamp(0, si.shape[ax] - 1))
        keep = keep.unsqueeze(-1) & ok if i else ok
    return torch.where(keep, si, torch.ones_like(si)), back(so_eq)


def _oracle(layer, x, p, draws, S, shared, check_native=False):
    """fp64 oracle of every sample of the last forward -> [S*B, ...] (differentiable in x and p). x: fp64 CPU, shared ([B, ...]) or
    stacked ([S*B, ...])."""
    from oracle import bt_oracle as O
    from bayesian_torch_amd.layers._family import FamilyConvLayer
    conv = _native_conv(layer)
    B = x.shape[0] // (1 if shared else S)
    family = isinstance(layer, FamilyConvLayer)
    outs = []
    for s in range(S):
        xs = x if shared else x[s * B:(s + 1) * B]
        ew = draws["eps_w"][s].cpu().double()
        eb = draws["eps_b"][s].cpu().double() if "eps_b" in draws else None
        if not layer._flip:
            outs.append(O.reparam_fwd_ref(xs, p["mu_w"], p["rho_w"], ew, p["mu_b"], p["rho_b"], eb, conv))
            continue
        si_key, so_key = ("sign_in_eq", "sign_out_eq") if family else ("sign_in", "sign_out")
        si, so = draws[si_key][s].cpu().double(), draws[so_key][s].cpu().double()
        if not family:       # Conv1d: the launch's [B][C][1][L] operands are the reference's [B][C][L]
            outs.append(O.flipout_fwd_ref(xs, p["mu_w"], p["rho_w"], ew, si.squeeze(2), so.squeeze(2), p["mu_b"], p["rho_b"], eb, conv))
            continue
        xe, c2, back = layer._x_eq(xs)
        o = back(O.flipout_fwd_ref(xe, layer._w_eq(p["mu_w"]), layer._w_eq(p["rho_w"]), layer._w_eq(ew), si, so, p["mu_b"], p["rho_b"], eb, c2))
        if check_native and layer._transposed and layer._nd < 3:
            # one sign per real element: the native transposed convolution on the gathered signs is the same function
            si_n, so_n = _native_signs(layer, xs, si, so, back)
            o_n = O.flipout_fwd_ref(xs, p["mu_w"], p["rho_w"], ew, si_n, so_n, p["mu_b"], p["rho_b"], eb, conv)
            assert_close(o_n.detach(), o.detach(), 1e-10, 1e-12, "native conv_transpose oracle vs the launch-operand oracle")
        outs.append(o)
    return torch.cat(outs)


def _make(cls, ctor, seed):
    import bayesian_torch_amd.layers as L
    torch.manual_seed(seed)
    layer = getattr(L, cls)(**ctor)
    with torch.no_grad():      # rho spread out, so sigma*eps is not a small correction of mu (a wrong draw must show)
        layer.rho_kernel.uniform_(-2.5, -0.5)
        if layer.rho_bias is not None:
            layer.rho_bias.uniform_(-2.5, -0.5)
    return layer.cuda()


def _check_run(layer, out, x, S, shared, want, what):
    got_fl = flavour(layer._last["kernel"])
    assert got_fl == want, f"{what}: chose {layer._last['kernel']}, the row is for {want}"
    ref = _oracle(layer, x.cpu().double(), _params64(layer), layer.materialize_last_draw(), S, shared, check_native=True)
    B = ref.shape[0] // S
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    for s in range(S):
        assert_close(out[s * B:(s + 1) * B].cpu(), ref[s * B:(s + 1) * B], 1e-4, 1e-5, f"{what} sample {s}")
    return layer._last["kernel"]


@pytest.mark.parametrize("rid,cls,ctor,xshape,want", ROWS, ids=[r[0] for r in ROWS])
def test_family_on_chip_draws_match_fp64_oracle(rid, cls, ctor, xshape, want):
    """S = 1 alone; S = 3 under mc_samples with a shared [B, ...] input (sample0 = 0) and with a stacked [S*B, ...] input
    (sample0 = 5): every sample against the fp64 oracle on the draws the layer reports."""
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    rng.manual_seed(1234)
    layer = _make(cls, ctor, 7)
    g = torch.Generator().manual_seed(3)
    B = xshape[0]
    x = torch.randn(xshape, generator=g).cuda()
    xs = torch.randn((3 * B,) + tuple(xshape[1:]), generator=g).cuda()
    names = []
    with torch.no_grad():
        out, kl = layer(x)
        names.append(_check_run(layer, out, x, 1, True, want, f"{rid} S=1"))
        with mc.mc_samples(3, B, sample0=0):
            out = layer(x, return_kl=False)
        names.append(_check_run(layer, out, x, 3, True, want, f"{rid} S=3 shared"))
        with mc.mc_samples(3, B, sample0=5):
            out = layer(xs, return_kl=False)
        names.append(_check_run(layer, out, xs, 3, False, want, f"{rid} S=3 stacked sample0=5"))
    from oracle import bt_oracle as O
    p = _params64(layer)
    prior = lambda t: None if t is None else t.cpu().double()
    klr = O.kl_layer_ref(p["mu_w"], p["rho_w"], prior(layer.prior_weight_mu), prior(layer.prior_weight_sigma), p["mu_b"], p["rho_b"],
                         prior(layer.prior_bias_mu), prior(layer.prior_bias_sigma))
    assert_close(kl.cpu(), klr, 1e-5, 0, f"{rid} kl")
    print(f"{rid:24s} {cls:34s} " + " | ".join(names))


def test_family_table_reaches_every_flavour():
    """Every row lands on the flavour it was chosen for (one S = 1 forward each), and the table reaches them all. The launch
    info reports the plan that ran: one workgroup per (group, channel tile, sample, pixel tile), several for the split-K flavour."""
    from bayesian_torch_amd import _lib, rng
    rng.set_mode("philox")
    rng.manual_seed(99)
    seen = {}
    for rid, cls, ctor, xshape, want in ROWS:
        layer = _make(cls, ctor, 1)
        with torch.no_grad():
            layer(torch.randn(xshape).cuda(), return_kl=False)
        name, li = layer._last["kernel"], _lib.last_launch_info()
        print(f"{rid:24s} -> {flavour(name):6s} {name} {li}")
        assert flavour(name) == want, (rid, name, want)
        grid = li["groups"] * li["n_tiles"] * li["S"] * li["m_tiles"]
        assert li["workgroups"] > 0 and grid > 0, (rid, name, li)
        if want == "skinny":
            assert li["workgroups"] % grid == 0, (rid, name, li)
        else:
            assert li["workgroups"] == grid, (rid, name, li)
        seen.setdefault(want, []).append(rid)
    assert set(seen) == set(FLAVOURS), seen
    classes = {r[1] for r in ROWS}
    assert classes == {"Conv1dReparameterization", "Conv1dFlipout", "Conv3dReparameterization", "Conv3dFlipout",
                       "ConvTranspose1dReparameterization", "ConvTranspose1dFlipout", "ConvTranspose2dReparameterization",
                       "ConvTranspose2dFlipout", "ConvTranspose3dReparameterization", "ConvTranspose3dFlipout"}, classes


# ---------------------------------------------------------------------------------------------------------------- gradients
GRAD_ROWS = [
    ("c1r", "Conv1dReparameterization", dict(in_channels=8, out_channels=12, kernel_size=3, stride=2, padding=1, groups=2), (3, 8, 21)),
    ("c1f", "Conv1dFlipout", dict(in_channels=6, out_channels=8, kernel_size=5, padding=2, dilation=2), (2, 6, 19)),
    ("c3r", "Conv3dReparameterization", dict(in_channels=3, out_channels=6, kernel_size=(2, 3, 3), stride=(2, 1, 1), padding=(1, 1, 0), **R3), (2, 3, 5, 6, 7)),
    ("c3f", "Conv3dFlipout", dict(in_channels=4, out_channels=6, kernel_size=3, padding=1, dilation=(2, 1, 1), groups=2), (2, 4, 6, 5, 5)),
    ("t1r", "ConvTranspose1dReparameterization", dict(in_channels=6, out_channels=4, kernel_size=4, stride=3, padding=5, output_padding=1), (2, 6, 17)),
    ("t1f", "ConvTranspose1dFlipout", dict(in_channels=4, out_channels=6, kernel_size=3, stride=2, padding=1, output_padding=1, bias=False), (3, 4, 11)),
    ("t2r", "ConvTranspose2dReparameterization", dict(in_channels=8, out_channels=6, kernel_size=3, stride=2, padding=1, output_padding=1, groups=2),
     (2, 8, 5, 6)),
    ("t2f", "ConvTranspose2dFlipout", dict(in_channels=6, out_channels=8, kernel_size=(3, 2), stride=(2, 1), padding=(1, 0), dilation=(1, 2),
                                           output_padding=(1, 0), groups=2), (2, 6, 5, 4)),
    ("t3r", "ConvTranspose3dReparameterization", dict(in_channels=4, out_channels=4, kernel_size=(2, 3, 3), stride=(2, 1, 2), padding=(0, 1, 1),
                                                     output_padding=(1, 0, 1)), (2, 4, 3, 4, 4)),
    ("t3f", "ConvTranspose3dFlipout", dict(in_channels=2, out_channels=4, kernel_size=3, stride=(1, 2, 1), padding=1, output_padding=(0, 1, 0)),
     (2, 2, 3, 4, 5)),
]


@pytest.mark.parametrize("rid,cls,ctor,xshape", GRAD_ROWS, ids=[r[0] for r in GRAD_ROWS])
@pytest.mark.parametrize("S", [1, 2])
def test_family_gradients_match_fp64_oracle_autograd(rid, cls, ctor, xshape, S):
    """dx, dmu, drho, dbias of out*gout + 3*KL (the fused forward, the HIP backward through the autograd bridge, the re-arrangements'
    own autograd) against torch autograd of the fp64 oracle on the same draws -- tolerances of test_gpu_autograd.py."""
    from oracle import bt_oracle as O
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    rng.manual_seed(11)
    layer = _make(cls, ctor, 3)
    x = torch.randn(xshape, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    if S == 1:
        out, kl = layer(x)
    else:
        with mc.mc_samples(S, xshape[0]):
            out, kl = layer(x)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).cuda()
    ((out * gout).sum() + 3.0 * kl).backward()

    p = _params64(layer, grad=True)
    xc = x.detach().cpu().double().requires_grad_(True)
    ref = _oracle(layer, xc, p, layer.materialize_last_draw(), S, True)
    prior = lambda t: None if t is None else t.cpu().double()
    klr = O.kl_layer_ref(p["mu_w"], p["rho_w"], prior(layer.prior_weight_mu), prior(layer.prior_weight_sigma), p["mu_b"], p["rho_b"],
                         prior(layer.prior_bias_mu), prior(layer.prior_bias_sigma))
    ((ref * gout.cpu().double()).sum() + 3.0 * klr).backward()
    assert_close(out.detach().cpu(), ref.detach(), 1e-4, 1e-5, f"{rid} out")
    assert_close(x.grad.cpu(), xc.grad, 1e-4, 1e-5, f"{rid} dL/dx")
    for k, t in (("mu_w", layer.mu_kernel), ("rho_w", layer.rho_kernel), ("mu_b", layer.mu_bias), ("rho_b", layer.rho_bias)):
        if t is not None:
            assert_close(t.grad.cpu(), p[k].grad, 2e-4, 2e-5, f"{rid} dL/d{k}")


# ---------------------------------------------------------------------------------------------------------------- fold passes
def _bits_before_after_fold(model, x, S, folds):
    from bayesian_torch_amd import rng
    model[0].dnn_to_bnn_flag = True        # (a converted model's layers return the output alone)
    from bayesian_torch_amd.fuse import fold_batchnorm, fold_relu
    from bayesian_torch_amd.mc import mc_forward
    rng.set_mode("philox")
    rng.manual_seed(21)
    before, kl0 = mc_forward(model, x, S)
    n = fold_batchnorm(model) + fold_relu(model)
    rng.manual_seed(21)
    after, kl1 = mc_forward(model, x, S)
    assert n == folds, (n, folds)
    assert torch.equal(before, after) and torch.equal(kl0, kl1)
    return model


def test_fold_passes_leave_family_layers_bit_identical():
    """ConvTranspose2d -> BatchNorm2d -> ReLU (a decoder block) and Conv3d -> ReLU: nothing folds, the same bits before and after;
    Conv1d -> ReLU: the ReLU folds into Conv1d's output stage, the same bits."""
    import torch.nn as nn
    import bayesian_torch_amd.layers as L
    torch.manual_seed(0)
    for cls in ("ConvTranspose2dReparameterization", "ConvTranspose2dFlipout"):
        bn = nn.BatchNorm2d(4)
        with torch.no_grad():
            bn.running_mean.uniform_(-1, 1), bn.running_var.uniform_(0.5, 2), bn.weight.uniform_(0.5, 2), bn.bias.uniform_(-1, 1)
        m = _bits_before_after_fold(nn.Sequential(getattr(L, cls)(8, 4, 3, stride=2), bn, nn.ReLU()).cuda().eval(),
                                    torch.randn(2, 8, 5, 5).cuda(), 3, 0)
        assert isinstance(m[1], nn.BatchNorm2d) and isinstance(m[2], nn.ReLU)
    m = _bits_before_after_fold(nn.Sequential(L.Conv3dFlipout(2, 4, 3), nn.ReLU()).cuda().eval(), torch.randn(2, 2, 5, 6, 6).cuda(), 2, 0)
    assert isinstance(m[1], nn.ReLU)
    for cls in ("Conv1dReparameterization", "Conv1dFlipout"):
        m = _bits_before_after_fold(nn.Sequential(getattr(L, cls)(4, 8, 3, padding=1), nn.ReLU()).cuda().eval(), torch.randn(3, 4, 40).cuda(), 2, 1)
        assert m[0].post_relu and isinstance(m[1], nn.Identity)


# ---------------------------------------------------------------------------------------------------------------- 128-tap limit
@pytest.mark.parametrize("cls,args,xshape", [("Conv2dReparameterization", (4, 4, 12), (1, 4, 16, 16)),
                                             ("Conv1dFlipout", (2, 2, 129), (1, 2, 200)),
                                             ("ConvTranspose1dReparameterization", (2, 2, 130), (1, 2, 8))])
def test_kernels_over_128_taps_are_refused_by_name(cls, args, xshape):
    import bayesian_torch_amd.layers as L
    layer = getattr(L, cls)(*args).cuda()
    with pytest.raises(NotImplementedError, match=f"{cls}.*128-tap limit"):
        with torch.no_grad():
            layer(torch.randn(xshape).cuda())


def test_refused_model_check_leaves_the_other_packs_current():
    """A model with a 12x12 layer between two 3x3 layers: after new values are written into the 3x3 layers' mu through .data,
    mc_forward refuses; each 3x3 layer run on its own then computes with its NEW parameters (its pack is not left stale against a
    fingerprint the refused check recorded)."""
    import torch.nn as nn
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import mc_forward
    rng.set_mode("philox")
    rng.manual_seed(5)
    torch.manual_seed(0)
    a, big, b = L.Conv2dReparameterization(4, 4, 3, padding=1), L.Conv2dReparameterization(4, 4, 12), L.Conv2dFlipout(4, 4, 3, padding=1)
    model = nn.Sequential(a, big, b).cuda().eval()
    x = torch.randn(2, 4, 16, 16).cuda()
    with torch.no_grad():
        a(x), b(x)                                  # packs built from the first values
        a.mu_kernel.data.copy_(torch.randn_like(a.mu_kernel))
        b.mu_kernel.data.copy_(torch.randn_like(b.mu_kernel))
    with pytest.raises(NotImplementedError, match="128-tap limit"):
        mc_forward(model, x, 2)
    for layer in (a, b):
        with torch.no_grad():
            out = layer(x, return_kl=False)
        ref = _oracle(layer, x.cpu().double(), _params64(layer), layer.materialize_last_draw(), 1, True)
        assert_close(out.cpu(), ref, 1e-4, 1e-5, type(layer).__name__ + " after the refused model check")


def test_pack_sync_refuses_before_any_launch():
    """bt_pack_sync_kl called directly (real device buffers for every segment) with a 144-tap segment beside a 9-tap one: the call
    fails, and the 9-tap segment's device state -- fingerprint, dirty flag, rebuild count -- is exactly what it was, so the next check
    rebuilds its pack from the new values."""
    from bayesian_torch_amd import functional as F
    dev = torch.device("cuda")
    torch.manual_seed(0)

    def seg(mu, rho, bufs):
        Co, Ci = mu.shape[:2]
        return dict(mu=mu, rho=rho, src_mu=None, src_rho=None, mu_packed=bufs[0], sigma_packed=bufs[1], state=bufs[2],
                    Co=Co, Ci=Ci, taps=mu[0, 0].numel(), force=False)

    mu, rho = torch.randn(4, 4, 3, 3, device=dev), torch.randn(4, 4, 3, 3, device=dev)
    mu_big, rho_big = torch.randn(4, 4, 12, 12, device=dev), torch.randn(4, 4, 12, 12, device=dev)
    bufs, bufs_big = F.pack_buffers(4, 4, 9, dev), F.pack_buffers(4, 4, 144, dev)
    F.pack_sync([seg(mu, rho, bufs)])
    packed = lambda t: t.reshape(4, 4, 9).permute(0, 2, 1)      # [Co][T][C4] with C4 == Ci
    assert int(bufs[2][3]) == 1 and torch.equal(bufs[0], packed(mu))
    mu.add_(1.0)
    state = bufs[2].clone()
    with pytest.raises(RuntimeError, match="128 taps"):
        F.pack_sync([seg(mu_big, rho_big, bufs_big), seg(mu, rho, bufs)])
    torch.cuda.synchronize()
    assert torch.equal(bufs[2], state), (bufs[2].tolist(), state.tolist())
    F.pack_sync([seg(mu, rho, bufs)])
    assert int(bufs[2][3]) == 2 and torch.equal(bufs[0], packed(mu))
