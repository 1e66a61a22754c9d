"""GPU: ConvTranspose1d / ConvTranspose2d on the "native" path -- the kernels read the un-upsampled x through the input-dilated fetch
(bt_*_conv2d_updil_fwd: xm 5 of the general split kernel, the UPD instantiations of fused_fwd_kernel) -- against the materialising
("upsample") path and the fp64 oracle on the draws the layers report.

The geometries (tests/test_convt_native_host.py: ROWS) are the smallest that reach each thing that can go wrong:
  a  T2d 16->24 k3 s2 p1 op1, x [3,16,9,11]           several tiles per image, ragged last tile, far-side pad != near-side pad
  b  T2d 16->16 k(3,2) s(2,1) p(1,0) d(1,2) groups 2   rectangular kernel; dilation in one axis, u = 1 in the other
  c  T1d 8->8 k5 s3 p2 op2, x [4,8,17]                 1 x k kernel, u = 3
  d  T2d 64->32 k2 s2, x [2,64,4,4]                    the U-Net upsampler: every output pixel meets ONE tap; also with 32-channel tiles forced
  e  T2d 6->4 k3 s2 p1 op1                             Cig % 8 != 0: fused_fwd_kernel
  f  T2d Flipout 16->16 groups 2; T1d Flipout no bias  Flipout tiles and sign indexing
  g  T2d 8->8 k3 s2 p3                                 a crop: must report x_path == "upsample"
Every row runs at S = 1, and at S = 3 with shared and with stacked x. The 256- and 512-wide tiles, which none of those plans picks,
have a test of their own. Tolerance: the project's rtol 1e-4, atol 1e-5 * max|ref| (conftest.assert_close)."""
import ctypes

import pytest
import torch

from conftest import assert_close
from test_convt_native_host import CROP_ROW, ROWS, make_layer

pytestmark = pytest.mark.gpu
ROW = {r[0]: r for r in ROWS}


@pytest.fixture(autouse=True)
def _restore_switches():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import _lib, rng
    prev, mode = L.get_transpose_path(), _lib.lib().bt_get_contraction()
    rng.set_mode("philox")
    yield
    L.set_transpose_path(prev)
    _lib.lib().bt_set_contraction(mode)
    ctypes.CDLL(_lib.LIB_PATH).bt_debug_force_bn32(-1)


def _inputs(xshape, S=3):
    g = torch.Generator().manual_seed(3)
    return torch.randn(xshape, generator=g).cuda(), torch.randn((S * xshape[0],) + tuple(xshape[1:]), generator=g).cuda()


def _runs(layer, x, xs, path, S=3, seed=1234):
    """The three forwards of a row on ``path`` from the same RNG coordinates -> [(out, kl or None, _last, materialised draw)]."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    L.set_transpose_path(path)
    rng.manual_seed(seed)
    B, res = x.shape[0], []
    with torch.no_grad():
        out, kl = layer(x)
        res.append((out, kl, dict(layer._last), layer.materialize_last_draw()))
        with mc.mc_samples(S, B, sample0=0):
            out = layer(x, return_kl=False)
        res.append((out, None, dict(layer._last), layer.materialize_last_draw()))
        with mc.mc_samples(S, B, sample0=5):
            out = layer(xs, return_kl=False)
        res.append((out, None, dict(layer._last), layer.materialize_last_draw()))
    return res


def _native_conv(layer):
    tup = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * layer._nd
    return dict(stride=tup(layer.stride), padding=tup(layer.padding), dilation=tup(layer.dilation), groups=layer.groups, transposed=True,
                output_padding=tup(layer.output_padding))


def _oracle(layer, x, draws, S, shared):
    """fp64 conv_transpose of every sample in the REFERENCE's layouts, on the reported draws -> [S*B, ...]."""
    from oracle import bt_oracle as O
    t = lambda v: None if v is None else v.detach().double().cpu()
    p = dict(mu_w=t(layer.mu_kernel), rho_w=t(layer.rho_kernel), mu_b=t(layer.mu_bias), rho_b=t(layer.rho_bias))
    conv, x = _native_conv(layer), x.double().cpu()
    B = x.shape[0] // (1 if shared else S)
    outs = []
    for s in range(S):
        xs = x if shared else x[s * B:(s + 1) * B]
        ew, eb = t(draws["eps_w"][s]), t(draws["eps_b"][s]) if "eps_b" in draws else None
        if layer._flip:
            outs.append(O.flipout_fwd_ref(xs, p["mu_w"], p["rho_w"], ew, t(draws["sign_in"][s]), t(draws["sign_out"][s]), p["mu_b"], p["rho_b"], eb, conv))
        else:
            outs.append(O.reparam_fwd_ref(xs, p["mu_w"], p["rho_w"], ew, p["mu_b"], p["rho_b"], eb, conv))
    return torch.cat(outs)


def _check_oracle(layer, run, x, S, shared, what):
    out, _, last, draws = run
    ref = _oracle(layer, x, draws, S, shared)
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    B = ref.shape[0] // S
    for s in range(S):
        assert_close(out[s * B:(s + 1) * B].cpu(), ref[s * B:(s + 1) * B], 1e-4, 1e-5, f"{what} sample {s} ({last['kernel']})")


def _is_split(name):
    return name.startswith("fused_split_kernel<")


# d-bn32: row d with the 32-channel tiles forced on (its 32 channels per group keep the 64-channel tile); d64-bn32: the same upsampler with
# 64 output channels, which takes them
ROW["D"] = ("D", ROW["d"][1], dict(ROW["d"][2], out_channels=64), ROW["d"][3])
REPARAM_IDS = ["a", "b", "c", "d", "d-bn32", "D-bn32"]


@pytest.mark.parametrize("rid", REPARAM_IDS)
def test_reparam_rows_equal_the_upsample_path_and_match_the_oracle(rid):
    from bayesian_torch_amd import _lib
    _, cls, ctor, xshape = ROW[rid[0]]
    if rid.endswith("bn32"):
        ctypes.CDLL(_lib.LIB_PATH).bt_debug_force_bn32(1)
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    nat, ups = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "upsample")
    real = tuple(x.unsqueeze(2).shape) if layer._nd == 1 else tuple(x.shape)
    for i, (n, u, (xin, S, shared)) in enumerate(zip(nat, ups, ((x, 1, True), (x, 3, True), (xs, 3, False)))):
        what = f"{rid} run {i}"
        assert n[2]["x_path"] == "native" and u[2].get("x_path", "upsample") == "upsample" and n[2]["x_shape"] == real and u[2]["x_shape"] != real
        kn, ku = n[2]["kernel"], u[2]["kernel"]
        assert _is_split(kn) and "xm=5" in kn and "bf16x3" in kn, kn
        assert _is_split(ku) and "xm=5" not in ku, ku      # (every row was chosen so that the materialised launch is the general split kernel's)
        assert kn.split(",xm=")[0] == ku.split(",xm=")[0]
        assert kn.startswith("fused_split_kernel<32,128," if rid == "D-bn32" else "fused_split_kernel<64,128,"), kn
        assert torch.equal(n[0], u[0]), f"{what}: {kn} vs {ku}: max abs {float((n[0] - u[0]).abs().max()):.3e}"
        assert torch.equal(n[3]["eps_w"], u[3]["eps_w"])
        _check_oracle(layer, n, xin, S, shared, what)
    assert torch.equal(nat[0][1], ups[0][1]) and float(nat[0][1]) > 0      # KL


@pytest.mark.parametrize("rid", ["e", "f2", "f1"])
def test_fp32_general_and_flipout_rows_match_the_oracle(rid):
    _, cls, ctor, xshape = ROW[rid]
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    nat, again = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "native")
    real = tuple(x.unsqueeze(2).shape) if layer._nd == 1 else tuple(x.shape)
    for i, (n, r, (xin, S, shared)) in enumerate(zip(nat, again, ((x, 1, True), (x, 3, True), (xs, 3, False)))):
        kn = n[2]["kernel"]
        assert n[2]["x_path"] == "native" and n[2]["x_shape"] == real
        if rid == "e":
            assert kn.startswith("fused_fwd_kernel<") and kn.endswith(",updil>"), kn
        else:
            assert _is_split(kn) and ",flip," in kn and "xm=5" in kn, kn
            si = n[3]["sign_in"]      # one sign per REAL input element, in the reference's layout
            assert tuple(si.shape) == (S, x.shape[0]) + tuple(x.shape[1:]) and bool((si.abs() == 1).all())
            assert tuple(n[3]["sign_out"].shape) == (S, x.shape[0]) + tuple(n[0].shape[1:])
            assert 0.3 < float((si > 0).float().mean()) < 0.7
        _check_oracle(layer, n, xin, S, shared, f"{rid} run {i}")
        assert torch.equal(n[0], r[0]), f"{rid} run {i}: a re-run from the same coordinates differs"
    if rid == "e":      # same draws on both paths (Reparameterization): the fast kernel's fp32 chain agrees within the tolerance
        ups = _runs(layer, x, xs, "upsample")
        for n, u in zip(nat, ups):
            assert u[2].get("x_path", "upsample") == "upsample" and not u[2]["kernel"].endswith(",updil>")
            assert_close(n[0].cpu(), u[0].cpu(), 1e-4, 1e-5, "e native vs upsample")
        assert torch.equal(nat[0][1], ups[0][1])


def test_crop_keeps_the_materialising_path():
    _, cls, ctor, xshape = CROP_ROW
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    nat, ups = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "upsample")
    for n, u, (xin, S, shared) in zip(nat, ups, ((x, 1, True), (x, 3, True), (xs, 3, False))):
        assert n[2]["x_path"] == "upsample" and n[2]["kernel"] == u[2]["kernel"] and n[2]["x_shape"] == u[2]["x_shape"]
        assert "x_path" not in u[2]      # the default setting's launch record is what it was
        assert torch.equal(n[0], u[0])
        _check_oracle(layer, n, xin, S, shared, "g")


def test_grad_and_supplied_draws_keep_the_materialising_path():
    import bayesian_torch_amd.layers as L
    _, cls, ctor, xshape = ROW["a"]
    layer = make_layer(cls, ctor).cuda()
    x, _ = _inputs(xshape)
    L.set_transpose_path("native")
    out, _ = layer(x)      # grad enabled, parameters require grad
    assert layer._last["x_path"] == "upsample" and out.requires_grad
    with torch.no_grad():
        layer(x)
        d = layer.materialize_last_draw()
        assert layer._last["x_path"] == "native"
        layer.inject_draw = dict(eps_w=d["eps_w"], eps_b=d["eps_b"])
        out2, _ = layer(x)
        layer.inject_draw = None
    assert layer._last["x_path"] == "upsample"


def test_bf16_mode_takes_the_dilated_fetch():
    from bayesian_torch_amd import _lib
    _, cls, ctor, xshape = ROW["a"]
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    exact = _runs(layer, x, xs, "native")
    assert _lib.lib().bt_set_contraction(3) == 0
    nat, ups = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "upsample")
    for n, u, e in zip(nat, ups, exact):
        kn, ku = n[2]["kernel"], u[2]["kernel"]
        assert _is_split(kn) and "bf16x1" in kn and "xm=5" in kn, kn
        assert _is_split(ku) and "bf16x1" in ku and "xm=5" not in ku, ku
        assert torch.equal(n[0], u[0]) and not torch.equal(n[0], e[0])


@pytest.mark.parametrize("rid", ["a", "d", "f2", "e"])
def test_dilated_kernels_never_read_lds_they_did_not_write(rid):
    """LDS survives from kernel to kernel: NaN patterns in all of it right before each launch -- finite, and the same bits."""
    from bayesian_torch_amd import _lib, mc, rng
    import bayesian_torch_amd.layers as Lm
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(4, dtype=torch.int32, device="cuda")
    _, cls, ctor, xshape = ROW[rid]
    layer = make_layer(cls, ctor).cuda().eval()
    x, _ = _inputs(xshape)
    Lm.set_transpose_path("native")
    outs = []
    with torch.no_grad():
        layer(x)      # (the pack is built: nothing but the forward runs behind the poisoning)
        for poison in (False, True):
            rng.manual_seed(77)
            if poison:
                assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0
            with mc.mc_samples(3, x.shape[0]):
                outs.append(layer(x, return_kl=False))
            assert layer._last["x_path"] == "native"
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[0], outs[1]), (rid, layer._last["kernel"])


# (class, constructor, x shape, S, the tile the plan picks): the 256- and 512-wide tiles of both flavours
WIDE = [
    ("ConvTranspose2dReparameterization", dict(in_channels=16, out_channels=16, kernel_size=3, stride=2, padding=1, output_padding=1), (8, 16, 16, 16), 8, "<64,256,"),
    ("ConvTranspose2dReparameterization", dict(in_channels=64, out_channels=8, kernel_size=3, stride=2, padding=1, output_padding=1), (8, 64, 32, 32), 3, "<64,512,"),
    ("ConvTranspose1dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, stride=2, padding=1, output_padding=1), (8, 16, 256), 16, "<64,256,"),
]


@pytest.mark.parametrize("cls,ctor,xshape,S,tile", WIDE, ids=["r256", "r512", "f256"])
def test_wide_tiles(cls, ctor, xshape, S, tile):
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    layer = make_layer(cls, ctor).cuda().eval()
    x, _ = _inputs(xshape, S=1)
    res = {}
    with torch.no_grad():
        for path in ("native", "upsample"):
            L.set_transpose_path(path)
            rng.manual_seed(5)
            with mc.mc_samples(S, x.shape[0]):
                out = layer(x, return_kl=False)
            res[path] = (out, None, dict(layer._last), layer.materialize_last_draw())
    kn = res["native"][2]["kernel"]
    assert res["native"][2]["x_path"] == "native" and _is_split(kn) and tile in kn and "xm=5" in kn, kn
    assert tile in res["upsample"][2]["kernel"]
    if not layer._flip:
        assert torch.equal(res["native"][0], res["upsample"][0])
    _check_oracle(layer, res["native"], x, S, True, f"wide {tile}")


def test_native_call_allocates_less_than_the_upsampled_tensor():
    """The test that states the feature: T2d 64->8 k3 s2 p1 op1 on [8,64,32,32], eval, no grad, after a warm-up call. The upsampled,
    padded x is 8*64*65*65 floats; the native call's peak stays below that (its output is 1 MB), the materialising call's exceeds it."""
    import bayesian_torch_amd.layers as L
    layer = make_layer("ConvTranspose2dReparameterization", dict(in_channels=64, out_channels=8, kernel_size=3, stride=2, padding=1, output_padding=1)).cuda().eval()
    x = torch.randn(8, 64, 32, 32, device="cuda")
    up_bytes = 8 * 64 * 65 * 65 * 4
    peak = {}
    with torch.no_grad():
        for path in ("native", "upsample"):
            L.set_transpose_path(path)
            layer(x, return_kl=False)      # warm-up: pack, workspaces
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = layer(x, return_kl=False)
            torch.cuda.synchronize()
            peak[path] = torch.cuda.max_memory_allocated() - base
            assert layer._last.get("x_path", "upsample") == path and tuple(out.shape) == (8, 8, 64, 64)
            del out
    print(f"peak allocation of one call: native {peak['native']} B, upsample {peak['upsample']} B, upsampled x {up_bytes} B")
    assert peak["native"] < up_bytes < peak["upsample"], peak


def test_decoder_under_mc_forward():
    """Conv2d -> ReLU -> ConvTranspose2d -> ReLU -> ConvTranspose2d, 16 channels, 8x8 input, S = 4, same seed on both paths."""
    import torch.nn as nn
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(11)
    # (dnn_to_bnn, like the reference, does not forward output_padding: 8x8 -> 15x15 -> 30x30)
    net = nn.Sequential(nn.Conv2d(16, 16, 3, padding=1), nn.ReLU(), nn.ConvTranspose2d(16, 16, 3, stride=2, padding=1), nn.ReLU(),
                        nn.ConvTranspose2d(16, 16, 2, stride=2))
    dnn_to_bnn(net, {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization",
                     "moped_enable": False, "moped_delta": 0.5})
    net = net.cuda().eval()
    x = torch.randn(4, 16, 8, 8, device="cuda")
    res = {}
    for path in ("native", "upsample"):
        L.set_transpose_path(path)
        rng.manual_seed(99)
        logits, kl = mc_forward(net, x, 4)
        res[path] = (logits, kl, [net[i]._last["kernel"] for i in (0, 2, 4)], [net[i]._last.get("x_path") for i in (2, 4)])
    (ln, kn, names_n, paths_n), (lu, ku, names_u, paths_u) = res["native"], res["upsample"]
    assert tuple(ln.shape) == (4, 4, 16, 30, 30) and paths_n == ["native", "native"] and paths_u == [None, None]
    assert names_n[0] == names_u[0] and all(_is_split(n) for n in names_n + names_u), (names_n, names_u)
    assert "xm=5" in names_n[1] and "xm=5" in names_n[2] and not any("xm=5" in n for n in names_u)
    assert [n.split(",xm=")[0] for n in names_n] == [n.split(",xm=")[0] for n in names_u]
    assert torch.equal(ln, lu) and torch.equal(kn, ku)      # (every launch ran the general split kernel on both paths)
