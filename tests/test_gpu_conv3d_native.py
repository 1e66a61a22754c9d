"""GPU: Conv3d on the "native" path -- the kernels read the real x through the depth-window fetch (bt_*_conv2d_dwin_fwd: xm 6 of the
general split kernel, the DWIN instantiations of fused_fwd_kernel) -- against the unfolding ("unfold") path and the fp64 oracle, an
ordinary conv3d, on the draws the layers report.

The geometries (tests/test_conv3d_native_host.py: ROWS) are the smallest that reach each thing that can go wrong:
  a   Reparam 8->24 k3 p(2,1,1), x [2,8,5,6,7]                 Cig*kd = 24; ragged last tile; windows with two of three depth taps in the padding
  b   Reparam 16->16 k(2,3,3) s(2,1,1) p(0,1,1) groups 2       depth stride; groups (x [2,16,10,5,5]: 10 launch images fill two 128-wide tiles --
                                                               with depth 6 the split planner declines the 59 %-filled tiles on BOTH paths)
  c   Reparam 8->16 k3 d(2,1,1) p(2,1,1) no bias               depth dilation
  d   Reparam 3->12 k3 p1                                      Cig*kd % 8 != 0: fused_fwd_kernel<..., dwin>
  e   Reparam 1->16 k(3,5,5) s(2,1,1) p(2,2,2)                 stem-like Cig*kd <= 4: the fp32 general kernel, never the quad kernel
  f1  Flipout 8->20 k(2,3,3) s(2,1,1) p(0,1,1)                 Flipout split tile, xm 6
  f2  Flipout 16->16 k3 p1 d(2,1,1) groups 2                   overlapping windows: the row whose signs are shared
Every row runs at S = 1, and at S = 3 with shared and with stacked x. The 256- and 512-wide tiles, which none of those plans picks,
have a test of their own. Tolerance: the project's rtol 1e-4, atol 1e-5 * max|ref| (conftest.assert_close)."""
import ctypes

import pytest
import torch

import _guard as G
from conftest import assert_close
from test_conv3d_native_host import _PRI, ROWS, make_layer

pytestmark = pytest.mark.gpu
ROW = {r[0]: r for r in ROWS}
# row a with 64 output channels: the variant that takes the 32-channel tiles
ROW["A"] = ("A", ROW["a"][1], dict(ROW["a"][2], out_channels=64), ROW["a"][3])
CASES = ((1, True), (3, True), (3, False))      # (S, shared x) of the three forwards of _runs


@pytest.fixture(autouse=True)
def _restore_switches():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import _lib, rng
    prev, mode = L.get_conv3d_path(), _lib.lib().bt_get_contraction()
    rng.set_mode("philox")
    yield
    L.set_conv3d_path(prev)
    _lib.lib().bt_set_contraction(mode)
    ctypes.CDLL(_lib.LIB_PATH).bt_debug_force_bn32(-1)


def _inputs(xshape, S=3):
    g = torch.Generator().manual_seed(3)
    return torch.randn(xshape, generator=g).cuda(), torch.randn((S * xshape[0],) + tuple(xshape[1:]), generator=g).cuda()


def _runs(layer, x, xs, path, S=3, seed=1234):
    """The three forwards of a row on ``path`` from the same RNG coordinates -> [(out, kl or None, _last, materialised draw)]."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    L.set_conv3d_path(path)
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


def _conv3d(layer):
    tup = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3
    return dict(stride=tup(layer.stride), padding=tup(layer.padding), dilation=tup(layer.dilation), groups=layer.groups)


def _oracle(layer, x, draws, S, shared):
    """fp64 conv3d of every sample in the REFERENCE's layouts, on the reported draws -> [S*B, Co, Do, Ho, Wo]. Flipout as the reference
    computes it: conv3d(x * sign_in, delta) * sign_out + conv3d(x, mu), ONE sign per element of x."""
    from oracle import bt_oracle as O
    t = lambda v: None if v is None else v.detach().double().cpu()
    p = dict(mu_w=t(layer.mu_kernel), rho_w=t(layer.rho_kernel), mu_b=t(layer.mu_bias), rho_b=t(layer.rho_bias))
    conv, x = _conv3d(layer), x.double().cpu()
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


def _launched(x):
    """The shape of the x a native call launches: the real x as [B, Ci * D, H, W]."""
    return (x.shape[0], x.shape[1] * x.shape[2], x.shape[3], x.shape[4])


@pytest.mark.parametrize("rid", ["a", "b", "c", "a-bn32", "A-bn32"])
def test_reparam_rows_equal_the_unfold_path_and_match_the_oracle(rid):
    from bayesian_torch_amd import _lib
    _, cls, ctor, xshape = ROW[rid[0]]
    if rid.endswith("bn32"):
        ctypes.CDLL(_lib.LIB_PATH).bt_debug_force_bn32(1)
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    nat, unf = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "unfold")
    for i, (n, u, (S, shared)) in enumerate(zip(nat, unf, CASES)):
        what, xin = f"{rid} run {i}", x if shared else xs
        assert n[2]["x_path"] == "native" and "x_path" not in u[2] and n[2]["x_shape"] == _launched(x) and u[2]["x_shape"] != _launched(x)
        assert n[2]["out_shape"] == u[2]["out_shape"] and n[2]["w_eq_shape"] == u[2]["w_eq_shape"]
        kn, ku = n[2]["kernel"], u[2]["kernel"]
        assert _is_split(kn) and "xm=6" in kn and "bf16x3" in kn, kn
        assert _is_split(ku) and "xm=6" not in ku, ku      # (every row was chosen so that the unfolded launch is the general split kernel's)
        assert kn.split(",xm=")[0] == ku.split(",xm=")[0]
        assert kn.startswith("fused_split_kernel<32,128," if rid == "A-bn32" else "fused_split_kernel<64,128,"), kn
        assert torch.equal(n[0], u[0]), f"{what}: {kn} vs {ku}: max abs {float((n[0] - u[0]).abs().max()):.3e}"
        assert torch.equal(n[3]["eps_w"], u[3]["eps_w"])
        if "eps_b" in n[3]:
            assert torch.equal(n[3]["eps_b"], u[3]["eps_b"])
        _check_oracle(layer, n, xin, S, shared, what)
    assert torch.equal(nat[0][1], unf[0][1]) and float(nat[0][1]) > 0      # KL


@pytest.mark.parametrize("rid", ["d", "e"])
def test_fp32_general_rows_match_the_oracle_and_the_unfold_path(rid):
    _, cls, ctor, xshape = ROW[rid]
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    nat, again, unf = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "native"), _runs(layer, x, xs, "unfold")
    for i, (n, r, u, (S, shared)) in enumerate(zip(nat, again, unf, CASES)):
        kn, ku = n[2]["kernel"], u[2]["kernel"]
        assert n[2]["x_path"] == "native" and n[2]["x_shape"] == _launched(x)
        assert kn.startswith("fused_fwd_kernel<") and kn.endswith(",dwin>"), kn
        assert "x_path" not in u[2] and not ku.endswith(",dwin>") and "xm=6" not in ku
        if rid == "e":
            assert ku.startswith("fused_split_quad_kernel<"), ku      # the stem kernel keeps the unfolded launch and never takes the window
        _check_oracle(layer, n, x if shared else xs, S, shared, f"{rid} run {i}")
        assert torch.equal(n[3]["eps_w"], u[3]["eps_w"])
        assert_close(n[0].cpu(), u[0].double().cpu(), 1e-4, 1e-5, f"{rid} run {i}: native vs unfold ({kn} vs {ku})")
        assert torch.equal(n[0], r[0]), f"{rid} run {i}: a re-run from the same coordinates differs"
    assert torch.equal(nat[0][1], unf[0][1])      # KL


@pytest.mark.parametrize("rid", ["f1", "f2"])
def test_flipout_rows_draw_one_sign_per_element_and_match_the_reference_formula(rid):
    """The tests that state the sign fix: sign_in is ONE sign per element of the real x, and the output is the reference's
    conv3d(x * sign_in, delta) * sign_out + conv3d(x, mu) on it. On f2 (kd 3, depth stride 1) every interior x element sits in three
    windows: the stream over the unfolded tensor gives it three independent signs and cannot satisfy this."""
    _, cls, ctor, xshape = ROW[rid]
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    nat, again = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "native")
    for i, (n, r, (S, shared)) in enumerate(zip(nat, again, CASES)):
        kn = n[2]["kernel"]
        assert n[2]["x_path"] == "native" and n[2]["x_shape"] == _launched(x)
        assert _is_split(kn) and ",flip," in kn and "xm=6" in kn, kn
        si, so = n[3]["sign_in"], n[3]["sign_out"]
        assert tuple(si.shape) == (S,) + tuple(x.shape) and bool((si.abs() == 1).all())
        assert tuple(so.shape) == (S, x.shape[0]) + tuple(n[0].shape[1:]) and bool((so.abs() == 1).all())
        assert "sign_in_eq" not in n[3] and "sign_out_eq" in n[3]
        assert 0.3 < float((si > 0).float().mean()) < 0.7
        _check_oracle(layer, n, x if shared else xs, S, shared, f"{rid} run {i}")
        assert torch.equal(n[0], r[0]), f"{rid} run {i}: a re-run from the same coordinates differs"
    unf = _runs(layer, x, xs, "unfold")      # the default path: the launch record and the sign keys it always had
    assert "x_path" not in unf[0][2] and "sign_in_eq" in unf[0][3] and "sign_in" not in unf[0][3] and "xm=6" not in unf[0][2]["kernel"]


# (class, constructor, x shape, S, the tile the plan picks): the 256- and 512-wide tiles (tests/test_conv3d_native_host.py's planner probe)
WIDE = [
    ("Conv3dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=3, padding=1, **_PRI), (4, 8, 4, 32, 32), 3, "<64,256,"),
    ("Conv3dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=3, padding=1, **_PRI), (8, 8, 4, 32, 32), 3, "<64,512,"),
    ("Conv3dFlipout", dict(in_channels=8, out_channels=16, kernel_size=3, padding=1), (4, 8, 4, 32, 32), 3, "<64,256,"),
]


@pytest.mark.parametrize("cls,ctor,xshape,S,tile", WIDE, ids=["r256", "r512", "f256"])
def test_wide_tiles(cls, ctor, xshape, S, tile):
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import mc, rng
    layer = make_layer(cls, ctor).cuda().eval()
    x, _ = _inputs(xshape, S=1)
    res = {}
    with torch.no_grad():
        for path in ("native", "unfold"):
            L.set_conv3d_path(path)
            rng.manual_seed(5)
            with mc.mc_samples(S, x.shape[0]):
                out = layer(x, return_kl=False)
            res[path] = (out, None, dict(layer._last), layer.materialize_last_draw())
    kn = res["native"][2]["kernel"]
    assert res["native"][2]["x_path"] == "native" and _is_split(kn) and tile in kn and "xm=6" in kn, kn
    assert tile in res["unfold"][2]["kernel"] and _is_split(res["unfold"][2]["kernel"])
    if not layer._flip:
        assert torch.equal(res["native"][0], res["unfold"][0])
    _check_oracle(layer, res["native"], x, S, True, f"wide {tile}")


def test_bf16_mode_takes_the_window_fetch():
    from bayesian_torch_amd import _lib
    _, cls, ctor, xshape = ROW["a"]
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    exact = _runs(layer, x, xs, "native")
    assert _lib.lib().bt_set_contraction(3) == 0
    nat, unf = _runs(layer, x, xs, "native"), _runs(layer, x, xs, "unfold")
    for n, u, e in zip(nat, unf, exact):
        kn, ku = n[2]["kernel"], u[2]["kernel"]
        assert _is_split(kn) and "bf16x1" in kn and "xm=6" in kn, kn
        assert _is_split(ku) and "bf16x1" in ku and "xm=6" not in ku, ku
        assert torch.equal(n[0], u[0]) and not torch.equal(n[0], e[0])


def test_grad_and_supplied_draws_unfold_and_the_default_records_no_path():
    import bayesian_torch_amd.layers as L
    _, cls, ctor, xshape = ROW["a"]
    layer = make_layer(cls, ctor).cuda()
    x, _ = _inputs(xshape)
    L.set_conv3d_path("native")
    out, _ = layer(x)      # grad enabled, parameters require grad
    assert layer._last["x_path"] == "unfold" and out.requires_grad and "xm=6" not in layer._last["kernel"]
    with torch.no_grad():
        ref, _ = layer(x)
        d = layer.materialize_last_draw()
        assert layer._last["x_path"] == "native"
        layer.inject_draw = dict(eps_w=d["eps_w"], eps_b=d["eps_b"])
        out2, _ = layer(x)
        layer.inject_draw = None
        assert layer._last["x_path"] == "unfold" and layer._last["x_shape"] != _launched(x)
        assert_close(out2.cpu(), ref.double().cpu(), 1e-4, 1e-5, "the reported draw, supplied again on the unfolding path")
        L.set_conv3d_path("unfold")
        layer(x)
        assert "x_path" not in layer._last


@pytest.mark.parametrize("rid", ["a", "d", "f1"])
def test_window_kernels_never_read_lds_they_did_not_write(rid):
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
    Lm.set_conv3d_path("native")
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


@pytest.mark.parametrize("rid", ["a", "f1"])
def test_guard_bands_around_the_real_x_and_the_output(rid):
    """The real x between NaN-filled bands at a 4-byte-aligned, not 16-byte-aligned base (S = 3, shared and stacked), `out` between canary
    bands at the same misalignment: the output equals the plain run's -- a read outside x that is used would poison it --, every output
    element is written and the canaries are intact."""
    import bayesian_torch_amd.layers as Lm
    from bayesian_torch_amd import mc, rng
    _, cls, ctor, xshape = ROW[rid]
    layer = make_layer(cls, ctor).cuda().eval()
    x, xs = _inputs(xshape)
    Lm.set_conv3d_path("native")
    with torch.no_grad():
        for xin, shared in ((x, True), (xs, False)):
            rng.manual_seed(31)
            with mc.mc_samples(3, x.shape[0]):
                plain = layer(xin, return_kl=False)
            assert layer._last["x_path"] == "native" and "xm=6" in layer._last["kernel"]
            xg = G.place(xin, 1)
            assert xg.data_ptr() % 16 == 4 and xg.is_contiguous()
            rng.manual_seed(31)
            with G.guarded_allocations(1) as log, mc.mc_samples(3, x.shape[0]):
                out = layer(xg, return_kl=False)
            torch.cuda.synchronize()
            assert layer._last["x_path"] == "native" and "xm=6" in layer._last["kernel"]
            assert len(log) >= 1 and log[0].view.data_ptr() % 16 == 4
            G.check_all(log)
            assert torch.isfinite(out).all() and torch.equal(out, plain), (rid, shared)


def test_native_call_allocates_less_than_the_unfolded_tensor():
    """The test that states the feature: Reparam 16->8 k3 p1 on [2,16,8,16,16], eval, no grad, after a warm-up call. The unfolded operand
    is 2*8 images of 16*3 channels of 16*16 floats; the native call's peak stays below that (it allocates its output, 131 KB, and the
    output's re-arranged copy), the unfolding call's exceeds it."""
    import bayesian_torch_amd.layers as L
    layer = make_layer("Conv3dReparameterization", dict(in_channels=16, out_channels=8, kernel_size=3, padding=1, **_PRI)).cuda().eval()
    x = torch.randn(2, 16, 8, 16, 16, device="cuda")
    unf = 2 * 8 * 16 * 3 * 16 * 16 * 4
    peak = {}
    with torch.no_grad():
        for path in ("native", "unfold"):
            L.set_conv3d_path(path)
            layer(x, return_kl=False)      # warm-up: pack, workspaces
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = layer(x, return_kl=False)
            torch.cuda.synchronize()
            peak[path] = torch.cuda.max_memory_allocated() - base
            assert layer._last.get("x_path", "unfold") == path and tuple(out.shape) == (2, 8, 8, 16, 16)
            del out
    print(f"peak allocation of one call: native {peak['native']} B, unfold {peak['unfold']} B, unfolded x {unf} B")
    assert peak["native"] < unf < peak["unfold"], peak


def test_video_block_under_mc_forward():
    """Conv3d(8->8, k3, p1) -> ReLU -> Conv3d(8->16, k3, s(2,1,1), p1) through dnn_to_bnn, under mc_forward, S = 4, x [2,8,4,6,6], the same
    seed on both paths. The first layer (8 launch images of 36 pixels per sample) runs the general split kernel on both paths: its
    output, and so the second layer's input, is the same bits. The second layer has 4 launch images of 36 pixels per sample: its
    128-wide tiles would be 56 % filled, below the split planner's 75 %, so -- on BOTH paths, the plan being that of the unfolded
    geometry -- it is an fp32 launch: the fast kernel over the unfolded x, the general kernel's dwin form over the real x. Those two
    accumulate the same fp32 products in different orders, so the logits are held to the project's tolerance, not to bit equality. KL
    comes from the parameters alone and is equal."""
    import torch.nn as nn
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import mc_forward
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(11)
    net = nn.Sequential(nn.Conv3d(8, 8, 3, padding=1), nn.ReLU(), nn.Conv3d(8, 16, 3, stride=(2, 1, 1), padding=1))
    dnn_to_bnn(net, {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization",
                     "moped_enable": False, "moped_delta": 0.5})
    net = net.cuda().eval()
    x = torch.randn(2, 8, 4, 6, 6, device="cuda")
    res = {}
    for path in ("native", "unfold"):
        L.set_conv3d_path(path)
        rng.manual_seed(99)
        logits, kl = mc_forward(net, x, 4)
        res[path] = (logits, kl, [net[i]._last["kernel"] for i in (0, 2)], [net[i]._last.get("x_path") for i in (0, 2)])
    (ln, kn, names_n, paths_n), (lu, ku, names_u, paths_u) = res["native"], res["unfold"]
    assert tuple(ln.shape) == (4, 2, 16, 2, 6, 6) and paths_n == ["native", "native"] and paths_u == [None, None]
    assert _is_split(names_n[0]) and _is_split(names_u[0]) and "xm=6" in names_n[0] and names_n[0].split(",xm=")[0] == names_u[0].split(",xm=")[0]
    assert names_n[1].startswith("fused_fwd_kernel<") and names_n[1].endswith(",dwin>") and names_u[1].startswith("fused_fast_kernel<"), (names_n, names_u)
    assert torch.equal(kn, ku)
    assert_close(ln.cpu(), lu.double().cpu(), 1e-4, 1e-5, "logits, native vs unfold")
