"""CPU: the input-dilated convolution entry points (bt_*_conv2d_updil_fwd) and the ConvTranspose "native" path's host side.

``bt_debug_plan_only(1)`` makes ``launch_kernel`` record the kernel name and return before it touches the runtime, so a forward call with
made-up aligned addresses runs the whole host chain -- argument checks, eligibility, tile planner, instantiation table -- on any machine
(tests/test_split_plan_parity.py). A dilated launch must plan exactly what the Conv2d launch over the materialised (virtual) image plans,
and differ from it in the x fetch alone. The GPU side is tests/test_gpu_convt_native.py; both files share the geometry table below."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000000          # any non-null, 16-byte aligned address

# (id, class, constructor, input shape): the smallest geometries that reach each thing that can go wrong (test_gpu_convt_native.py)
ROWS = [
    ("a", "ConvTranspose2dReparameterization", dict(in_channels=16, out_channels=24, kernel_size=3, stride=2, padding=1, output_padding=1), (3, 16, 9, 11)),
    ("b", "ConvTranspose2dReparameterization", dict(in_channels=16, out_channels=16, kernel_size=(3, 2), stride=(2, 1), padding=(1, 0), dilation=(1, 2), groups=2),
     (4, 16, 4, 7)),
    ("c", "ConvTranspose1dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=5, stride=3, padding=2, output_padding=2), (4, 8, 17)),
    ("d", "ConvTranspose2dReparameterization", dict(in_channels=64, out_channels=32, kernel_size=2, stride=2), (2, 64, 4, 4)),
    ("e", "ConvTranspose2dReparameterization", dict(in_channels=6, out_channels=4, kernel_size=3, stride=2, padding=1, output_padding=1), (2, 6, 9, 8)),
    ("f2", "ConvTranspose2dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, stride=2, padding=1, output_padding=1, groups=2), (2, 16, 6, 5)),
    ("f1", "ConvTranspose1dFlipout", dict(in_channels=8, out_channels=8, kernel_size=5, stride=3, padding=2, output_padding=2, bias=False), (4, 8, 17)),
]
CROP_ROW = ("g", "ConvTranspose2dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=3, stride=2, padding=3), (2, 8, 9, 9))


def make_layer(cls, ctor, seed=7):
    import bayesian_torch_amd.layers as L
    torch.manual_seed(seed)
    layer = getattr(L, cls)(**ctor)
    with torch.no_grad():      # rho spread out, so sigma*eps is not a small correction of mu (a wrong draw must show)
        layer.rho_kernel.uniform_(-2.5, -0.5)
        if layer.rho_bias is not None:
            layer.rho_bias.uniform_(-2.5, -0.5)
    return layer


@pytest.fixture()
def plan_only():
    from bayesian_torch_amd import _lib
    L, h = _lib.lib(), C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
    before = L.bt_get_contraction()
    h.bt_debug_plan_only(1)
    try:
        yield _lib, L, h
    finally:
        h.bt_debug_force_bn32(-1)
        h.bt_debug_plan_only(0)
        L.bt_set_contraction(before)


def _call(m, L, flip, geom, S, xss, updil=None, draws=None, pool=False):
    """One plan-only forward -> (rc, kernel name, the 16 launch-info integers)."""
    par = m.bt_params(P, P, P, P, P, P, P, P, P, P, 0, 0)
    draws = draws or m.bt_draws(None, None, None, None, m.bt_rng(1, None, 0, 1, 0, 0))
    ep = m.bt_epilogue(None, None, None, 0, 0, 1) if pool else None
    tail = (S, P, xss, C.byref(par), C.byref(draws), C.byref(ep) if ep else None, P, P, P, m.WORKSPACE_BYTES, None)
    if updil is None:
        rc = (L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd)(C.byref(geom), *tail)
    else:
        rc = (L.bt_flipout_conv2d_updil_fwd if flip else L.bt_reparam_conv2d_updil_fwd)(C.byref(geom), C.byref(updil), *tail)
    info = (C.c_int64 * 16)()
    L.bt_last_launch_info(info, 16)
    return rc, L.bt_last_kernel_name().decode(), tuple(int(v) for v in info)


def _geoms(m, layer, xshape):
    """The layer's two launches: (real geometry, bt_updil) of the native path, and the Conv2d geometry over the materialised image."""
    x = torch.zeros(xshape)
    xn, conv, _ = layer._x_native(x)
    xe, conv_e, _ = layer._x_eq(x)
    Co, _, kh, kw = layer._w_eq(layer.mu_kernel.detach()).shape
    g_nat = m.bt_conv2d_geom(xn.shape[0], xn.shape[1], xn.shape[2], xn.shape[3], Co, kh, kw, *conv["stride"], 0, 0, *conv["dilation"], conv["groups"])
    g_eq = m.bt_conv2d_geom(xe.shape[0], xe.shape[1], xe.shape[2], xe.shape[3], Co, kh, kw, *conv_e["stride"], *conv_e["padding"], *conv_e["dilation"], conv_e["groups"])
    return g_nat, m.bt_updil(*conv["updil"], *conv["pads"]), g_eq


def test_entry_points_exist_and_agree_with_the_header():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in ("bt_reparam_conv2d_updil_fwd", "bt_flipout_conv2d_updil_fwd"):
        assert name in _lib.EXPORTS and hasattr(handle, name)
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        assert decl.count(",") + 1 == len(_lib._PROTOS[name][1]) == 13       # bt_*_conv2d_fwd's twelve arguments + the bt_updil
        assert re.match(r"const bt_conv2d_geom \*g, const bt_updil \*u, int32_t S,", decl)
    fields = re.search(r"typedef struct bt_updil \{(.*?)\} bt_updil;", hdr, flags=re.S).group(1)
    names = re.findall(r"\b([a-z]+(?:_[a-z])?)\b(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [n for n, _ in _lib.bt_updil._fields_] == ["uh", "uw", "lo_h", "hi_h", "lo_w", "hi_w"]
    assert C.sizeof(_lib.bt_updil) == 24 and C.sizeof(_lib.bt_conv2d_geom) == 56 and _lib.lib().bt_version() == 302


def test_bad_arguments_are_refused_before_any_launch(plan_only):
    m, L, _ = plan_only
    g = m.bt_conv2d_geom(2, 16, 5, 5, 16, 3, 3, 1, 1, 0, 0, 1, 1, 1)
    ok = _call(m, L, False, g, 1, 0, m.bt_updil(2, 2, 1, 2, 1, 2))
    assert ok[0] == 0 and "xm=5" in ok[1]
    bad = [m.bt_updil(0, 2, 1, 1, 1, 1), m.bt_updil(2, 0, 1, 1, 1, 1), m.bt_updil(2, 2, -1, 1, 1, 1), m.bt_updil(2, 2, 1, -1, 1, 1),
           m.bt_updil(2, 2, 1, 1, -1, 1), m.bt_updil(2, 2, 1, 1, 1, -2)]
    for flip in (False, True):
        for u in bad:
            assert _call(m, L, flip, g, 1, 0, u)[0] == -1
            assert b"conv2d_updil_fwd" in L.bt_last_error_string()
        gp = m.bt_conv2d_geom(2, 16, 5, 5, 16, 3, 3, 1, 1, 1, 0, 1, 1, 1)
        assert _call(m, L, flip, gp, 1, 0, m.bt_updil(2, 2, 1, 1, 1, 1))[0] == -1        # ph != 0
        gp = m.bt_conv2d_geom(2, 16, 5, 5, 16, 3, 3, 1, 1, 0, 2, 1, 1, 1)
        assert _call(m, L, flip, gp, 1, 0, m.bt_updil(2, 2, 1, 1, 1, 1))[0] == -1        # pw != 0
        fn = L.bt_flipout_conv2d_updil_fwd if flip else L.bt_reparam_conv2d_updil_fwd
        assert fn(C.byref(g), None, 1, P, 0, None, None, None, P, None, None, 0, None) == -1      # no bt_updil
    # supplied draws (natural or packed layout) and the fused max-pool: BT_ERR_UNSUPPORTED, nothing launched
    u = m.bt_updil(2, 2, 1, 2, 1, 2)
    assert _call(m, L, False, g, 1, 0, u, draws=m.bt_draws(P, P, None, None, m.bt_rng(1, None, 0, 1, 0, 0)))[0] == -2
    assert _call(m, L, False, g, 1, 0, u, draws=m.bt_draws(P, P, None, None, m.bt_rng(1, None, 0, 1, 0, m.DRAWS_EPS_PACKED)))[0] == -2
    assert _call(m, L, True, g, 1, 0, u, draws=m.bt_draws(P, P, P, P, m.bt_rng(1, None, 0, 1, 0, m.DRAWS_EPS_PACKED | m.DRAWS_SIGNS_PACKED)))[0] == -2
    assert _call(m, L, False, g, 1, 0, u, pool=True)[0] == -2
    # nothing was recorded by any refused call: the name and the plan are still the first call's
    assert _last(m, L) == ok[1:]


def _last(m, L):
    info = (C.c_int64 * 16)()
    L.bt_last_launch_info(info, 16)
    return L.bt_last_kernel_name().decode(), tuple(int(v) for v in info)


def _strip_fetch(name):
    return re.sub(r",updil>$", ">", re.sub(r"xm=\d", "xm=*", name))


@pytest.mark.parametrize("rid,cls,ctor,xshape", ROWS, ids=[r[0] for r in ROWS])
def test_dilated_launch_plans_what_the_materialised_launch_plans(plan_only, rid, cls, ctor, xshape):
    """Plan, kernel name apart from the fetch, and launch info of the dilated launch equal those of the Conv2d launch on the virtual
    geometry wherever that one runs the general split kernel or fused_fwd_kernel; a launch the stem / direct / split-K / fast kernels
    would take runs one of those two instead. S = 1 and 3, shared and stacked x; 32-channel tiles automatic and forced on."""
    m, L, h = plan_only
    layer = make_layer(cls, ctor)
    flip = layer._flip
    g_nat, u, g_eq = _geoms(m, layer, xshape)
    n_nat, n_eq = g_nat.B * g_nat.Ci * g_nat.H * g_nat.W, g_eq.B * g_eq.Ci * g_eq.H * g_eq.W
    assert g_eq.H == (g_nat.H - 1) * u.uh + 1 + u.lo_h + u.hi_h and g_eq.W == (g_nat.W - 1) * u.uw + 1 + u.lo_w + u.hi_w
    compared = 0
    for mode in ((0,) if flip else (0, 3)):
        assert L.bt_set_contraction(mode) == 0
        for bn32 in (-1, 1):
            h.bt_debug_force_bn32(bn32)
            for S, stacked in ((1, False), (3, False), (3, True)):
                rc_e, name_e, info_e = _call(m, L, flip, g_eq, S, n_eq if stacked else 0)
                rc_n, name_n, info_n = _call(m, L, flip, g_nat, S, n_nat if stacked else 0, u)
                assert rc_e == 0 and rc_n == 0
                assert name_n.startswith(("fused_split_kernel<", "fused_fwd_kernel<")), name_n
                assert ("xm=5" in name_n) if name_n.startswith("fused_split_kernel<") else name_n.endswith(",updil>")
                if mode == 3 and name_n.startswith("fused_split_kernel<"):
                    assert "bf16x1" in name_n
                if name_e.startswith(("fused_split_kernel<", "fused_fwd_kernel<")):
                    assert _strip_fetch(name_n) == _strip_fetch(name_e) and info_n == info_e, (rid, mode, S, stacked)
                    compared += 1
    if rid != "e":      # (6 channels per group: the materialised launch is the fp32 fast kernel's)
        assert compared == (6 if flip else 12)
    else:
        assert name_n.startswith("fused_fwd_kernel<") and name_e.startswith("fused_fast_kernel<")


def test_stem_direct_skinny_and_fast_launches_fall_to_the_two_general_kernels(plan_only):
    m, L, _ = plan_only
    L.bt_set_contraction(0)
    u2 = m.bt_updil(2, 2, 0, 0, 0, 0)
    # (geometry of the dilated launch, its bt_updil, prefix of the materialised launch's kernel, of the dilated launch's)
    cases = [
        (m.bt_conv2d_geom(8, 3, 16, 16, 32, 3, 3, 1, 1, 0, 0, 1, 1, 1), m.bt_updil(2, 2, 1, 2, 1, 2), "fused_split_quad_kernel<", "fused_fwd_kernel<"),      # stem
        (m.bt_conv2d_geom(8, 64, 8, 8, 64, 1, 1, 1, 1, 0, 0, 1, 1, 1), u2, "fused_split_direct_kernel<", "fused_split_kernel<"),                            # 1x1 kernel
        (m.bt_conv2d_geom(8, 6, 8, 8, 16, 3, 3, 1, 1, 0, 0, 1, 1, 1), m.bt_updil(2, 2, 1, 1, 1, 1), "fused_fast_kernel<", "fused_fwd_kernel<"),              # Cig % 8 != 0
        (m.bt_conv2d_geom(256, 64, 8, 8, 64, 3, 3, 1, 1, 0, 0, 1, 1, 1), m.bt_updil(2, 2, 1, 1, 1, 1), "fused_split_kernel<", "fused_split_kernel<"),
    ]
    for g, u, want_e, want_n in cases:
        Hv, Wv = (g.H - 1) * u.uh + 1 + u.lo_h + u.hi_h, (g.W - 1) * u.uw + 1 + u.lo_w + u.hi_w
        g_eq = m.bt_conv2d_geom(g.B, g.Ci, Hv, Wv, g.Co, g.kh, g.kw, g.sh, g.sw, 0, 0, g.dh, g.dw, g.groups)
        for flip in (False, True):
            rc_e, name_e, _ = _call(m, L, flip, g_eq, 2, 0)
            rc_n, name_n, _ = _call(m, L, flip, g, 2, 0, u)
            assert rc_e == 0 and rc_n == 0
            if not flip:
                assert name_e.startswith(want_e), name_e
            assert name_n.startswith(want_n if not flip or want_n == "fused_fwd_kernel<" else ("fused_split_kernel<", "fused_fwd_kernel<")), name_n
            assert "xm=5" in name_n or name_n.endswith(",updil>")
    # f32 and bf16x2 contraction modes have no dilated split instantiation: the fp32 general kernel
    g, u = cases[3][0], cases[3][1]
    for mode in (1, 2):
        L.bt_set_contraction(mode)
        assert _call(m, L, False, g, 2, 0, u)[1].startswith("fused_fwd_kernel<") and L.bt_last_kernel_name().decode().endswith(",updil>")
    # no dilation and no padding: the plain convolution, launch for launch
    L.bt_set_contraction(0)
    assert _call(m, L, False, g, 2, 0, m.bt_updil(1, 1, 0, 0, 0, 0))[1:] == _call(m, L, False, g, 2, 0)[1:]


def test_switch_names_and_environment_variable():
    import bayesian_torch_amd.layers as L
    assert L.get_transpose_path() == os.environ.get("BT_CONVT_PATH", "upsample")
    prev = L.set_transpose_path("native")
    try:
        assert L.get_transpose_path() == "native" and L.set_transpose_path("upsample") == "native"
        with pytest.raises(ValueError, match="set_transpose_path"):
            L.set_transpose_path("fast")
        assert L.get_transpose_path() == "upsample"
    finally:
        L.set_transpose_path(prev)
    code = "import bayesian_torch_amd.layers as L; print(L.get_transpose_path())"
    for value, want in (("native", "native"), (None, "upsample")):
        env = {k: v for k, v in os.environ.items() if k != "BT_CONVT_PATH"}
        if value is not None:
            env["BT_CONVT_PATH"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, r.stderr
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, BT_CONVT_PATH="bogus"), capture_output=True, text=True)
    assert r.returncode != 0 and "BT_CONVT_PATH" in r.stderr


def test_eligibility_rule():
    import bayesian_torch_amd.layers as L
    prev = L.set_transpose_path("native")
    try:
        for _, cls, ctor, _ in ROWS:
            layer = make_layer(cls, ctor)
            assert layer._native_eligible(False, False)
            assert not layer._native_eligible(True, False)        # grad: the backward kernels have no dilation
            assert not layer._native_eligible(False, True)        # a supplied draw
        assert not make_layer(*CROP_ROW[1:3])._native_eligible(False, False)      # d*(k-1) - p < 0: a crop
        assert not make_layer("ConvTranspose1dFlipout", dict(in_channels=8, out_channels=8, kernel_size=5, stride=3, padding=6, output_padding=2))._native_eligible(False, False)
        assert not L.ConvTranspose3dReparameterization(4, 8, 3, stride=2)._native_eligible(False, False)
        assert not L.ConvTranspose3dFlipout(4, 8, 3, stride=2)._native_eligible(False, False)
        assert not L.Conv3dFlipout(4, 8, 3)._native_eligible(False, False)
        L.set_transpose_path("upsample")
        assert not make_layer(*ROWS[0][1:3])._native_eligible(False, False)       # the default: every launch as before
    finally:
        L.set_transpose_path(prev)


@pytest.mark.parametrize("rid,cls,ctor,xshape", ROWS, ids=[r[0] for r in ROWS])
def test_x_eq_is_the_virtual_image_of_the_struct(rid, cls, ctor, xshape):
    """_x_eq's tensor IS the image (uh, uw, lo, hi) describe: same size, x at the lattice points behind the leading pads, zeros elsewhere."""
    layer = make_layer(cls, ctor)
    x = torch.arange(1, 1 + torch.Size(xshape).numel(), dtype=torch.float32).reshape(xshape)
    xe, conv_e, _ = layer._x_eq(x)
    xn, conv, _ = layer._x_native(x)
    (uh, uw), (lo_h, hi_h, lo_w, hi_w) = conv["updil"], conv["pads"]
    assert conv_e["stride"] == conv["stride"] == (1, 1) and tuple(conv_e["padding"]) == tuple(conv["padding"]) == (0, 0)
    assert tuple(conv_e["dilation"]) == tuple(conv["dilation"]) and conv_e["groups"] == conv["groups"]
    H, W = xn.shape[2:]
    assert tuple(xe.shape) == (xn.shape[0], xn.shape[1], (H - 1) * uh + 1 + lo_h + hi_h, (W - 1) * uw + 1 + lo_w + hi_w)
    virt = torch.zeros_like(xe)
    virt[:, :, lo_h:lo_h + (H - 1) * uh + 1:uh, lo_w:lo_w + (W - 1) * uw + 1:uw] = xn
    assert torch.equal(virt, xe)
