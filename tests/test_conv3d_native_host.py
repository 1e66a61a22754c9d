"""CPU: the depth-window convolution entry points (bt_*_conv2d_dwin_fwd) and the Conv3d "native" path's host side.

``bt_debug_plan_only(1)`` makes ``launch_kernel`` record the kernel name and return before it touches the runtime, so a forward call with
made-up aligned addresses runs the whole host chain -- argument checks, eligibility, tile planner, instantiation table -- on any machine
(tests/test_split_plan_parity.py). A depth-window launch must plan exactly what the Conv2d launch over the materialised (unfolded)
operand plans, and differ from it in the x fetch alone. The GPU side is tests/test_gpu_conv3d_native.py; both files share the table below."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000000          # any non-null, 16-byte aligned address
_PRI = dict(prior_mean=0.0, prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0)

# (id, class, constructor, input shape): the smallest geometries that reach each thing that can go wrong (test_gpu_conv3d_native.py)
ROWS = [
    ("a", "Conv3dReparameterization", dict(in_channels=8, out_channels=24, kernel_size=3, padding=(2, 1, 1), **_PRI), (2, 8, 5, 6, 7)),
    ("b", "Conv3dReparameterization", dict(in_channels=16, out_channels=16, kernel_size=(2, 3, 3), stride=(2, 1, 1), padding=(0, 1, 1), groups=2, **_PRI),
     (2, 16, 10, 5, 5)),
    ("c", "Conv3dReparameterization", dict(in_channels=8, out_channels=16, kernel_size=3, dilation=(2, 1, 1), padding=(2, 1, 1), bias=False, **_PRI), (3, 8, 7, 4, 4)),
    ("d", "Conv3dReparameterization", dict(in_channels=3, out_channels=12, kernel_size=3, padding=1, **_PRI), (2, 3, 5, 9, 9)),
    ("e", "Conv3dReparameterization", dict(in_channels=1, out_channels=16, kernel_size=(3, 5, 5), stride=(2, 1, 1), padding=(2, 2, 2), **_PRI), (2, 1, 6, 12, 12)),
    ("f1", "Conv3dFlipout", dict(in_channels=8, out_channels=20, kernel_size=(2, 3, 3), stride=(2, 1, 1), padding=(0, 1, 1)), (2, 8, 6, 10, 10)),
    ("f2", "Conv3dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, padding=1, dilation=(2, 1, 1), groups=2), (2, 16, 6, 5, 5)),
]
SPLIT_ROWS = ("a", "b", "c", "f1", "f2")      # Cig * kd is a multiple of 8 and > 4: the general split kernel, xm 6
FP32_ROWS = ("d", "e")                        # Cig * kd % 8 != 0 / <= 4: fused_fwd_kernel<..., dwin>


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


def _call(m, L, flip, geom, S, xss, dwin=None, draws=None, pool=False):
    """One plan-only forward -> (rc, kernel name, the 16 launch-info integers)."""
    par = m.bt_params(P, P, P, P, P, P, P, P, P, P, 0, 0)
    draws = draws or m.bt_draws(None, None, None, None, m.bt_rng(1, None, 0, 1, 0, 0))
    ep = m.bt_epilogue(None, None, None, 0, 0, 1) if pool else None
    tail = (S, P, xss, C.byref(par), C.byref(draws), C.byref(ep) if ep else None, P, P, P, m.WORKSPACE_BYTES, None)
    if dwin is None:
        rc = (L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd)(C.byref(geom), *tail)
    else:
        rc = (L.bt_flipout_conv2d_dwin_fwd if flip else L.bt_reparam_conv2d_dwin_fwd)(C.byref(geom), C.byref(dwin), *tail)
    info = (C.c_int64 * 16)()
    L.bt_last_launch_info(info, 16)
    return rc, L.bt_last_kernel_name().decode(), tuple(int(v) for v in info)


def _last(m, L):
    info = (C.c_int64 * 16)()
    L.bt_last_launch_info(info, 16)
    return L.bt_last_kernel_name().decode(), tuple(int(v) for v in info)


def _geoms(m, layer, xshape):
    """The layer's launch geometry (over the unfolded operand: the same struct on both paths), the bt_dwin of the native path, and the real
    and unfolded element counts of one sample's x. The native geometry comes from functional._geometry, as the forward builds it."""
    from bayesian_torch_amd import functional as F
    x = torch.zeros(xshape)
    xn, conv, _ = layer._x_native(x)
    xe, conv_e, _ = layer._x_eq(x)
    w = layer._w_eq(layer.mu_kernel.detach())
    Bn, g_nat, n_real, tail_n = F._geometry(xn, w, conv, 1, True)
    Be, g_eq, n_unf, tail_e = F._geometry(xe, w, conv_e, 1, True)
    assert Bn == Be == xe.shape[0] and tail_n == tail_e and n_real == x.numel() and n_unf == xe.numel()
    assert bytes(g_nat) == bytes(g_eq)      # g describes the Conv2d launch over the virtual operand, exactly as _x_eq would launch it
    return g_eq, m.bt_dwin(*conv["dwin"]), n_real, n_unf


def test_entry_points_exist_and_agree_with_the_header():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in ("bt_reparam_conv2d_dwin_fwd", "bt_flipout_conv2d_dwin_fwd"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(handle, name)
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        assert decl.count(",") + 1 == len(_lib._PROTOS[name][1]) == 13       # bt_*_conv2d_fwd's twelve arguments + the bt_dwin
        assert re.match(r"const bt_conv2d_geom \*g, const bt_dwin \*w, int32_t S,", decl)
    fields = re.search(r"typedef struct bt_dwin \{(.*?)\} bt_dwin;", hdr, flags=re.S).group(1)
    names = re.findall(r"\b([A-Za-z]+)\b(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [n for n, _ in _lib.bt_dwin._fields_] == ["kd", "D", "sd", "dd", "pd"]
    assert C.sizeof(_lib.bt_dwin) == 20 and C.sizeof(_lib.bt_conv2d_geom) == 56 and C.sizeof(_lib.bt_updil) == 24
    assert _lib.lib().bt_version() == 302


def test_bad_arguments_are_refused_before_any_launch(plan_only):
    m, L, _ = plan_only
    L.bt_set_contraction(0)
    # real [2, 8, 5, 5, 5], k3 p1 in every axis: Do = 5, 10 launch images of 24 channels
    g = m.bt_conv2d_geom(10, 24, 5, 5, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    ok = _call(m, L, False, g, 1, 0, m.bt_dwin(3, 5, 1, 1, 1))
    assert ok[0] == 0 and "xm=6" in ok[1]
    bad = [m.bt_dwin(0, 5, 1, 1, 1), m.bt_dwin(3, 0, 1, 1, 1), m.bt_dwin(3, 5, 0, 1, 1), m.bt_dwin(3, 5, 1, 0, 1), m.bt_dwin(3, 5, 1, 1, -1),
           m.bt_dwin(3, 1, 1, 1, 0),       # Do < 1: the window is longer than the depth
           m.bt_dwin(3, 5, 1, 2, 1),       # Do = 3: 10 launch images are no multiple of it
           m.bt_dwin(3, 6, 1, 1, 1),       # Do = 6: the same
           m.bt_dwin(5, 5, 1, 1, 2)]       # Do = 5, but 24 channels per group are no multiple of kd = 5
    for flip in (False, True):
        who = b"bt_flipout_conv2d_dwin_fwd" if flip else b"bt_reparam_conv2d_dwin_fwd"
        for w in bad:
            assert _call(m, L, flip, g, 1, 0, w)[0] == -1, tuple(getattr(w, n) for n, _ in w._fields_)
            assert who in L.bt_last_error_string()
        gg = m.bt_conv2d_geom(10, 24, 6, 6, 16, 3, 3, 1, 1, 1, 1, 1, 1, 2)         # groups 2: 12 channels per group are a multiple of kd = 3 ...
        assert _call(m, L, flip, gg, 1, 0, m.bt_dwin(3, 5, 1, 1, 1))[0] == 0
        assert _call(m, L, flip, gg, 1, 0, m.bt_dwin(4, 5, 1, 1, 1))[0] == -1      # ... kd = 4: Do = 4 does not divide 10
        gg = m.bt_conv2d_geom(8, 24, 6, 6, 18, 3, 3, 1, 1, 1, 1, 1, 1, 3)          # 8 channels per group, kd = 3
        assert _call(m, L, flip, gg, 1, 0, m.bt_dwin(3, 4, 1, 1, 1))[0] == -1 and who in L.bt_last_error_string()
        # 2^30 elements: the unfolded x (1024 images x 2^20), and the real x alone (depth stride 2: 2048 planes behind 1024 windows)
        big = m.bt_conv2d_geom(1024, 1024, 32, 32, 8, 1, 1, 1, 1, 0, 0, 1, 1, 1)
        assert _call(m, L, flip, big, 1, 0, m.bt_dwin(1, 1024, 1, 1, 0))[0] == -1 and who in L.bt_last_error_string()
        big = m.bt_conv2d_geom(1024, 512, 32, 32, 8, 1, 1, 1, 1, 0, 0, 1, 1, 1)
        assert _call(m, L, flip, big, 1, 0, m.bt_dwin(1, 2047, 2, 1, 0))[0] == 0            # 2^29 unfolded, 2^29 - 2^19 real
        assert _call(m, L, flip, big, 1, 0, m.bt_dwin(1, 2048, 2, 1, 0))[0] == -1 and who in L.bt_last_error_string()
        fn = L.bt_flipout_conv2d_dwin_fwd if flip else L.bt_reparam_conv2d_dwin_fwd
        assert fn(C.byref(g), None, 1, P, 0, None, None, None, P, None, None, 0, None) == -1 and who in L.bt_last_error_string()      # no bt_dwin
        assert fn(None, C.byref(m.bt_dwin(3, 5, 1, 1, 1)), 1, P, 0, None, None, None, P, None, None, 0, None) == -1
    ok = _call(m, L, False, g, 1, 0, m.bt_dwin(3, 5, 1, 1, 1))
    # supplied draws (natural or packed layout) and the fused max-pool: BT_ERR_UNSUPPORTED, nothing launched
    w = m.bt_dwin(3, 5, 1, 1, 1)
    for rc in (_call(m, L, False, g, 1, 0, w, draws=m.bt_draws(P, P, None, None, m.bt_rng(1, None, 0, 1, 0, 0)))[0],
               _call(m, L, False, g, 1, 0, w, draws=m.bt_draws(P, P, None, None, m.bt_rng(1, None, 0, 1, 0, m.DRAWS_EPS_PACKED)))[0],
               _call(m, L, False, g, 1, 0, w, pool=True)[0]):
        assert rc == -2 and b"bt_reparam_conv2d_dwin_fwd" in L.bt_last_error_string()
    for rc in (_call(m, L, True, g, 1, 0, w, draws=m.bt_draws(P, P, P, P, m.bt_rng(1, None, 0, 1, 0, 0)))[0],
               _call(m, L, True, g, 1, 0, w, draws=m.bt_draws(P, P, P, P, m.bt_rng(1, None, 0, 1, 0, m.DRAWS_EPS_PACKED | m.DRAWS_SIGNS_PACKED)))[0],
               _call(m, L, True, g, 1, 0, w, pool=True)[0]):
        assert rc == -2 and b"bt_flipout_conv2d_dwin_fwd" in L.bt_last_error_string()
    # nothing was recorded by any refused call: the name and the plan are still the last good call's
    assert _last(m, L) == ok[1:]


def _strip_fetch(name):
    return re.sub(r",dwin>$", ">", re.sub(r"xm=\d", "xm=*", name))


@pytest.mark.parametrize("rid,cls,ctor,xshape", ROWS, ids=[r[0] for r in ROWS])
def test_window_launch_plans_what_the_unfolded_launch_plans(plan_only, rid, cls, ctor, xshape):
    """Plan, kernel name apart from the fetch, and launch info of the depth-window launch equal those of the Conv2d launch on the unfolded
    geometry wherever that one runs the general split kernel or fused_fwd_kernel; a launch the stem / fast kernels would take runs
    fused_fwd_kernel<..., dwin> instead. S = 1 and 3, shared and stacked x; 32-channel tiles automatic and forced on."""
    m, L, h = plan_only
    layer = make_layer(cls, ctor)
    flip = layer._flip
    g, w, n_real, n_unf = _geoms(m, layer, xshape)
    compared = 0
    for mode in ((0,) if flip else (0, 3)):
        assert L.bt_set_contraction(mode) == 0
        for bn32 in (-1, 1):
            h.bt_debug_force_bn32(bn32)
            for S, stacked in ((1, False), (3, False), (3, True)):
                rc_e, name_e, info_e = _call(m, L, flip, g, S, n_unf if stacked else 0)
                rc_n, name_n, info_n = _call(m, L, flip, g, S, n_real if stacked else 0, w)
                assert rc_e == 0 and rc_n == 0
                if rid in SPLIT_ROWS:
                    assert name_n.startswith("fused_split_kernel<") and "xm=6" in name_n, name_n
                    assert name_e.startswith("fused_split_kernel<") and "xm=6" not in name_e, name_e
                    assert ("bf16x1" if mode == 3 else "bf16x3") in name_n
                    assert (",flip," in name_n) == flip
                else:
                    assert name_n.startswith("fused_fwd_kernel<") and name_n.endswith(",dwin>"), name_n
                if name_e.startswith(("fused_split_kernel<", "fused_fwd_kernel<")):
                    assert _strip_fetch(name_n) == _strip_fetch(name_e) and info_n == info_e, (rid, mode, S, stacked, name_n, name_e)
                    compared += 1
    if rid in SPLIT_ROWS:
        assert compared == (6 if flip else 12)
    elif rid == "d":      # (9 channels per group: the unfolded launch is the fp32 fast kernel's)
        assert name_e.startswith("fused_fast_kernel<"), name_e
    else:                 # (3 channels per group: the unfolded launch is the stem kernel's)
        assert name_e.startswith("fused_split_quad_kernel<"), name_e


def test_stem_direct_skinny_fast_and_pooled_launches_never_take_a_window(plan_only):
    m, L, h = plan_only
    L.bt_set_contraction(0)
    # (launch geometry over the unfolded operand, bt_dwin, prefix of the unfolded launch's kernel, of the window launch's)
    cases = [
        (m.bt_conv2d_geom(8 * 4, 3, 16, 16, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1), m.bt_dwin(3, 4, 1, 1, 1), "fused_split_quad_kernel<", "fused_fwd_kernel<"),    # stem: 1 x 3
        (m.bt_conv2d_geom(8 * 4, 64, 8, 8, 64, 1, 1, 1, 1, 0, 0, 1, 1, 1), m.bt_dwin(2, 5, 1, 1, 0), "fused_split_direct_kernel<", "fused_split_kernel<"),  # 1x1 in space
        (m.bt_conv2d_geom(8 * 2, 512, 1, 1, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1), m.bt_dwin(2, 3, 1, 1, 0), "fused_split_skinny_kernel<", "fused_fwd_kernel<"),    # one-pixel maps, split-K
        (m.bt_conv2d_geom(8 * 5, 9, 8, 8, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1), m.bt_dwin(3, 5, 1, 1, 1), "fused_fast_kernel<", "fused_fwd_kernel<"),              # Cig % 8 != 0
        (m.bt_conv2d_geom(64 * 4, 24, 8, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1), m.bt_dwin(3, 4, 1, 1, 1), "fused_split_kernel<", "fused_split_kernel<"),
    ]
    for g, w, want_e, want_n in cases:
        for flip in (False, True):
            scratch = int(L.bt_fused_scratch_bytes(C.byref(g), 2))
            rc_e, name_e, _ = _call_ws(m, L, flip, g, 2, None, scratch)
            rc_n, name_n, _ = _call_ws(m, L, flip, g, 2, w, scratch)
            assert rc_e == 0 and rc_n == 0
            if not flip:
                assert name_e.startswith(want_e), name_e
            assert name_n.startswith(want_n if not flip or want_n == "fused_fwd_kernel<" else ("fused_split_kernel<", "fused_fwd_kernel<")), name_n
            assert "xm=6" in name_n or name_n.endswith(",dwin>"), name_n
    # f32 and bf16x2 contraction modes have no windowed split instantiation: the fp32 general kernel
    g, w = cases[4][0], cases[4][1]
    for mode in (1, 2):
        L.bt_set_contraction(mode)
        assert _call(m, L, False, g, 2, 0, w)[1].startswith("fused_fwd_kernel<") and L.bt_last_kernel_name().decode().endswith(",dwin>")
    L.bt_set_contraction(0)
    # the fused max-pool: refused (bt_*_conv2d_fwd pools this launch)
    gp = m.bt_conv2d_geom(8 * 4, 24, 16, 16, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    assert _call(m, L, False, gp, 2, 0, pool=True)[0] == 0
    assert _call(m, L, False, gp, 2, 0, m.bt_dwin(3, 4, 1, 1, 1), pool=True)[0] == -2
    # one depth tap over one plane, no padding: the plain convolution, launch for launch
    for flip in (False, True):
        assert _call(m, L, flip, g, 2, 0, m.bt_dwin(1, 1, 1, 1, 0))[1:] == _call(m, L, flip, g, 2, 0)[1:]
        assert _call(m, L, flip, g, 2, 0, m.bt_dwin(1, 1, 3, 2, 0))[1:] == _call(m, L, flip, g, 2, 0)[1:]


def _call_ws(m, L, flip, geom, S, dwin, scratch):
    """_call with the split-K scratch behind the workspace that the Conv2d launch may want (the window launch asks for none)."""
    par = m.bt_params(P, P, P, P, P, P, P, P, P, P, 0, 0)
    draws = m.bt_draws(None, None, None, None, m.bt_rng(1, None, 0, 1, 0, 0))
    tail = (S, P, 0, C.byref(par), C.byref(draws), None, P, P, P, m.WORKSPACE_BYTES + scratch, None)
    if dwin is None:
        rc = (L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd)(C.byref(geom), *tail)
    else:
        rc = (L.bt_flipout_conv2d_dwin_fwd if flip else L.bt_reparam_conv2d_dwin_fwd)(C.byref(geom), C.byref(dwin), *tail)
    return (rc,) + _last(m, L)


def test_switch_names_and_environment_variable():
    import bayesian_torch_amd.layers as L
    assert L.get_conv3d_path() == os.environ.get("BT_CONV3D_PATH", "unfold")
    prev = L.set_conv3d_path("native")
    try:
        assert L.get_conv3d_path() == "native" and L.set_conv3d_path("unfold") == "native"
        with pytest.raises(ValueError, match="set_conv3d_path"):
            L.set_conv3d_path("upsample")
        assert L.get_conv3d_path() == "unfold"
        L.set_conv3d_path("native")
        assert L.get_transpose_path() == os.environ.get("BT_CONVT_PATH", "upsample")      # the two switches are independent
    finally:
        L.set_conv3d_path(prev)
    code = "import bayesian_torch_amd.layers as L; print(L.get_conv3d_path())"
    for value, want in (("native", "native"), ("unfold", "unfold"), (None, "unfold")):
        env = {k: v for k, v in os.environ.items() if k != "BT_CONV3D_PATH"}
        if value is not None:
            env["BT_CONV3D_PATH"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, r.stderr
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, BT_CONV3D_PATH="bogus"), capture_output=True, text=True)
    assert r.returncode != 0 and "BT_CONV3D_PATH" in r.stderr


def test_eligibility_rule(plan_only):
    """The rule on the layer, and the launch the eligible call makes -- through functional's geometry step -- with the kernels stubbed."""
    import bayesian_torch_amd.layers as Lm
    m, L, _ = plan_only
    L.bt_set_contraction(0)
    prev, prev_t = Lm.set_conv3d_path("native"), Lm.get_transpose_path()
    try:
        for rid, cls, ctor, xshape in ROWS:
            layer = make_layer(cls, ctor)
            assert layer._native_setting()
            assert layer._native_eligible(False, False)
            assert not layer._native_eligible(True, False)        # grad: the backward kernels have no depth map
            assert not layer._native_eligible(False, True)        # a supplied draw, or rng mode "torch"
            g, w, n_real, _ = _geoms(m, layer, xshape)
            rc, name, _ = _call(m, L, layer._flip, g, 1, 0, w)
            assert rc == 0 and ("xm=6" in name if rid in SPLIT_ROWS else name.endswith(",dwin>")), (rid, name)
        # the switch is Conv3d's alone
        assert not Lm.ConvTranspose3dReparameterization(4, 8, 3, stride=2)._native_eligible(False, False)
        assert not Lm.ConvTranspose2dFlipout(8, 8, 3, stride=2)._native_eligible(False, False)
        assert not Lm.ConvTranspose2dFlipout(8, 8, 3, stride=2)._native_setting()
        with pytest.raises(NotImplementedError):      # string padding: refused as on the unfolding path
            make_layer("Conv3dFlipout", dict(in_channels=8, out_channels=8, kernel_size=3, padding="same"))._x_native(torch.zeros(1, 8, 4, 4, 4))
        Lm.set_transpose_path("native")
        Lm.set_conv3d_path("unfold")
        layer = make_layer(*ROWS[0][1:3])
        assert not layer._native_eligible(False, False) and not layer._native_setting()      # the default: every launch as before
    finally:
        Lm.set_conv3d_path(prev)
        Lm.set_transpose_path(prev_t)


def test_functional_validates_the_window():
    from bayesian_torch_amd import functional as F
    w = torch.zeros(16, 24, 3, 3)
    x = torch.zeros(2, 8 * 5, 6, 6)
    conv = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1)
    B, g, n, tail = F._geometry(x, w, dict(conv, dwin=(3, 5, 1, 1, 1)), 1, True)
    assert (B, g.B, g.Ci, g.H, g.W, n, tail) == (10, 10, 24, 6, 6, x.numel(), (16, 6, 6))
    B, g, n, tail = F._geometry(x.repeat(3, 1, 1, 1), w, dict(conv, dwin=(3, 5, 2, 1, 1)), 3, False)
    assert (B, g.B, n) == (6, 6, x.numel())
    for bad in ((0, 5, 1, 1, 1), (3, 0, 1, 1, 1), (3, 5, 0, 1, 1), (3, 5, 1, 0, 1), (3, 5, 1, 1, -1), (3, 7, 1, 1, 1), (3, 5, 1, 1), (3, 5, 1, 3, 0), (3.5, 5, 1, 1, 1)):
        with pytest.raises(RuntimeError):
            F._geometry(x, w, dict(conv, dwin=bad), 1, True)
    with pytest.raises(RuntimeError, match="channels"):
        F._geometry(x, w, dict(conv, dwin=(2, 5, 1, 1, 1)), 1, True)       # 8 * 2 launch channels against a 24-channel kernel
    with pytest.raises(RuntimeError):
        F._geometry(x, w, dict(conv, dwin=(3, 5, 1, 1, 1), updil=(1, 1), pads=(0, 0, 0, 0)), 1, True)


@pytest.mark.parametrize("rid,cls,ctor,xshape", ROWS, ids=[r[0] for r in ROWS])
def test_x_eq_is_the_window_map_of_the_struct(rid, cls, ctor, xshape):
    """_x_eq's tensor, element by element, is the gather of the real one that the entry points' contract states: launch image
    b * Do + do, launch channel ci * kd + j, pixel (y, x) <- x[b][ci][do * sd - pd + j * dd][y][x], zero outside [0, D)."""
    layer = make_layer(cls, ctor)
    x = torch.arange(1, 1 + torch.Size(xshape).numel(), dtype=torch.float32).reshape(xshape)
    xe, conv_e, back_e = layer._x_eq(x)
    xn, conv, back_n = layer._x_native(x)
    kd, D, sd, dd, pd = conv["dwin"]
    assert {k: tuple(v) if isinstance(v, (tuple, list)) else v for k, v in conv_e.items()} == \
           {k: tuple(v) if isinstance(v, (tuple, list)) else v for k, v in conv.items() if k != "dwin"}
    B, Ci, _, H, W = xshape
    Do = (D + 2 * pd - dd * (kd - 1) - 1) // sd + 1
    assert D == xshape[2] and tuple(xn.shape) == (B, Ci * D, H, W) and xn.data_ptr() == x.data_ptr()      # a view: no copy
    assert tuple(xe.shape) == (B * Do, Ci * kd, H, W)
    virt = torch.zeros_like(xe)
    for b in range(B):
        for do in range(Do):
            for ci in range(Ci):
                for j in range(kd):
                    z = do * sd - pd + j * dd
                    if 0 <= z < D:
                        virt[b * Do + do, ci * kd + j] = x[b, ci, z]
    assert torch.equal(virt, xe)
    o = torch.arange(float(B * Do * 2 * 3 * 3)).reshape(B * Do, 2, 3, 3)
    assert torch.equal(back_e(o), back_n(o)) and tuple(back_n(o).shape) == (B, 2, Do, 3, 3)      # the output permute stays
