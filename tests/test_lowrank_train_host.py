"""CPU: the host side of the low-rank multivariate layer's fused training path -- the path decision under both values of
``set_lowrank_train_path``, the switch itself, the new C-ABI symbols (declared, bound, exported, refusing bad arguments on the host), their
plan-only launch records (a child process, as tests/test_bwd_host.py), and the closed-form KL gradient the GPU tests compare against,
held here to autograd of tests/_lowrank_ref.py on every golden."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import _lowrank_ref as R
import _lowrank_train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"bt_lowrank_conv2d_bwd_workspace", "bt_lowrank_conv2d_bwd", "bt_lowrank_conv2d_bwd_info", "bt_lowrank_wgrad_finish", "bt_kl_lowrank_bwd_workspace",
       "bt_kl_lowrank_bwd"}

# tests/test_lowrank_host.py::test_path_decision's table: (rank, d_uniform, prior_diag, needs_grad, (path, kl_path))
TABLE = [
    (1, True, True, False, ("in_kernel", "kernel")), (4, True, True, False, ("in_kernel", "kernel")),
    (5, True, True, False, ("mean_prepass", "kernel")), (432, True, True, False, ("mean_prepass", "kernel")),
    (3, True, False, False, ("in_kernel", "materialised")), (7, True, False, False, ("mean_prepass", "materialised")),
    (2, False, True, False, ("materialised", "materialised")), (2, True, True, True, ("materialised", "materialised")),
    (9, False, False, True, ("materialised", "materialised")),
]


@pytest.mark.parametrize("rank,d_uniform,prior_diag,needs_grad,want", TABLE)
def test_path_decision_under_both_switch_values(rank, d_uniform, prior_diag, needs_grad, want):
    from bayesian_torch_amd.layers._lowrank import choose_path
    today = choose_path(rank, d_uniform, prior_diag, needs_grad)
    assert today[:2] == want
    assert choose_path(rank, d_uniform, prior_diag, needs_grad, train_path="materialised") == today      # the default changes nothing
    fused = choose_path(rank, d_uniform, prior_diag, needs_grad, train_path="fused")
    if not needs_grad:
        assert fused == today
    elif not d_uniform:
        assert fused == ("materialised", "materialised", "D_param is not one constant")
    else:
        assert fused == choose_path(rank, d_uniform, prior_diag, False)      # a call that needs gradients keeps its inference paths


def test_fused_path_decision_by_rank_and_prior():
    from bayesian_torch_amd.layers._lowrank import choose_path
    f = lambda *a: choose_path(*a, train_path="fused")
    assert f(1, True, True, True) == f(4, True, True, True) == ("in_kernel", "kernel", None)
    assert f(5, True, True, True) == f(432, True, True, True) == ("mean_prepass", "kernel", None)
    assert f(3, True, False, True) == ("in_kernel", "materialised", "prior_cov_L is not zero")      # the differentiable torch KL
    assert f(7, False, True, True) == ("materialised", "materialised", "D_param is not one constant")


def test_the_switch_refuses_unknown_names_and_reads_the_environment():
    import bayesian_torch_amd.layers as BL
    from bayesian_torch_amd.layers import _lowrank
    assert BL.set_lowrank_train_path is _lowrank.set_lowrank_train_path and BL.get_lowrank_train_path is _lowrank.get_lowrank_train_path
    assert BL.get_lowrank_train_path() == os.environ.get("BT_LOWRANK_TRAIN_PATH", "materialised")
    prev = BL.set_lowrank_train_path("fused")
    try:
        assert BL.get_lowrank_train_path() == "fused" and BL.set_lowrank_train_path("materialised") == "fused"
        with pytest.raises(ValueError, match=r"set_lowrank_train_path: expected one of \('fused', 'materialised'\), got 'native'"):
            BL.set_lowrank_train_path("native")
        assert BL.get_lowrank_train_path() == "materialised"      # a refused name changes nothing
    finally:
        BL.set_lowrank_train_path(prev)
    code = "import bayesian_torch_amd.layers as L; print(L.get_lowrank_train_path())"
    env = {k: v for k, v in os.environ.items() if k != "BT_LOWRANK_TRAIN_PATH"}
    for value, want in ((None, "materialised"), ("fused", "fused"), ("materialised", "materialised")):
        e = dict(env) if value is None else dict(env, BT_LOWRANK_TRAIN_PATH=value)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, r.stderr[-400:]
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, BT_LOWRANK_TRAIN_PATH="native"), capture_output=True, text=True)
    assert r.returncode != 0 and "BT_LOWRANK_TRAIN_PATH" in r.stderr


def test_new_symbols_are_declared_bound_exported_and_refuse_on_the_host():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*\*?(bt_[a-z0-9_]+)\(", hdr, flags=re.M))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(NEW):
        assert hasattr(handle, name), name
    L = _lib.lib()
    assert L.bt_version() == 302 and re.search(r"#define BT_VERSION (\d+)", hdr).group(1) == "302"
    one = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch
    rngc = _lib.bt_rng(0, None, 0, 1, 0, 0)
    good = (2, 4, 6, 6, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    err = lambda: L.bt_last_error_string()

    def bwd(geom=good, S=1, x=one, stride=0, g=one, mean=one, mstride=0, Lp=one, R_=3, sd=1e-5, z=None, rng=rngc, eps=None, dx=one, dw=one, ws=one, nbytes=1 << 30):
        gm = _lib.bt_conv2d_geom(*geom)
        return L.bt_lowrank_conv2d_bwd(ctypes.byref(gm), S, x, stride, g, mean, mstride, Lp, R_, sd, z, None if rng is None else ctypes.byref(rng), eps, dx, dw, ws,
                                       nbytes, None)

    bad = [dict(x=None), dict(g=None), dict(mean=None), dict(dx=None, dw=None), dict(S=0), dict(stride=-1), dict(mstride=-1), dict(R_=5), dict(R_=-1),
           dict(R_=2, Lp=None), dict(sd=0.0), dict(sd=-1.0), dict(sd=float("inf")), dict(sd=float("nan")), dict(rng=None), dict(eps=one), dict(z=one),
           dict(geom=good[:13] + (2,)), dict(geom=(2, 4, 6, 6, 8, 3, 3, 0, 1, 1, 1, 1, 1, 1)), dict(geom=(2, 4, 1, 1, 8, 3, 3, 1, 1, 0, 0, 1, 1, 1))]
    for kw in bad:
        assert bwd(**kw) == -1 and b"bt_lowrank_conv2d_bwd" in err(), (kw, err())
    assert L.bt_lowrank_conv2d_bwd(None, 1, one, 0, one, one, 0, one, 3, 1e-5, None, ctypes.byref(rngc), None, one, one, one, 16, None) == -1 and b"bt_lowrank_conv2d_bwd" in err()
    assert bwd(geom=(1, 1 << 16, 1 << 8, 1 << 8, 8, 1, 1, 1, 1, 0, 0, 1, 1, 1)) == -2 and b"bt_lowrank_conv2d_bwd" in err()      # 2^32 input elements: bwd_plan's limit
    gm = _lib.bt_conv2d_geom(*good)
    wsz = lambda geom, S, r: L.bt_lowrank_conv2d_bwd_workspace(ctypes.byref(_lib.bt_conv2d_geom(*geom)), S, r)
    assert wsz(good, 1, 3) >= 16 and wsz(good, 2, 5) == wsz(good, 2, 0) + 4 * 2 * 8 * 4 * 9      # the pre-pass slab of a rank above the bound
    assert wsz(good, 1, -1) == 0 and wsz(good, 1, 4097) == 0 and wsz(good, 0, 3) == 0 and wsz(good[:13] + (2,), 1, 3) == 0
    assert L.bt_lowrank_conv2d_bwd_workspace(None, 1, 3) == 0
    assert L.bt_lowrank_conv2d_bwd_info(None, 10) == -1 and b"bt_lowrank_conv2d_bwd_info" in err()

    fin = lambda dw=one, n=10, r=3, S=1, z=None, rng=rngc, dmu=one, dL=one: L.bt_lowrank_wgrad_finish(dw, n, r, S, z, None if rng is None else ctypes.byref(rng), dmu, dL, None)
    for kw in (dict(dw=None), dict(n=0), dict(r=0), dict(S=0), dict(dmu=None, dL=None), dict(rng=None)):
        assert fin(**kw) == -1 and b"bt_lowrank_wgrad_finish" in err(), kw
    assert fin(r=4097) == -2 and b"bt_lowrank_wgrad_finish" in err()

    klb = lambda mu=one, Lp=one, n=10, r=2, d=1e-10, pm=one, pv=one, g=one, dmu=one, dL=one, ws=one, nbytes=1 << 30: L.bt_kl_lowrank_bwd(mu, Lp, n, r, d, pm, pv, g, dmu, dL, None, ws,
                                                                                                                                         nbytes, None)
    for kw in (dict(mu=None), dict(Lp=None), dict(pm=None), dict(pv=None), dict(g=None), dict(dmu=None, dL=None), dict(n=0), dict(r=0), dict(d=0.0), dict(d=-1.0)):
        assert klb(**kw) == -1 and b"bt_kl_lowrank_bwd" in err(), kw
    assert klb(r=4097) == -2 and b"bt_kl_lowrank_bwd" in err()
    assert klb(ws=None, nbytes=0) == -3 and klb(nbytes=8) == -3 and klb(ws=ctypes.c_void_p(260)) == -3 and b"bt_kl_lowrank_bwd" in err()
    assert L.bt_kl_lowrank_bwd_workspace(10, 4097) == 0 and L.bt_kl_lowrank_bwd_workspace(10, 0) == 0 and L.bt_kl_lowrank_bwd_workspace(0, 3) == 0
    assert L.bt_kl_lowrank_bwd_workspace(432, 432) >= L.bt_kl_lowrank_workspace(432, 432) + 8 * 2 * 432 * 432


# One child: every new entry point under plan-only mode on made-up (never dereferenced) pointers.
#   -> {name: [rc, launches, last grid x, y, z, block x]} and the backward's own records.
PLAN_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, json.loads(sys.argv[2]))
from bayesian_torch_amd import _lib
L = _lib.lib()
h = C.CDLL(_lib.LIB_PATH)
h.bt_debug_last_launch_record.argtypes = [C.POINTER(C.c_int64), C.c_int]
rec = (C.c_int64 * 11)()
A = lambda i: 0x10000000 + (i << 24)
rng = _lib.bt_rng(seed=5, call=1, layer_id=2, sample0=0)
out, info = {}, {}
def run(name, fn, *args):
    h.bt_debug_last_launch_record(rec, 11)
    rc = getattr(L, fn)(*args)
    h.bt_debug_last_launch_record(rec, 11)
    out[name] = [rc, rec[9], rec[0], rec[1], rec[2], rec[3]]
h.bt_debug_plan_only(1)
small = _lib.bt_conv2d_geom(2, 5, 8, 8, 6, 3, 3, 2, 2, 1, 1, 1, 1, 1)
n = 6 * 5 * 9
run("bwd R3", "bt_lowrank_conv2d_bwd", C.byref(small), 1, A(1), 0, A(2), A(3), 0, A(4), 3, 1e-5, None, C.byref(rng), None, A(5), A(6), A(7), 1 << 30, None)
info["bwd R3"] = _lib.lowrank_bwd_info()
run("bwd R3 dx only", "bt_lowrank_conv2d_bwd", C.byref(small), 1, A(1), 0, A(2), A(3), 0, A(4), 3, 1e-5, None, C.byref(rng), None, A(5), None, A(7), 1 << 30, None)
info["bwd R3 dx only"] = _lib.lowrank_bwd_info()
run("bwd R3 dW only", "bt_lowrank_conv2d_bwd", C.byref(small), 1, A(1), 0, A(2), None, 0, None, 0, 0.0, None, None, None, None, A(6), A(7), 1 << 30, None)
info["bwd R3 dW only"] = _lib.lowrank_bwd_info()
run("finish r3", "bt_lowrank_wgrad_finish", A(6), n, 3, 1, None, C.byref(rng), A(8), A(9), None)
run("prepass r7", "bt_lowrank_mean", A(3), A(4), n, 7, 2, None, C.byref(rng), A(10), None)
run("bwd R0 behind the pre-pass", "bt_lowrank_conv2d_bwd", C.byref(small), 2, A(1), 0, A(2), A(10), n, None, 0, 1e-5, None, C.byref(rng), None, A(5), A(6), A(7), 1 << 30, None)
info["bwd R0 behind the pre-pass"] = _lib.lowrank_bwd_info()
run("finish r7", "bt_lowrank_wgrad_finish", A(6), n, 7, 2, None, C.byref(rng), A(8), A(9), None)
wide = _lib.bt_conv2d_geom(3, 68, 10, 10, 70, 3, 3, 1, 1, 1, 1, 1, 1, 1)
need = L.bt_lowrank_conv2d_bwd_workspace(C.byref(wide), 2, 2)
run("bwd wide", "bt_lowrank_conv2d_bwd", C.byref(wide), 2, A(1), 0, A(2), A(3), 0, A(4), 2, 1e-5, None, C.byref(rng), None, A(5), A(6), A(7), need, None)
info["bwd wide"] = _lib.lowrank_bwd_info()
info["wide workspace"] = need
run("bwd wide, short workspace", "bt_lowrank_conv2d_bwd", C.byref(wide), 2, A(1), 0, A(2), A(3), 0, A(4), 2, 1e-5, None, C.byref(rng), None, A(5), A(6), A(7), need - 32, None)
for r in (3, 40):
    run("kl bwd r%d" % r, "bt_kl_lowrank_bwd", A(1), A(2), 1000, r, 1e-10, A(3), A(4), A(5), A(6), A(7), None, A(8), L.bt_kl_lowrank_bwd_workspace(1000, r), None)
    run("kl fwd r%d" % r, "bt_kl_lowrank", A(1), A(2), 1000, r, 1e-10, A(3), A(4), A(5), None, A(8), L.bt_kl_lowrank_workspace(1000, r), None)
h.bt_debug_plan_only(0)
print(json.dumps(dict(out=out, info=info)))
"""


def test_plan_only_records_of_the_new_entry_points():
    from bayesian_torch_amd import _lib
    r = subprocess.run([sys.executable, "-c", PLAN_PROBE, _lib.LIB_PATH, json.dumps(ROOT)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"the probe died with exit status {r.returncode}: {r.stderr[-800:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    cdiv = lambda a, b: (a + b - 1) // b
    n = 6 * 5 * 9
    # small: B 2, 5 -> 6 channels, 8 x 8, k 3, stride 2, pad 1 -> 4 x 4: M = 32 (one chunk), 6 output channels (one piece);
    # wgrad's tile axis is T * Ci4 = 72 -> 2 tiles, dgrad's is B * H * W = 128 -> 2 tiles
    # wide (the GPU suite's tile-crossing shape): M = 300 -> by bwd_plan 3 chunks of 112; 70 output channels -> 3 pieces of 32
    want = {
        "bwd R3": [0, 2, 2, 1, 1, 256],                               # dgrad, wgrad (the record's last launch)
        "bwd R3 dx only": [0, 1, 2, 1, 1, 256],
        "bwd R3 dW only": [0, 1, 2, 1, 1, 256],
        "finish r3": [0, 1, cdiv(n * 4, 256), 1, 1, 256],
        "prepass r7": [0, 1, cdiv(n, 64), 1, 1, 64],
        "bwd R0 behind the pre-pass": [0, 2, 2, 1, 2, 256],           # one workgroup per (tile, sample)
        "finish r7": [0, 1, cdiv(n * 8, 256), 1, 1, 256],
        "bwd wide": [0, 4, cdiv(2 * 70 * 68 * 9, 256), 1, 1, 256],    # dgrad, its pieces summed, wgrad, its chunks summed
        "bwd wide, short workspace": [-3, 0, cdiv(2 * 70 * 68 * 9, 256), 1, 1, 256],
    }
    for rk in (3, 40):
        want["kl bwd r%d" % rk] = [0, 5, cdiv(1000 * rk, 256), 1, 1, 256]     # sweep, factor, factor inverse, inverse, gradient
        want["kl fwd r%d" % rk] = [0, 2, 1, 1, 1, 1024]                        # unchanged: sweep, finish
    assert got["out"] == want
    info = got["info"]
    assert info["bwd R3"] == dict(dgrad_launches=1, wgrad_launches=1, dgrad_pieces=1, wgrad_chunks=1, dgrid_x=2, dgrid_y=1, dgrid_z=1, wgrid_x=2, wgrid_y=1, wgrid_z=1)
    assert (info["bwd R3 dx only"]["dgrad_launches"], info["bwd R3 dx only"]["wgrad_launches"]) == (1, 0)
    assert (info["bwd R3 dW only"]["dgrad_launches"], info["bwd R3 dW only"]["wgrad_launches"]) == (0, 1)
    assert info["bwd R0 behind the pre-pass"] == dict(info["bwd R3"], dgrid_z=2, wgrid_z=2)
    assert info["bwd wide"] == dict(dgrad_launches=2, wgrad_launches=2, dgrad_pieces=3, wgrad_chunks=3, dgrid_x=5, dgrid_y=2, dgrid_z=6, wgrid_x=10, wgrid_y=2, wgrid_z=6)
    assert info["wide workspace"] == 4 * (2 * 3 * 70 * 68 * 9 + 3 * 2 * 3 * 68 * 100)      # wgrad's [S][3][n], dgrad's [3][S][x]


@pytest.mark.parametrize("tag", R.CASES)
def test_closed_form_kl_gradient_against_autograd(tag):
    """The GPU suite's reference for bt_kl_lowrank_bwd, held to fp64 autograd of _lowrank_ref.kl_diag: 1e-10 of the largest element on
    the full-rank case (cond ~ 7e5), 1e-15 on the others."""
    g = R.load(tag)
    mu, L = g["mu_kernel"].double().requires_grad_(True), g["L_param"].double().requires_grad_(True)
    R.kl_diag(mu, L, g["D_param"], g["prior_mean"], g["prior_cov_D"]).backward()
    dmu, dL = T.kl_grad_closed_form(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], g["prior_cov_D"])
    tol = 1e-10 if g["meta"]["ctor"]["rank"] > 100 else 1e-15
    for name, got, want in (("dmu", dmu, mu.grad), ("dL", dL, L.grad)):
        err, top = float((got - want).abs().max()), float(want.abs().max())
        print(f"{tag} {name}: max |closed form - autograd| {err:.3e}, max |autograd| {top:.3e} (rel {err / top:.2e})")
        assert err <= tol * top, (tag, name, err, top)
    c = 0.37
    dmu_c, dL_c = T.kl_grad_closed_form(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], g["prior_cov_D"], c)
    assert torch.allclose(dmu_c, c * dmu, rtol=1e-14, atol=0) and torch.allclose(dL_c, c * dL, rtol=1e-14, atol=0)
