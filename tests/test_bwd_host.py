"""CPU: what the training backward's host side refuses, and the small entry points under plan-only mode.

The backward's entry points share the forward's geometry check (``geom_error`` in ``csrc/bt_api_internal.h``) through the one plan of
``csrc/bt_bwd_plan.h``. Before that, ``bt_conv2d_bwd_workspace`` and ``bt_conv2d_bwd`` divided by a stride, a kernel size or a channel
count they had not looked at and the process died of SIGFPE -- so every probe here runs in a child Python process that loads the
library with ctypes alone (no torch, no GPU): a regression is a failed assert, not a dead pytest. The launch-parity fixture
(``test_bwd_launch_parity.py``) cannot hold these cases: the commit it was recorded from does not survive them.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("B", "Ci", "H", "W", "Co", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "groups")
GOOD = dict(B=2, Ci=4, H=6, W=6, Co=8, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, groups=2)

# The child: bt_conv2d_bwd_workspace, then bt_conv2d_bwd_kl on made-up (never dereferenced) pointers with plan-only on, so that a
# call that is NOT refused still launches nothing.  Prints one JSON object.
GEOM_PROBE = r"""
import ctypes as C, json, sys
L = C.CDLL(sys.argv[1])
case = json.loads(sys.argv[2])
vp = C.c_void_p
class Geom(C.Structure):
    _fields_ = [(n, C.c_int32) for n in case["fields"]]
class Rng(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("call_base_dev", vp), ("call", C.c_uint32), ("layer_id", C.c_uint32), ("sample0", C.c_uint32), ("flags", C.c_uint32)]
class Params(C.Structure):
    _fields_ = [(n, vp) for n in ("mu_w", "rho_w", "mu_b", "rho_b", "prior_mu_w", "prior_sigma_w", "prior_mu_b", "prior_sigma_b", "mu_packed", "sigma_packed")] \
        + [("prior_kind", C.c_int32), ("reserved", C.c_int32)]
class Draws(C.Structure):
    _fields_ = [("eps_w", vp), ("eps_b", vp), ("sign_in", vp), ("sign_out", vp), ("rng", Rng)]
L.bt_conv2d_bwd_workspace.restype = C.c_size_t
L.bt_conv2d_bwd_workspace.argtypes = [C.POINTER(Geom), C.c_int32]
L.bt_conv2d_bwd_kl.argtypes = [C.POINTER(Geom), C.c_int32, C.c_int32, vp, C.c_int64, vp, C.POINTER(Params), C.POINTER(Draws), vp, vp, vp, vp, vp, C.c_size_t, vp]
L.bt_last_error_string.restype = C.c_char_p
L.bt_debug_plan_only(1)
g = Geom(*case["geom"])
p, d = Params(), Draws()
A = lambda i: 0x10000000 + (i << 24)
p.mu_w, p.rho_w, p.prior_mu_w, p.prior_sigma_w, p.mu_packed, p.sigma_packed = A(1), A(2), A(3), A(4), A(5), A(6)
ws = L.bt_conv2d_bwd_workspace(C.byref(g), case["S"])
rc = L.bt_conv2d_bwd_kl(C.byref(g), case["S"], 0, A(7), case["stride"], A(8), C.byref(p), C.byref(d), A(9), A(10), A(11), A(12), A(13), 1 << 40, None)
print(json.dumps(dict(ws=ws, rc=rc, err=L.bt_last_error_string().decode())))
"""


def lib_path():
    return os.environ.get("BT_LIB_PATH") or os.path.join(ROOT, "bayesian_torch_amd", "libbtorch_hip.so")


def run_child(script, arg):
    r = subprocess.run([sys.executable, "-c", script, lib_path(), json.dumps(arg)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"the probe died with exit status {r.returncode}: {r.stderr[-500:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


def geom_probe(S=1, stride=0, **change):
    g = dict(GOOD, **change)
    return run_child(GEOM_PROBE, dict(fields=FIELDS, geom=[g[f] for f in FIELDS], S=S, stride=stride))


BAD = [(f + "=0", {f: 0}, 1) for f in ("sh", "sw", "dh", "dw", "kh", "kw", "H", "W", "Ci", "Co", "B")] + [
    ("ph=-1", dict(ph=-1), 1), ("pw=-1", dict(pw=-1), 1), ("groups=0", dict(groups=0), 1), ("groups not dividing Ci", dict(groups=3, Co=9), 1),
    ("groups not dividing Co", dict(Co=9), 1), ("S=0", {}, 0), ("S=-1", {}, -1)]


@pytest.mark.parametrize("change,S", [b[1:] for b in BAD], ids=[b[0] for b in BAD])
def test_bad_geometry_is_refused_not_divided_by(change, S):
    r = geom_probe(S=S, **change)
    assert r == dict(ws=0, rc=-1, err="bt_conv2d_bwd: bad geometry")      # BT_ERR_BAD_ARG


@pytest.mark.parametrize("change", [dict(H=1, W=1, ph=0, pw=0), dict(H=5, W=2, ph=0, pw=0), dict(H=2, W=5, ph=0, pw=0, dh=2, dw=1)],
                         ids=["1x1 k3 p0", "5x2 k3 p0", "2x5 k3 p0 dilated"])
def test_an_empty_output_is_refused(change):
    """H = 1, k = 3, p = 0: the query used to return a size computed from a negative M."""
    r = geom_probe(**change)
    assert r == dict(ws=0, rc=-1, err="bt_conv2d_bwd: empty output")


def test_a_negative_x_sample_stride_is_refused_and_the_good_geometry_is_not():
    good = geom_probe(stride=GOOD["B"] * GOOD["Ci"] * GOOD["H"] * GOOD["W"])
    assert good["rc"] == 0 and good["ws"] > 0
    assert geom_probe(stride=0) == good      # x shared by the samples
    r = geom_probe(stride=-1)
    assert (r["rc"], r["err"], r["ws"]) == (-1, "bt_conv2d_bwd: bad geometry", good["ws"])


# ---------------------------------------------------------------------------------------------- the small entry points, plan-only
# One child (it imports the package's ctypes prototypes): every entry point below launches through launch_kernel, so with plan-only on
# it returns BT_OK on a machine without a device and leaves its launch count and last grid.  -> {name: [rc, launches, grid x, y, z, block x]}
SMALL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, json.loads(sys.argv[2]))
from bayesian_torch_amd import _lib
L = _lib.lib()
h = C.CDLL(_lib.LIB_PATH)
h.bt_debug_last_launch_record.argtypes = [C.POINTER(C.c_int64), C.c_int]
rec = (C.c_int64 * 11)()
A = lambda i: 0x10000000 + (i << 24)
rng = _lib.bt_rng(seed=5, call=1, layer_id=2, sample0=0)
out = {}
def run(name, fn, *args):
    h.bt_debug_last_launch_record(rec, 11)
    rc = getattr(L, fn)(*args)
    h.bt_debug_last_launch_record(rec, 11)
    out[name] = [rc, rec[9], rec[0], rec[1], rec[2], rec[3]]
h.bt_debug_plan_only(1)
run("kl_normal_bwd", "bt_kl_normal_bwd", A(1), A(2), A(3), A(4), A(5), 70001, 0, A(6), A(7), None)
run("kl_normal_bwd big", "bt_kl_normal_bwd", A(1), A(2), A(3), A(4), A(5), 4096 * 256 + 1, 0, A(6), A(7), None)
run("pack_signs", "bt_pack_signs", A(1), 3, 1001, A(2), A(3), None)
run("rng_normal_fill", "bt_rng_normal_fill", C.byref(rng), 0, 3, 20, 6, 9, A(1), None)
run("rng_sign_fill", "bt_rng_sign_fill", C.byref(rng), 2, 3, 1000, A(1), None)
for Cc in (10, 64, 65):
    run("mc_epilogue C%d" % Cc, "bt_mc_epilogue", 4, 9, Cc, A(1), A(2), None)
run("maxpool", "bt_maxpool_3x3s2", A(1), A(2), 6, 9, 10, None)
run("pack_params", "bt_pack_params", A(1), A(2), 20, 6, 9, A(3), A(4), None)
run("lowrank_mean", "bt_lowrank_mean", A(1), A(2), 1000, 3, 17, None, C.byref(rng), A(3), None)
for r in (3, 40):
    run("kl_lowrank r%d" % r, "bt_kl_lowrank", A(1), A(2), 1000, r, 0.5, A(3), A(4), A(5), A(6), A(7), L.bt_kl_lowrank_workspace(1000, r), None)
for Cc in (10, 64, 65):
    wsb = L.bt_avu_workspace_bytes(4, 9, Cc, 21)
    run("avu_fwd C%d" % Cc, "bt_avu_fwd", 4, 9, Cc, A(1), A(2), 0, 21, None, 1.0, A(3), A(4), A(5), A(6), A(7), A(8), A(9), wsb, None)
    run("avu_bwd C%d" % Cc, "bt_avu_bwd", 4, 9, Cc, A(1), 0, 21, A(2), A(3), A(4), wsb, A(5), None)
h.bt_debug_plan_only(0)
print(json.dumps(out))
"""


def test_small_entry_points_plan_without_a_device():
    got = run_child(SMALL_PROBE, ROOT)
    cdiv = lambda a, b: (a + b - 1) // b
    rows = lambda B, C: cdiv(B, 4) if C <= 64 else B      # one wave per row up to 64 classes, else one workgroup per row
    want = {
        "kl_normal_bwd": [0, 1, cdiv(70001, 256), 1, 1, 256],
        "kl_normal_bwd big": [0, 1, 4096, 1, 1, 256],
        "pack_signs": [0, 1, cdiv(3 * (cdiv(1001, 16) * 16 // 4), 256), 1, 1, 256],
        "rng_normal_fill": [0, 1, cdiv(20 * 9 * 2, 256), 3, 1, 256],
        "rng_sign_fill": [0, 1, cdiv(1000, 256), 3, 1, 256],
        "maxpool": [0, 1, cdiv(6 * 5 * 3, 256), 1, 1, 256],          # 9 x 10 -> 5 x 5 outputs, two per thread: 3 per row
        "pack_params": [0, 1, cdiv(20 * 9 * 8, 256), 1, 1, 256],
        "lowrank_mean": [0, 1, cdiv(1000, 64), cdiv(17, 8), 1, 64],
    }
    for C in (10, 64, 65):
        want["mc_epilogue C%d" % C] = [0, 1, rows(9, C), 1, 1, 256]
        want["avu_fwd C%d" % C] = [0, 2, 1, 1, 1, 1024]              # rows, then the one finishing workgroup (the record's last launch)
        want["avu_bwd C%d" % C] = [0, 1, rows(9, C), 1, 1, 256]
    for r in (3, 40):
        want["kl_lowrank r%d" % r] = [0, 2, 1, 1, 1, 1024]           # sweep, then the one finishing workgroup
    assert got == want
