"""Host-only checks of the packed-draw path (no GPU): the ``rng.set_inject_path`` option, the new symbol, and the argument
validation of a BT_DRAWS_EPS_PACKED launch, which runs on the host before anything is launched."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _py(code, **env):
    e = {k: v for k, v in os.environ.items() if k != "BT_INJECT_PATH"}
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)


def test_inject_path_option():
    from bayesian_torch_amd import rng
    before = rng.get_inject_path()
    try:
        rng.set_inject_path("split")
        assert rng.get_inject_path() == "split"
        rng.set_inject_path("general")
        assert rng.get_inject_path() == "general"
        with pytest.raises(ValueError, match="general"):
            rng.set_inject_path("fast")
        assert rng.get_inject_path() == "general"
    finally:
        rng.set_inject_path(before)


def test_inject_path_default_and_environment():
    show = "from bayesian_torch_amd import rng; print(rng.get_inject_path())"
    r = _py(show)
    assert r.returncode == 0 and r.stdout.strip() == "general", r.stderr
    r = _py(show, BT_INJECT_PATH="split")
    assert r.returncode == 0 and r.stdout.strip() == "split", r.stderr
    r = _py(show, BT_INJECT_PATH="bf16")
    assert r.returncode != 0 and "BT_INJECT_PATH" in r.stderr


def test_pack_eps_is_declared_and_exported():
    from bayesian_torch_amd import _lib
    assert "bt_pack_eps" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    assert "int bt_pack_eps(" in hdr and "#define BT_DRAWS_EPS_PACKED 1u" in hdr and "uint32_t flags;" in hdr
    assert _lib.DRAWS_EPS_PACKED == 1 and [f[0] for f in _lib.bt_rng._fields_][-1] == "flags"
    L = _lib.lib()
    assert L.bt_version() == 302
    assert L.bt_pack_eps(None, 1, 1, 1, 1, None, None) == -1 and b"bt_pack_eps" in L.bt_last_error_string()
    assert L.bt_pack_eps(0x1000, 0, 1, 1, 1, 0x1000, None) == -1
    assert L.bt_pack_eps(0x1000, 1, 4, 4, 129, 0x1000, None) == -2      # more taps than the fused kernels take


def test_flagged_launch_is_validated_on_the_host():
    """BT_DRAWS_EPS_PACKED with sign tensors / Flipout: BT_ERR_UNSUPPORTED; without the packed parameters: BT_ERR_BAD_ARG; an unknown
    flag bit: BT_ERR_BAD_ARG -- all before any launch (the pointers below are never dereferenced)."""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    p = 0x1000      # any non-null, 16-byte aligned address
    geom = _lib.bt_conv2d_geom(4, 8, 6, 6, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    out = ctypes.c_void_p(p)

    def call(fn, params, draws, linear=False):
        tail = (p, 0, ctypes.byref(params), ctypes.byref(draws), None, out, None, None, 0, None)
        return fn(4, 8, 8, 1, *tail) if linear else fn(ctypes.byref(geom), 1, *tail)

    packed = _lib.bt_params(p, p, None, None, None, None, None, None, p, p, 0, 0)
    bare = _lib.bt_params(p, p, None, None, None, None, None, None, None, None, 0, 0)
    flagged = _lib.bt_rng(1, None, 0, 1, 0, _lib.DRAWS_EPS_PACKED)
    # Flipout entry, sign tensors
    d = _lib.bt_draws(p, None, p, p, flagged)
    assert call(L.bt_flipout_conv2d_fwd, packed, d) == -2 and b"BT_DRAWS_EPS_PACKED" in L.bt_last_error_string()
    assert call(L.bt_flipout_linear_fwd, packed, d, linear=True) == -2
    # no packed parameters
    d = _lib.bt_draws(p, None, None, None, flagged)
    assert call(L.bt_reparam_conv2d_fwd, bare, d) == -1 and b"mu_packed" in L.bt_last_error_string()
    assert call(L.bt_reparam_linear_fwd, bare, d, linear=True) == -1
    # the flag without a draw, a misaligned draw, an unknown bit
    assert call(L.bt_reparam_conv2d_fwd, packed, _lib.bt_draws(None, None, None, None, flagged)) == -1
    assert call(L.bt_reparam_conv2d_fwd, packed, _lib.bt_draws(p + 4, None, None, None, flagged)) == -1
    assert call(L.bt_reparam_conv2d_fwd, packed, _lib.bt_draws(p, None, None, None, _lib.bt_rng(1, None, 0, 1, 0, 2))) == -1
    assert b"flags" in L.bt_last_error_string()
