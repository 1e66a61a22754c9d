"""Host-only checks of the contraction knob (no GPU): ``bt_set_contraction`` accepts mode 3 (bf16) and nothing past it,
``bt_get_contraction`` reports what is in force, ``bayesian_torch_amd.precision`` names the modes and restores them, the environment
selects the mode of a fresh process, and a packed-draw launch in mode 3 is refused on the host before anything is launched (the
pointers below are never dereferenced)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2


@pytest.fixture(autouse=True)
def _automatic_mode_afterwards():
    yield
    from bayesian_torch_amd import _lib
    _lib.lib().bt_set_contraction(0)


def test_mode_3_is_accepted_and_nothing_past_it():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.bt_set_contraction(3) == 0
    assert L.bt_set_contraction(4) == BAD_ARG and b"bt_set_contraction" in L.bt_last_error_string()
    assert L.bt_set_contraction(-1) == BAD_ARG
    assert L.bt_get_contraction() == 3      # a refused call changes nothing


def test_getter_round_trips():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    for mode in (0, 1, 2, 3, 0):
        assert L.bt_set_contraction(mode) == 0 and L.bt_get_contraction() == mode


def test_header_and_binding_list_the_same_symbols():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*\*?(bt_[a-z0-9_]+)\(", hdr, flags=re.M))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert "bt_get_contraction" in declared and "int bt_get_contraction(void);" in hdr
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "bt_get_contraction")
    assert _lib.lib().bt_version() == 302
    assert ctypes.sizeof(_lib.bt_rng) == 32 and ctypes.sizeof(_lib.bt_draws) == 64 and ctypes.sizeof(_lib.bt_params) == 88      # no struct changed size


def test_python_names_round_trip():
    import bayesian_torch_amd as bta
    from bayesian_torch_amd import _lib, precision
    assert bta.precision is precision and bta.contraction is precision.contraction
    assert bta.set_contraction is precision.set_contraction and bta.get_contraction is precision.get_contraction
    assert precision.NAMES == ("auto", "f32", "bf16x2", "bf16")
    for mode, name in enumerate(precision.NAMES):
        precision.set_contraction(name)
        assert precision.get_contraction() == name and _lib.lib().bt_get_contraction() == mode
    for bad in ("bf16x3", "BF16", "", None, 3):
        with pytest.raises(ValueError):
            precision.set_contraction(bad)
        with pytest.raises(ValueError):
            with precision.contraction(bad):
                pass
    assert precision.get_contraction() == "bf16"      # a refused name changes nothing


def test_context_manager_restores_the_previous_mode():
    from bayesian_torch_amd import precision
    precision.set_contraction("f32")
    with precision.contraction("bf16"):
        assert precision.get_contraction() == "bf16"
        with precision.contraction("auto"):
            assert precision.get_contraction() == "auto"
        assert precision.get_contraction() == "bf16"
    assert precision.get_contraction() == "f32"

    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with precision.contraction("bf16"):
            assert precision.get_contraction() == "bf16"
            raise Boom()
    assert precision.get_contraction() == "f32"


def _py(code, **env):
    e = {k: v for k, v in os.environ.items() if k != "BT_CONTRACTION"}
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)


def test_environment_selects_the_mode_of_a_fresh_process():
    show = "from bayesian_torch_amd import precision; print(precision.get_contraction())"
    r = _py(show, BT_CONTRACTION="bf16")
    assert r.returncode == 0 and r.stdout.strip() == "bf16", r.stderr
    r = _py(show, BT_CONTRACTION="bf16x2")
    assert r.returncode == 0 and r.stdout.strip() == "bf16x2", r.stderr


def test_packed_draws_in_mode_3_are_refused_before_any_launch():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    p = 0x1000      # any non-null, 16-byte aligned address
    geom = _lib.bt_conv2d_geom(4, 8, 6, 6, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    out = ctypes.c_void_p(p)
    EPS, SIGNS = _lib.DRAWS_EPS_PACKED, _lib.DRAWS_SIGNS_PACKED

    def call(fn, params, draws, linear=False):
        tail = (p, 0, ctypes.byref(params), ctypes.byref(draws), None, out, None, None, 0, None)
        return fn(4, 8, 8, 1, *tail) if linear else fn(ctypes.byref(geom), 1, *tail)

    packed = _lib.bt_params(p, p, None, None, None, None, None, None, p, p, 0, 0)
    assert L.bt_set_contraction(3) == 0
    for fn, lin in ((L.bt_reparam_conv2d_fwd, False), (L.bt_reparam_linear_fwd, True)):
        d = _lib.bt_draws(p, None, None, None, _lib.bt_rng(1, None, 0, 1, 0, EPS))
        assert call(fn, packed, d, lin) == UNSUPPORTED
        assert b"contraction" in L.bt_last_error_string() and b"bf16" in L.bt_last_error_string()
    for fn, lin in ((L.bt_flipout_conv2d_fwd, False), (L.bt_flipout_linear_fwd, True)):
        d = _lib.bt_draws(p, None, p, p, _lib.bt_rng(1, None, 0, 1, 0, EPS | SIGNS))
        assert call(fn, packed, d, lin) == UNSUPPORTED and b"contraction" in L.bt_last_error_string()
