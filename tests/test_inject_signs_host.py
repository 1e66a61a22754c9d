"""Host-only checks of the packed-sign path (no GPU): ``bt_pack_signs`` is declared, listed and exported, refuses null / zero
arguments, and the flag rules of a BT_DRAWS_SIGNS_PACKED launch hold on dummy pointers -- every one of them is decided on the host
before anything is launched, so the pointers below are never dereferenced."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2


def test_pack_signs_is_declared_and_exported():
    from bayesian_torch_amd import _lib
    assert "bt_pack_signs" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    assert "int bt_pack_signs(" in hdr and "#define BT_DRAWS_SIGNS_PACKED 2u" in hdr and "#define BT_DRAWS_EPS_PACKED 1u" in hdr
    assert "read as +1" in hdr      # the zero-sign rule is part of the contract
    assert _lib.DRAWS_SIGNS_PACKED == 2 and _lib.DRAWS_EPS_PACKED == 1
    assert [_lib.signs_packed_stride(n) for n in (1, 15, 16, 17, 4097)] == [16, 16, 16, 32, 4112]
    L = _lib.lib()
    assert L.bt_version() == 302
    assert ctypes.sizeof(_lib.bt_rng) == 32 and ctypes.sizeof(_lib.bt_draws) == 64      # no struct changed size


def test_pack_signs_refuses_null_and_zero_arguments():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    p = 0x1000
    assert L.bt_pack_signs(None, 1, 1, p, p, None) == BAD_ARG and b"bt_pack_signs" in L.bt_last_error_string()
    assert L.bt_pack_signs(p, 1, 1, None, p, None) == BAD_ARG
    assert L.bt_pack_signs(p, 1, 1, p, None, None) == BAD_ARG
    assert L.bt_pack_signs(p, 0, 1, p, p, None) == BAD_ARG
    assert L.bt_pack_signs(p, 1, 0, p, p, None) == BAD_ARG
    assert L.bt_pack_signs(p, 1, 1, p + 4, p, None) == BAD_ARG and b"aligned" in L.bt_last_error_string()


def test_signs_flag_rules_on_the_host():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    p = 0x1000      # any non-null, 16-byte aligned address
    geom = _lib.bt_conv2d_geom(4, 8, 6, 6, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    out = ctypes.c_void_p(p)
    EPS, SIGNS = _lib.DRAWS_EPS_PACKED, _lib.DRAWS_SIGNS_PACKED

    def call(fn, params, draws, linear=False):
        tail = (p, 0, ctypes.byref(params), ctypes.byref(draws), None, out, None, None, 0, None)
        return fn(4, 8, 8, 1, *tail) if linear else fn(ctypes.byref(geom), 1, *tail)

    def rng(flags):
        return _lib.bt_rng(1, None, 0, 1, 0, flags)

    def err():
        return L.bt_last_error_string()

    packed = _lib.bt_params(p, p, None, None, None, None, None, None, p, p, 0, 0)
    biased = _lib.bt_params(p, p, p, p, None, None, None, None, p, p, 0, 0)
    bare = _lib.bt_params(p, p, None, None, None, None, None, None, None, None, 0, 0)
    whole = lambda flags: _lib.bt_draws(p, None, p, p, rng(flags))
    flip = (L.bt_flipout_conv2d_fwd, False), (L.bt_flipout_linear_fwd, True)
    for fn, lin in flip:
        # a bit above 3
        assert call(fn, packed, whole(4 | EPS | SIGNS), lin) == BAD_ARG and b"unknown bt_rng.flags bit" in err()
        assert call(fn, packed, whole(8), lin) == BAD_ARG and b"unknown bt_rng.flags bit" in err()
        # the sign flag without the draw flag
        assert call(fn, packed, whole(SIGNS), lin) == BAD_ARG and b"flags" in err()
        # the draw flag alone on a Flipout entry: still refused as unsupported, by name
        assert call(fn, packed, whole(EPS), lin) == UNSUPPORTED and b"BT_DRAWS_EPS_PACKED" in err()
        # both flags: what the path needs
        assert call(fn, packed, _lib.bt_draws(None, None, p, p, rng(EPS | SIGNS)), lin) == BAD_ARG and b"eps_w" in err()
        assert call(fn, packed, _lib.bt_draws(p, None, None, p, rng(EPS | SIGNS)), lin) == BAD_ARG and b"sign_in" in err()
        assert call(fn, packed, _lib.bt_draws(p, None, p, None, rng(EPS | SIGNS)), lin) == BAD_ARG and b"sign_in" in err()
        assert call(fn, bare, whole(EPS | SIGNS), lin) == BAD_ARG and b"mu_packed" in err()
        assert call(fn, packed, _lib.bt_draws(p + 4, None, p, p, rng(EPS | SIGNS)), lin) == BAD_ARG and b"aligned" in err()
        assert call(fn, packed, _lib.bt_draws(p, None, p + 4, p, rng(EPS | SIGNS)), lin) == BAD_ARG and b"aligned" in err()
        assert call(fn, packed, _lib.bt_draws(p, None, p, p + 8, rng(EPS | SIGNS)), lin) == BAD_ARG and b"aligned" in err()
        # eps_b exactly when the layer has a bias
        assert call(fn, packed, _lib.bt_draws(p, p, p, p, rng(EPS | SIGNS)), lin) == BAD_ARG and b"eps_b" in err()
        assert call(fn, biased, whole(EPS | SIGNS), lin) == BAD_ARG and b"inject all draws" in err()
    # on a Reparameterization entry: refused, and the message names the flags
    for fn, lin in ((L.bt_reparam_conv2d_fwd, False), (L.bt_reparam_linear_fwd, True)):
        assert call(fn, packed, _lib.bt_draws(p, None, None, None, rng(EPS | SIGNS)), lin) == BAD_ARG and b"flags" in err()
        assert call(fn, packed, _lib.bt_draws(p, None, None, None, rng(SIGNS)), lin) == BAD_ARG and b"flags" in err()
    # a forced f32 / bf16x2 contraction: unsupported before any launch
    try:
        for mode in (1, 2):
            assert L.bt_set_contraction(mode) == 0
            for fn, lin in flip:
                assert call(fn, packed, whole(EPS | SIGNS), lin) == UNSUPPORTED and b"contraction" in err()
    finally:
        L.bt_set_contraction(0)
