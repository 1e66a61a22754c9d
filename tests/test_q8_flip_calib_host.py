"""CPU: the calibration flow of the INT8 Flipout layers without a GPU -- what ``prepare(flipout=True)`` does
and which layers still refuse it, the walk and the pairing, the C ABI's refusals (before any launch), plan-only records and kernel
names, the fixtures the reference's own flow recorded (tests/golden/q8cal_flip_*.npz, tools/make_q8cal_flip_goldens.py) against
``observer_qparams`` and against the double-precision oracle, and the converter's ten pairs and refusals. No kernels are launched."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import _q8_flip_model as FM
import _q8cal_cases as K
import _q8cal_flip_cases as KF
from conftest import ROOT

INF = float("inf")


def test_prepare_on_request_registers_thirteen_statistics():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import functional as F
    assert F.CALIB_FLIP_ROWS == KF.ROWS and len(F.CALIB_FLIP_ROWS) == 13
    assert [F.CALIB_FLIP_ROWS[i] for i in KF.PAIR_ROWS] == list(F.Q8_FLIP_PAIRS) == list(FM.PAIRS)
    for layer in (L.LinearFlipout(6, 3), L.Conv2dFlipout(5, 7, 3, padding=1)):
        with pytest.raises(NotImplementedError):          # without the keyword it keeps raising
            layer.prepare()
        with pytest.raises(NotImplementedError):
            layer.prepare(flipout=False)
        assert layer.quant_prepare is False and "calib_minmax" not in layer.state_dict()
        layer.prepare(flipout=True)
        assert layer.quant_prepare is True and layer._calib_fused is False and layer.calib_coef is None and layer.calib_shift is None
        mm, bad = layer.calib_minmax, layer.calib_nonfinite
        assert mm.shape == (13, 2) and mm.dtype == torch.float32 and bool((mm[:, 0] == INF).all()) and bool((mm[:, 1] == -INF).all())
        assert bad.numel() == 1 and not bad.dtype.is_floating_point and int(bad) == 0
        assert {"calib_minmax", "calib_nonfinite"} <= set(layer.state_dict()) and "calib_coef" not in layer.state_dict()
    bn = nn.BatchNorm2d(7).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5), bn.bias.normal_(), bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2.0)
    conv = L.Conv2dFlipout(5, 7, 3, padding=1)
    conv.prepare(flipout=True, bn=bn)
    coef, shift = KF.bn_affine(bn)
    assert conv._calib_fused and len(bn._forward_hooks) == 1 and torch.equal(conv.calib_coef, coef) and torch.equal(conv.calib_shift, shift)
    conv.prepare(flipout=True)          # a second prepare() takes the hook out again
    assert not bn._forward_hooks and not conv._calib_fused


def test_prepare_still_raises_elsewhere():
    import bayesian_torch_amd.layers as L
    for layer in (L.Conv1dFlipout(2, 2, 3), L.Conv3dFlipout(2, 2, 3), L.ConvTranspose2dFlipout(2, 2, 3), L.QuantizedLinearFlipout(3, 2), L.QuantizedConv2dFlipout(2, 2, 3)):
        for kw in ({}, {"flipout": True}):
            with pytest.raises((NotImplementedError, TypeError)):
                layer.prepare(**kw)
        assert getattr(layer, "quant_prepare", False) is False
    with pytest.raises(NotImplementedError, match="float Flipout layer"):          # the message names the flow that exists
        L.QuantizedConv2dFlipout(2, 2, 3).prepare()
    with pytest.raises(NotImplementedError, match="groups"):
        L.Conv2dFlipout(4, 4, 3, groups=2).prepare(flipout=True)
    staged = L.Conv2dFlipout(4, 4, 3)
    staged.post_relu = True
    with pytest.raises(RuntimeError, match="output stage"):
        staged.prepare(flipout=True)
    bn = nn.BatchNorm2d(4).train()
    with pytest.raises(RuntimeError, match="training mode"):
        L.Conv2dFlipout(4, 4, 3).prepare(flipout=True, bn=bn)
    with pytest.raises(TypeError):          # the Reparameterization layers take no such keyword
        L.Conv2dReparameterization(4, 4, 3).prepare(flipout=True)


class _Mixed(nn.Module):
    """conv1 / bn1 and conv2 / bn2 are pairs of the folding rules; one of each estimator."""

    def __init__(self, L):
        super().__init__()
        self.conv1 = L.Conv2dFlipout(3, 4, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(4)
        self.conv2 = L.Conv2dReparameterization(4, 4, 3, 1, 1)
        self.bn2 = nn.BatchNorm2d(4)
        self.odd = L.Conv1dFlipout(2, 2, 3)
        self.fc = L.LinearFlipout(4, 2)


def test_walk_and_pairing():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.quantization import enable_prepare, prepare
    prepared = lambda net: [n for n, m in net.named_modules() if getattr(m, "quant_prepare", False)]
    net = _Mixed(L).eval()
    assert prepare(net) is net and prepared(net) == ["conv2"]                    # by default the Flipout layers are left alone
    net = _Mixed(L).eval()
    assert enable_prepare(net, flipout=True) == ["conv1", "conv2", "fc"] and prepared(net) == ["conv1", "conv2", "fc"]
    assert net.conv1.calib_minmax.shape == (13, 2) and net.conv2.calib_minmax.shape == (7, 2) and not net.bn1._forward_hooks
    assert all(getattr(net, n).dnn_to_bnn_flag for n in ("conv1", "conv2", "fc")) and not net.odd.quant_prepare
    net = _Mixed(L).eval()
    prepare(net, fuse_conv_bn=True, flipout=True)
    assert prepared(net) == ["conv1", "conv2", "fc"]
    for conv, bn in ((net.conv1, net.bn1), (net.conv2, net.bn2)):
        assert conv._calib_fused and len(bn._forward_hooks) == 1 and torch.equal(conv.calib_coef, K.bn_coef(bn))
    assert torch.equal(net.conv1.calib_shift, KF.bn_affine(net.bn1)[1]) and not net.fc._calib_fused
    net = _Mixed(L).eval()
    prepare(net, fuse_conv_bn=True)
    assert prepared(net) == ["conv2"] and not net.bn1._forward_hooks
    with pytest.raises(RuntimeError, match="eval"):
        prepare(_Mixed(L), flipout=True)


# ---------------------------------------------------------------------------- the C ABI
def _calls(_lib, L):
    P = _lib.bt_params(1024, 2048, 3072, 4096, None, None, None, None, None, None, 0, 0)
    P_nob = _lib.bt_params(1024, 2048, None, None, None, None, None, None, None, None, 0, 0)
    rng = lambda: _lib.bt_rng(1, None, 0, 1, 0, 0)
    ok = dict(B=5, In=64, Out=7, S=1, x=8192, stride=0, p=P, eps_w=None, eps_b=None, sign_in=None, sign_out=None, coef=None, shift=None,
              mm=(16384, 16392, 16400, 16408), bad=16416, groups=1, flags=0)

    def lin(**kw):
        a = dict(ok, **kw)
        R = rng()
        R.flags = a["flags"]
        D = _lib.bt_draws(a["eps_w"], a["eps_b"], a["sign_in"], a["sign_out"], R)
        return L.bt_q8_flip_observe_linear(a["B"], a["In"], a["Out"], a["S"], a["x"], a["stride"], None if a["p"] is None else C.byref(a["p"]), C.byref(D), a["coef"],
                                           a["shift"], *a["mm"], a["bad"], None)

    def conv(**kw):
        a = dict(ok, **kw)
        g = _lib.bt_conv2d_geom(2, 4, 9, 9, 8, 3, 3, 1, 1, 1, 1, 1, 1, a["groups"])
        D = _lib.bt_draws(a["eps_w"], a["eps_b"], a["sign_in"], a["sign_out"], rng())
        return L.bt_q8_flip_observe_conv2d(C.byref(g) if a.get("geom", True) else None, a["S"], a["x"], a["stride"], C.byref(a["p"]), C.byref(D), a["coef"], a["shift"],
                                           *a["mm"], a["bad"], None)

    def sweep(n=100, S=1, x=8192, stride=0, sign_in=None, use_rng=True, mm=(16384, 16392, 16400), bad=16416):
        R = rng()
        return L.bt_q8_flip_observe_x(n, S, x, stride, sign_in, C.byref(R) if use_rng else None, *mm, bad, None)

    return lin, conv, sweep, P_nob


def test_c_abi_refuses_before_any_launch():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    err = lambda: L.bt_last_error_string()
    lin, conv, sweep, P_nob = _calls(_lib, L)
    whole = dict(eps_w=512, eps_b=640, sign_in=768, sign_out=896)
    # BT_ERR_BAD_ARG: null pointers, S < 1, some draws supplied and others not, misaligned pointers
    assert lin(x=None) == -1 and lin(p=None) == -1 and lin(bad=None) == -1 and b"null" in err()
    for i in range(4):
        mm = [16384, 16392, 16400, 16408]
        mm[i] = None
        assert lin(mm=tuple(mm)) == -1 and b"null statistics" in err()
    assert conv(geom=False) == -1 and b"null geometry" in err()
    assert lin(S=0) == -1 and lin(B=0) == -1
    for k in whole:          # a partial draw: every subset but all and none
        part = dict(whole)
        part.pop(k)
        assert lin(**part) == -1 and b"inject all draws" in err(), k
    assert lin(eps_w=512) == -1 and lin(sign_out=896) == -1
    assert lin(p=P_nob, eps_w=512, eps_b=640, sign_in=768, sign_out=896) == -1 and b"without bias" in err()
    assert lin(coef=256) == -1 and lin(shift=256) == -1 and b"scale and shift" in err()
    assert lin(x=8194) == -1 and b"4-byte aligned" in err()
    assert lin(coef=258, shift=256) == -1 and lin(mm=(16386, 16392, 16400, 16408)) == -1 and lin(bad=16418) == -1 and lin(**dict(whole, sign_in=770)) == -1
    assert lin(flags=1) == -1 and b"flags" in err()
    # BT_ERR_UNSUPPORTED: groups, S, the sizes the fp32 general kernel refuses
    assert conv(groups=2) == -2 and b"groups" in err()
    assert lin(S=65536) == -2 and b"65535" in err()
    assert lin(B=1 << 16, In=1 << 15) == -2 and b"2^30" in err()
    g = _lib.bt_conv2d_geom(1, 1, 40, 40, 1, 12, 12, 1, 1, 0, 0, 1, 1, 1)          # 144 taps
    D = _lib.bt_draws(None, None, None, None, _lib.bt_rng(1, None, 0, 1, 0, 0))
    P = _lib.bt_params(1024, 2048, None, None, None, None, None, None, None, None, 0, 0)
    assert L.bt_q8_flip_observe_conv2d(C.byref(g), 1, 8192, 0, C.byref(P), C.byref(D), None, None, 16384, 16392, 16400, 16408, 16416, None) == -2 and b"128 taps" in err()
    # the sweep
    assert sweep(x=None) == -1 and sweep(bad=None) == -1 and sweep(mm=(16384, None, 16400)) == -1 and b"null" in err()
    assert sweep(S=0) == -1 and sweep(n=0) == -1 and sweep(stride=-1) == -1
    assert sweep(use_rng=False) == -1 and b"draw source" in err()                 # neither
    assert sweep(sign_in=768) == -1 and b"draw source" in err()                   # both
    assert sweep(x=8193) == -1 and sweep(sign_in=770, use_rng=False) == -1 and b"aligned" in err()
    assert sweep(S=65536) == -2 and sweep(n=1 << 32) == -2


def test_plan_only_launches_and_kernel_names():
    """The host side up to the launch, recorded instead of made (bt_debug_plan_only): grids, workgroup sizes and the kernel names."""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    lin, conv, sweep, P_nob = _calls(_lib, L)
    handle = C.CDLL(_lib.LIB_PATH)
    handle.bt_debug_last_launch_record.argtypes = [C.POINTER(C.c_int64), C.c_int]
    handle.bt_debug_plan_only(1)
    try:
        rec = (C.c_int64 * 11)()
        whole = dict(eps_w=512, eps_b=640, sign_in=768, sign_out=896)
        assert lin() == 0 and L.bt_last_kernel_name() == b"fused_fwd_kernel<64,64,2,flip,linear,trans,inj=0,obs>"
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:6]) == [1, 1, 1, 512, 1, 1]
        assert _lib.last_launch_info()["n_tiles"] == 1 and _lib.last_launch_info()["m_tiles"] == 1 and _lib.last_launch_info()["fused_kl"] == 0
        assert lin(**whole) == 0 and L.bt_last_kernel_name() == b"fused_fwd_kernel<64,64,2,flip,linear,trans,inj=1,obs>"
        assert lin(In=567, S=3, B=70, Out=130) == 0 and L.bt_last_kernel_name() == b"fused_fwd_kernel<64,64,2,flip,conv,trans,inj=0,obs>"          # K % 4 != 0: the 1 x 1 convolution
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:3]) == [3 * 2 * 3, 1, 1]                                                                          # 3 channel tiles x 2 position tiles x 3 samples
        assert lin(x=8196) == 0 and L.bt_last_kernel_name() == b"fused_fwd_kernel<64,64,2,flip,conv,trans,inj=0,obs>"      # x not 16-byte aligned: no float4 rows
        assert conv() == 0 and L.bt_last_kernel_name() == b"fused_fwd_kernel<64,64,2,flip,conv,notrans,inj=0,obs>"
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:3]) == [3, 1, 1] and _lib.last_launch_info()["m_tiles"] == 3                                      # 2 x 81 positions
        assert conv(coef=256, shift=512, **whole) == 0 and L.bt_last_kernel_name() == b"fused_fwd_kernel<64,64,2,flip,conv,notrans,inj=1,obs>"
        assert sweep(n=5000, S=3) == 0 and L.bt_last_kernel_name() == b"q8_flip_observe_x<signs on chip>"
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:6]) == [5, 3, 1, 256, 1, 1]
        assert sweep(n=1 << 24, S=32) == 0                                       # a large input: 2048 workgroups in all
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:3]) == [64, 32, 1]
        assert sweep(sign_in=768, use_rng=False, stride=100) == 0 and L.bt_last_kernel_name() == b"q8_flip_observe_x<signs injected>"
    finally:
        handle.bt_debug_last_launch_record((C.c_int64 * 11)(), 11)
        handle.bt_debug_plan_only(0)


def test_header_binding_and_library_agree():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("bt_q8_flip_observe_conv2d", 14), ("bt_q8_flip_observe_linear", 16), ("bt_q8_flip_observe_x", 11)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._PROTOS[name][1]), name
        assert name in _lib.EXPORTS and hasattr(handle, name), name
    assert _lib.lib().bt_version() == 302
    mk = open(os.path.join(ROOT, "bayesian_torch_amd", "csrc", "Makefile")).read()
    assert "bt_fused_flipout_obs.hip" in mk and "bt_observe.h" in mk and "bt_q8_observe.hip" in mk


# ---------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("tag", KF.FIXTURES)
def test_recorded_ranges_give_the_recorded_scales(tag):
    """The reference's own twelve observers: their recorded (min, max) give the (scale, zero point) its convert() left on every stub,
    exactly, and with them the ten-entry selection in Q8_FLIP_PAIRS' order."""
    from bayesian_torch_amd.quantization import observer_qparams
    g = KF.load(tag)
    assert g["minmax13"].shape == (13, 2) and tuple(g["minmax13"][4].tolist()) == (INF, -INF)
    for row, name in enumerate(KF.ROWS):
        if name == "add":
            continue
        s, z = observer_qparams(g["minmax13"][row, 0], g["minmax13"][row, 1], torch.qint8 if row < 4 else torch.quint8)
        assert torch.equal(s, g["scales13"][row]) and int(z) == int(g["zero_points13"][row]), (name, float(s), float(g["scales13"][row]), int(z))
    qd = KF.dict_of(g["minmax13"])
    assert [torch.tensor(d["scale"], dtype=torch.float64).float().item() for d in qd] == g["dict_scales"].tolist()
    assert [d["zero_point"] for d in qd] == g["dict_zero_points"].tolist()
    for name in ("mean", "pert", "pert_signed", "out"):          # the generator's promise: no tolerance row's zero point sits near a rounding tie
        i = KF.ROWS.index(name)
        q = min(float(g["minmax13"][i, 0]), 0.0) / float(g["scales13"][i])
        assert abs(abs(q - int(q)) - 0.5) >= 1e-3, (name, q)


@pytest.mark.parametrize("tag", KF.FIXTURES)
def test_the_oracle_reproduces_the_recorded_ranges(tag):
    """``float_flipout`` (double) on the recorded draws against the reference's twelve recorded ranges, within the tolerances the device
    is held to: this holds the oracle of the GPU tests to the reference."""
    g = KF.load(tag)
    conv = None if tag.startswith("linear") else KF.CONV1
    n = g["x"].shape[0]
    mm = None
    mags = {}
    for i in range(n):          # three calibration batches of one sample each, merged
        m1, g1 = KF.host_stats(g["x"][i], g["mu_w"], g["rho_w"], g["eps_w"][i:i + 1], g["sign_in"][i:i + 1], g["sign_out"][i:i + 1], g["mu_b"], g["rho_b"],
                               g["eps_b"][i:i + 1], conv)
        mm = m1 if mm is None else torch.stack([torch.minimum(mm[:, 0], m1[:, 0]), torch.maximum(mm[:, 1], m1[:, 1])], 1)
        mags = {k: max(v, mags.get(k, 0.0)) for k, v in g1.items()}
    seen = KF.check_rows(mm, g["minmax13"], mags, f"oracle vs recorded {tag}")
    assert set(seen) == set(KF.ROWS) - {"add"}


# ---------------------------------------------------------------------------- the converter
def _plant(net, stats):
    for name, (mm, _) in stats.items():
        getattr(net, name).calib_minmax.copy_(mm.float())


def test_converter_builds_ten_pairs_and_refuses():
    from bayesian_torch_amd.quantization import convert, prepare
    net, xs, draws = KF.fold_net()
    stats = KF.fold_host_stats(KF.fold_net()[0], xs, draws)          # host-planted statistics (from an unprepared twin)
    prepare(net, fuse_conv_bn=True, flipout=True)
    with pytest.raises(RuntimeError, match="conv1.*still empty"):          # prepared, never run
        convert(net, fuse_conv_bn=True, flipout=True)
    _plant(net, stats)
    net.conv1.calib_minmax[4] = torch.tensor([INF, -INF])          # "add": not needed, may stay empty; so may sigma and mu
    net.conv1.calib_minmax[0] = torch.tensor([INF, -INF])
    with pytest.raises(RuntimeError, match="prepared with fuse_conv_bn=True and is being converted with fuse_conv_bn=False"):
        convert(net, fuse_conv_bn=False, flipout=True)
    net.fc.calib_nonfinite.fill_(3)
    with pytest.raises(RuntimeError, match="fc.*non-finite"):
        convert(net, fuse_conv_bn=True, flipout=True)          # (conv1 is converted by then; the model is rebuilt below)
    net, _, _ = KF.fold_net()
    prepare(net, fuse_conv_bn=True, flipout=True)
    _plant(net, stats)
    net.fc.calib_minmax[KF.ROWS.index("pert_signed")] = torch.tensor([INF, -INF])
    with pytest.raises(RuntimeError, match="fc.*pert_signed.*still empty"):
        convert(net, fuse_conv_bn=True, flipout=True)
    net, _, _ = KF.fold_net()
    prepare(net, fuse_conv_bn=True, flipout=True)
    _plant(net, stats)
    bn = net.bn1
    assert convert(net, fuse_conv_bn=True, flipout=True) is net
    assert type(net.conv1).__name__ == "QuantizedConv2dFlipout" and type(net.fc).__name__ == "QuantizedLinearFlipout"
    assert type(net.bn1).__name__ == "Identity" and not bn._forward_hooks
    for name in ("conv1", "fc"):
        q, mm = getattr(net, name), stats[name][0].float()
        assert len(q.quant_dict) == 10 and q.quant_dict == KF.dict_of(mm)
        assert all(type(d["scale"]) is float and type(d["zero_point"]) is int for d in q.quant_dict)
        assert q.quant_dict[0]["zero_point"] == 0 and q.quant_dict[1]["zero_point"] == 0          # eps, delta: symmetric
        for i, pname in enumerate(FM.PAIRS):          # the right row behind every entry: the scale is its range's
            lo, hi = mm[KF.ROWS.index(pname)].tolist()
            span = max(-min(lo, 0.0), max(hi, 0.0)) / 127.5 if i < 2 else (max(hi, 0.0) - min(lo, 0.0)) / 255
            assert abs(q.quant_dict[i]["scale"] - span) <= 1e-6 * span, (name, pname)
    plain, _, _ = KF.fold_net()          # unprepared Flipout layers convert exactly as before: the default pairs
    convert(plain, fuse_conv_bn=True, flipout=True)
    assert plain.conv1.quant_dict is None and plain.fc.quant_dict is None
    assert torch.equal(net.conv1.quantized_mu_weight, plain.conv1.quantized_mu_weight) and torch.equal(net.fc.quantized_sigma_weight, plain.fc.quantized_sigma_weight)
