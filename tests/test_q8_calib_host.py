"""CPU: the calibration flow of the INT8 layers without a GPU -- ``observer_qparams`` against torch's MinMaxObserver with exact
equality, the fixtures the reference's prepare / calibrate / convert flow recorded (tests/golden/q8cal_*.npz,
tools/make_q8cal_goldens.py), the C ABI's refusals (before any launch) and surface, the alias import paths, what ``prepare()`` does and
which layers still refuse it, and the converter's refusals (never calibrated, non-finite values, the other ``fuse_conv_bn``). No kernels
are launched."""
import ctypes as C
import itertools
import os
import re
import warnings

import pytest
import torch
import torch.nn as nn

import _q8cal_cases as K
from conftest import ROOT


def _grid():
    """(min, max) pairs: every ordered pair of a value list that crosses zero, all-positive and all-negative ranges, min = max = 0,
    ranges below 1e-8, and ranges whose affine zero point clamps at 0 (all positive) and at 255 (all negative)."""
    vals = [0.0, 1e-12, 3e-10, 9.9e-9, 1e-8, 1.1920929e-07, 2.5e-7, 1e-5, 0.00123, 0.0291, 0.1, 0.3337, 1.0, 2.7182817, 5.0, 12.75, 127.5, 255.0, 1e3, 3.3e7, 1e30]
    vals = sorted(set(vals + [-v for v in vals]))
    pairs = [(a, b) for a, b in itertools.product(vals, vals) if a <= b]
    g = torch.Generator().manual_seed(11)
    rnd = torch.randn(1500, 2, generator=g) * torch.pow(10.0, torch.randint(-9, 3, (1500, 1), generator=g).float())
    pairs += [(float(min(a, b)), float(max(a, b))) for a, b in rnd.tolist()]
    return pairs


def test_observer_qparams_is_minmaxobserver_exactly():
    from torch.ao.quantization.observer import MinMaxObserver
    from bayesian_torch_amd.quantization import observer_qparams
    pairs = _grid()
    assert len(pairs) >= 2000
    assert (0.0, 0.0) in pairs and any(0 < b - a < 1e-8 for a, b in pairs) and any(a > 0 for a, b in pairs) and any(b < 0 for a, b in pairs)
    clamp = set()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dtype, scheme in ((torch.qint8, torch.per_tensor_symmetric), (torch.quint8, torch.per_tensor_affine)):
            obs = MinMaxObserver(dtype=dtype, qscheme=scheme)
            for lo, hi in pairs:
                obs.min_val, obs.max_val = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
                s, z = obs.calculate_qparams()
                s2, z2 = observer_qparams(lo, hi, dtype)
                assert s2.dtype == torch.float32 and torch.equal(s.reshape(()), s2) and int(z) == int(z2), (dtype, lo, hi, float(s), float(s2), int(z), int(z2))
                if dtype == torch.quint8:
                    clamp.add(int(z2))
                else:
                    assert int(z2) == 0
    assert 0 in clamp and 255 in clamp
    with pytest.raises(ValueError):
        observer_qparams(0.0, 1.0, torch.qint32)


@pytest.mark.parametrize("tag", K.FIXTURES)
def test_recorded_ranges_give_the_recorded_scales(tag):
    """The reference's own observers: their recorded (min, max) give the (scale, zero point) its convert() left on every stub, and
    the five-entry quant_dict its converter selected, exactly."""
    from bayesian_torch_amd.quantization import observer_qparams
    g = K.load(tag)
    assert g["minmax"].shape == (7, 2)
    for row in range(7):
        s, z = observer_qparams(g["minmax"][row, 0], g["minmax"][row, 1], torch.qint8 if row < 5 else torch.quint8)
        assert torch.equal(s, g["scales"][row]) and int(z) == int(g["zero_points"][row]), (row, float(s), float(g["scales"][row]))
    qd = K.dict_of(g["minmax"])
    assert [torch.tensor(d["scale"], dtype=torch.float64).float().item() for d in qd] == g["dict_scales"].tolist()
    assert [d["zero_point"] for d in qd] == g["dict_zero_points"].tolist()
    # and the recorded ranges are those of the recorded tensors (the fixture is self-consistent)
    rows = K.host_weight_rows(g["mu_w"], g["rho_w"], g["eps_w"])
    assert K.aminmax(rows["eps"]) == tuple(g["minmax"][2].tolist()) and K.aminmax(rows["mu"]) == tuple(g["minmax"][1].tolist())
    assert K.aminmax(g["x"]) == tuple(g["minmax"][5].tolist())


def test_c_abi_refuses_before_any_launch():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    R = _lib.bt_rng(1, None, 0, 1, 0, 0)
    ok = dict(mu=1024, rho=2048, coef=None, rows=4, inner=5, taps=9, S=1, eps=None, rng=C.byref(R), stats=4096, bad=8192)

    def obs(**kw):
        a = dict(ok, **kw)
        return L.bt_q8_observe_w(a["mu"], a["rho"], a["coef"], a["rows"], a["inner"], a["taps"], a["S"], a["eps"], a["rng"], a["stats"], a["bad"], None)

    for name in ("mu", "rho", "stats", "bad"):
        assert obs(**{name: None}) == -1 and b"null" in L.bt_last_error_string(), name
    assert obs(S=0) == -1 and obs(rows=0) == -1 and obs(inner=0) == -1 and obs(taps=0) == -1
    assert obs(rng=None) == -1 and b"draw source" in L.bt_last_error_string()          # neither
    assert obs(eps=512) == -1 and b"draw source" in L.bt_last_error_string()            # both
    assert obs(mu=1026) == -1 and b"aligned" in L.bt_last_error_string()
    assert obs(S=65536) == -2 and obs(rows=1 << 20, inner=1 << 20, taps=4) == -2

    def mm(n, segs, bad=8192):
        arr = (_lib.bt_minmax_seg * max(1, len(segs)))(*[_lib.bt_minmax_seg(*s) for s in segs])
        return L.bt_minmax_update(n, arr if segs else None, bad, None)

    seg = (1024, 7, 2048)
    assert mm(0, [seg]) == -1 and mm(5, [seg] * 5) == -1 and b"1 to 4" in L.bt_last_error_string()
    assert mm(1, []) == -1 and mm(1, [seg], bad=None) == -1
    assert mm(1, [(None, 7, 2048)]) == -1 and mm(1, [(1024, 7, None)]) == -1 and mm(2, [seg, (1024, 0, 2048)]) == -1
    assert mm(1, [(1025, 7, 2048)]) == -1 and b"aligned" in L.bt_last_error_string()


def test_plan_only_launches_and_kernel_names():
    """The host side up to the launch, recorded instead of made (bt_debug_plan_only): grid shapes and the kernel names."""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    handle = C.CDLL(_lib.LIB_PATH)
    handle.bt_debug_plan_only(1)
    try:
        rec = (C.c_int64 * 11)()
        R = _lib.bt_rng(1, None, 0, 1, 0, 0)
        assert L.bt_q8_observe_w(1024, 2048, None, 33, 19, 9, 3, None, C.byref(R), 4096, 8192, None) == 0
        assert L.bt_last_kernel_name() == b"q8_observe_w<eps on chip>"
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:6]) == [((33 * 19 * 9 + 3) // 4 + 255) // 256, 3, 1, 256, 1, 1] and rec[9] == 1
        assert L.bt_q8_observe_w(1024, 2048, None, 512, 512, 9, 32, None, C.byref(R), 4096, 8192, None) == 0          # a large layer: 2048 workgroups in all
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:3]) == [64, 32, 1]
        assert L.bt_q8_observe_w(1024, 2048, 512, 33, 19, 9, 3, 16384, None, 4096, 8192, None) == 0
        assert L.bt_last_kernel_name() == b"q8_observe_w<eps injected>"
        handle.bt_debug_last_launch_record(rec, 11)
        assert list(rec[:3]) == [((33 * 19 * 9 + 3) // 4 + 255) // 256, 3, 1]
        for k in (1, 2, 3, 4):
            arr = (_lib.bt_minmax_seg * k)(*[_lib.bt_minmax_seg(1024, 5000 if i == 0 else 3, 2048) for i in range(k)])
            assert L.bt_minmax_update(k, arr, 8192, None) == 0
            assert L.bt_last_kernel_name() == f"minmax_update<{k} segs>".encode()
            handle.bt_debug_last_launch_record(rec, 11)
            assert list(rec[:3]) == [5, k, 1]
    finally:
        handle.bt_debug_plan_only(0)


def test_header_binding_and_library_agree():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in ("bt_q8_observe_w", "bt_minmax_update"):
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), name
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(handle, name), name
    assert "#define BT_MINMAX_MAX_SEGS 4" in hdr and _lib.MINMAX_MAX_SEGS == 4 and C.sizeof(_lib.bt_minmax_seg) == 24
    assert _lib.lib().bt_version() == 302
    assert "bt_q8_observe.hip" in open(os.path.join(ROOT, "bayesian_torch_amd", "csrc", "Makefile")).read()


def test_alias_imports():
    import bayesian_torch.ao.quantization.quantize as A
    import bayesian_torch.quantization.quantize as R
    import bayesian_torch_amd.quantization.quantize as Q
    from bayesian_torch.quantization import convert, prepare
    for name in ("observer_qparams", "enable_prepare", "prepare", "convert"):
        assert getattr(A, name) is getattr(R, name) is getattr(Q, name), name
    assert prepare is Q.prepare and convert is Q.convert


def test_prepare_registers_the_statistics():
    import bayesian_torch_amd.layers as L
    for layer in (L.LinearReparameterization(6, 3), L.Conv2dReparameterization(5, 7, 3, padding=1)):
        assert layer.quant_prepare is False and "calib_minmax" not in layer.state_dict()
        layer.prepare()
        assert layer.quant_prepare is True and layer._calib_fused is False and layer.calib_coef is None
        mm, bad = layer.calib_minmax, layer.calib_nonfinite
        assert mm.shape == (7, 2) and mm.dtype == torch.float32 and bool((mm[:, 0] == float("inf")).all()) and bool((mm[:, 1] == float("-inf")).all())
        assert bad.numel() == 1 and not bad.dtype.is_floating_point and int(bad) == 0
        assert {"calib_minmax", "calib_nonfinite"} <= set(layer.state_dict())          # persistent


def test_prepare_still_raises_elsewhere():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.layers.variational_layers import hiearchial_variational_layers as H
    from bayesian_torch_amd.layers.variational_layers.conv_variational import Conv2dReparameterization_Multivariate
    for layer in (L.LinearFlipout(3, 2), L.Conv2dFlipout(2, 2, 3), L.Conv1dReparameterization(2, 2, 3), L.ConvTranspose2dReparameterization(2, 2, 3),
                  Conv2dReparameterization_Multivariate(2, 2, 3), L.QuantizedLinearReparameterization(3, 2), L.QuantizedConv2dReparameterization(2, 2, 3),
                  H.LinearReparameterizationHierarchical_Weightwise(3, 2), H.Conv2dReparameterizationHierarchical_Weightwise(2, 2, 3, bias=False)):
        with pytest.raises(NotImplementedError):
            layer.prepare()
        assert getattr(layer, "quant_prepare", False) is False
    with pytest.raises(NotImplementedError, match="groups"):
        L.Conv2dReparameterization(4, 4, 3, groups=2).prepare()
    staged = L.Conv2dReparameterization(4, 4, 3)
    staged.post_relu = True                                    # what fuse.py folds in
    with pytest.raises(RuntimeError, match="output stage"):
        staged.prepare()
    staged = L.LinearReparameterization(4, 4)
    staged.post_scale = torch.ones(4)
    with pytest.raises(RuntimeError, match="output stage"):
        staged.prepare()


def test_enable_prepare_walk_and_pairing():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.models.bnn_to_qbnn import conv_bn_pairs
    from bayesian_torch_amd.quantization import enable_prepare, prepare
    from test_q8_host import _Net
    net = _Net(L).eval()
    names = enable_prepare(net)
    assert names == ["conv1", "layer1.0.conv1", "layer1.0.conv2", "layer1.0.downsample.0", "layer1.0.extra", "fc"]
    assert all(m.dnn_to_bnn_flag and not m._calib_fused for m in net.modules() if getattr(m, "quant_prepare", False))
    assert not net.bn1._forward_hooks
    net = _Net(L).eval()
    assert [(c, b) for _, c, b in conv_bn_pairs(net.layer1[0])] == [("conv1", "bn1"), ("conv2", "bn2"), ("0", "1")]
    assert prepare(net, fuse_conv_bn=True) is net
    blk = net.layer1[0]
    assert [n for n, m in net.named_modules() if getattr(m, "quant_prepare", False)] == ["conv1", "layer1.0.conv1", "layer1.0.conv2", "layer1.0.downsample.0", "fc"]
    assert blk.extra.quant_prepare is False                    # no folding rule names it: it stays float in the converted model
    for conv, bn in ((net.conv1, net.bn1), (blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.downsample[0], blk.downsample[1])):
        assert conv._calib_fused and len(bn._forward_hooks) == 1
        assert torch.equal(conv.calib_coef, K.bn_coef(bn))
    assert net.fc._calib_fused is False
    with pytest.raises(RuntimeError, match="eval"):
        prepare(_Net(L), fuse_conv_bn=True)
    tr = _Net(L).eval()
    tr.layer1[0].bn2.train()
    with pytest.raises(RuntimeError, match="training mode"):
        enable_prepare(tr, fuse_conv_bn=True)


def _calibrated_by_hand(net, stats):
    for name, mm in stats.items():
        getattr(net, name).calib_minmax.copy_(mm)


def test_converter_uses_and_refuses_the_statistics():
    from bayesian_torch_amd.quantization import convert, prepare
    net, xs, draws = K.fold_net()
    prepare(net, fuse_conv_bn=True)
    with pytest.raises(RuntimeError, match="conv1.*still empty"):              # prepared, never run
        convert(net, fuse_conv_bn=True)
    stats = K.host_stats(K.fold_net()[0], xs, draws, True)          # (from an unprepared twin: the prepared model's BatchNorm hook observes on the device)
    _calibrated_by_hand(net, stats)
    with pytest.raises(RuntimeError, match="prepared with fuse_conv_bn=True and is being converted with fuse_conv_bn=False"):
        convert(net, fuse_conv_bn=False)
    net.fc.calib_nonfinite.fill_(3)
    with pytest.raises(RuntimeError, match="fc.*non-finite"):
        convert(net, fuse_conv_bn=True)      # (conv1 is converted by then; the model is rebuilt below)
    net, xs, draws = K.fold_net()
    prepare(net, fuse_conv_bn=False)
    _calibrated_by_hand(net, K.host_stats(K.fold_net()[0], xs, draws, False))
    with pytest.raises(RuntimeError, match="prepared with fuse_conv_bn=False and is being converted with fuse_conv_bn=True"):
        convert(net, fuse_conv_bn=True)
    net, xs, draws = K.fold_net()
    prepare(net, fuse_conv_bn=True)
    stats = K.host_stats(K.fold_net()[0], xs, draws, True)          # (from an unprepared twin: the prepared model's BatchNorm hook observes on the device)
    _calibrated_by_hand(net, stats)
    bn = net.bn1
    assert convert(net, fuse_conv_bn=True) is net
    assert type(net.conv1).__name__ == "QuantizedConv2dReparameterization" and type(net.bn1).__name__ == "Identity" and not bn._forward_hooks
    for name in ("conv1", "fc"):
        q = getattr(net, name)
        assert q.quant_dict == K.dict_of(stats[name]) and len(q.quant_dict) == 5
        assert all(type(d["scale"]) is float and type(d["zero_point"]) is int for d in q.quant_dict)
    direct, _, _ = K.converted_cpu(True, True)                  # the same int8 images as a conversion that was never prepared
    assert torch.equal(net.conv1.quantized_mu_weight, direct.conv1.quantized_mu_weight) and torch.equal(net.fc.quantized_sigma_weight, direct.fc.quantized_sigma_weight)
    plain, _, _ = K.fold_net()                                   # unprepared layers convert as before: the default branch
    convert(plain, fuse_conv_bn=True)
    assert plain.conv1.quant_dict is None and plain.fc.quant_dict is None


def test_calibration_helps_on_the_cpu_model():
    """The inequality of the GPU test "it helps", held on the CPU model (tests/_q8_model.py) with statistics computed on the host."""
    calibrated, default = K.helps_on_cpu()
    print(f"mean |int8 - float|: calibrated {calibrated:.5f}, default branch {default:.5f}")
    assert calibrated < default
