"""CPU: u8 activations between the INT8 layers without a GPU -- the carrier's blocked layout and surface, the __torch_function__
dispatch of an unmodified model's modules (the launch functions monkeypatched), the refusals of the new entry points (raised on the
host, before any launch), the C ABI's surface and the alias imports. No kernels are launched."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import _q8_u8_model as U
from conftest import ROOT

NEW = ("bt_q8_conv2d_fwd_act", "bt_q8_linear_fwd_act", "bt_q8_flip_conv2d_fwd_act", "bt_q8_flip_linear_fwd_act", "bt_q8_act_quantize", "bt_q8_act_dequantize",
       "bt_q8_act_relu", "bt_q8_act_add", "bt_q8_act_max_pool2d", "bt_q8_act_avg_pool", "bt_q8_act_unblock")


def _levels(shape, seed=0):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(torch.uint8)


# ---------------------------------------------------------------------------- layout and surface
@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (1, 16, 2, 2), (3, 20, 3, 1), (2, 70, 2, 3), (4, 20), (2, 32), (3, 5)])
def test_blocked_layout_round_trips(shape):
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.quantization import qact
    lv = _levels(shape)
    q = qact.from_int_repr(lv, 0.05, 91)
    assert tuple(q.data.shape) == F.q8_blocked_shape(shape) and q.data.dtype == torch.uint8 and q.data.is_contiguous()
    assert torch.equal(q.data, U.block(lv, 91))                  # [N][ceil(C / 16)][H][W][16], padding channels hold the zero point
    assert torch.equal(q.int_repr(), lv) and q.int_repr().is_contiguous()
    assert q.q_scale() == 0.05 and q.q_zero_point() == 91 and q.dtype == torch.quint8
    assert q.shape == torch.Size(shape) and q.size() == torch.Size(shape) and q.size(1) == shape[1] and q.dim() == len(shape)
    assert q.device == lv.device and q.contiguous() is q


def test_flatten_of_a_1x1_map_is_free_and_larger_maps_launch(monkeypatch):
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.quantization import qact
    lv = _levels((3, 20, 1, 1))
    q = qact.from_int_repr(lv, 0.1, 7)
    calls = []
    monkeypatch.setattr(F, "q8_act_unblock", lambda data, shape, z: calls.append(tuple(shape)) or (U.block(U.unblock(data, shape).flatten(1), z), (shape[0], shape[1] * shape[2] * shape[3])))
    for f in (q.flatten(1), torch.flatten(q, 1), q.view(3, -1), q.reshape(3, -1), nn.Flatten()(q)):
        assert f.shape == (3, 20) and f.data.data_ptr() == q.data.data_ptr() and torch.equal(f.int_repr(), lv.flatten(1))
    assert calls == []
    lv = _levels((2, 5, 3, 2))
    q = qact.from_int_repr(lv, 0.1, 7)
    f = torch.flatten(q, 1)
    assert calls == [(2, 5, 3, 2)] and f.shape == (2, 30) and torch.equal(f.int_repr(), lv.flatten(1)) and f.pair == (0.1, 7)
    assert bool((f.data[:, 30:] == 7).all())
    with pytest.raises(NotImplementedError):
        q.flatten(0)
    with pytest.raises(NotImplementedError):
        q.view(4, -1)


def test_carrier_refuses_bad_pairs_and_shapes():
    from bayesian_torch_amd.quantization import qact
    lv = _levels((2, 3, 2, 2))
    for s, z in ((0.0, 0), (-1.0, 0), (0.1, -1), (0.1, 256)):
        with pytest.raises(ValueError):
            qact.from_int_repr(lv, s, z)
    with pytest.raises(ValueError, match="blocked"):
        qact.QActivation(lv, 0.1, 0, lv.shape)          # natural order is not the storage


# ---------------------------------------------------------------------------- dispatch
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.relu = nn.ReLU(inplace=True)
        self.relu2 = nn.ReLU()
        self.pool = nn.MaxPool2d(3, 2, 1)
        self.id = nn.Identity()
        self.avg = nn.AdaptiveAvgPool2d(1)
        self.flat = nn.Flatten()

    def forward(self, x):
        x = self.id(self.pool(self.relu2(self.relu(x))))
        return self.flat(self.avg(x))


def test_unmodified_modules_reach_the_carrier(monkeypatch):
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.quantization import qact
    log = []

    def fake_relu(data, shape, z, inplace=False):
        log.append(("relu", tuple(shape), z, inplace))
        out = torch.clamp(data, min=z)
        if inplace:
            data.copy_(out)
            return data
        return out

    def fake_pool(data, shape, kernel, stride, padding):
        log.append(("max_pool2d", tuple(shape), kernel, stride, padding))
        lv = U.max_pool2d(U.unblock(data, shape), kernel, stride, padding)
        return U.block(lv, 0), tuple(lv.shape)

    def fake_avg(data, shape, z):
        log.append(("avg_pool", tuple(shape), z))
        lv = U.avg_pool(U.unblock(data, shape), z)
        return U.block(lv, z), tuple(lv.shape)

    monkeypatch.setattr(F, "q8_act_relu", fake_relu)
    monkeypatch.setattr(F, "q8_act_max_pool2d", fake_pool)
    monkeypatch.setattr(F, "q8_act_avg_pool", fake_avg)
    lv = _levels((2, 5, 9, 7), 3)
    q = qact.from_int_repr(lv, 0.05, 100)
    out = _Net()(q)
    assert [e[0] for e in log] == ["relu", "relu", "max_pool2d", "avg_pool"]
    assert log[0] == ("relu", (2, 5, 9, 7), 100, True) and log[1][3] is False and log[2] == ("max_pool2d", (2, 5, 9, 7), (3, 3), (2, 2), (1, 1))
    assert log[3] == ("avg_pool", (2, 5, 5, 4), 100)
    assert isinstance(out, qact.QActivation) and out.shape == (2, 5) and out.pair == (0.05, 100)
    want = U.avg_pool(U.max_pool2d(U.relu(lv, 100), 3, 2, 1), 100).flatten(1)
    assert torch.equal(out.int_repr(), want)
    assert torch.equal(q.int_repr(), U.relu(lv, 100))          # nn.ReLU(inplace=True) wrote the carrier's own bytes
    # a global nn.AvgPool2d and the functional forms
    log.clear()
    q = qact.from_int_repr(lv, 0.05, 100)
    assert torch.equal(nn.AvgPool2d((9, 7))(q).int_repr(), U.avg_pool(lv, 100)) and log[-1][0] == "avg_pool"
    assert torch.relu(q).shape == q.shape and torch.nn.functional.relu(q, inplace=False).pair == q.pair
    with pytest.raises(NotImplementedError, match="global"):
        nn.AvgPool2d(3)(q)
    with pytest.raises(NotImplementedError):
        nn.AdaptiveAvgPool2d(2)(q)


def test_unknown_functions_and_plus_raise():
    from bayesian_torch_amd.quantization import qact
    q = qact.from_int_repr(_levels((2, 3, 2, 2)), 0.1, 0)
    with pytest.raises(TypeError, match="batch_norm"):          # there is no quantised BatchNorm: an unfused one raises
        nn.BatchNorm2d(3).eval()(q)
    with pytest.raises(TypeError, match="sigmoid"):
        torch.sigmoid(q)
    with pytest.raises(TypeError, match="cat"):
        torch.cat([q, q])
    for f in (lambda: q + q, lambda: q + 1.0, lambda: 1.0 + q, lambda: q + torch.zeros(2, 3, 2, 2)):
        with pytest.raises(TypeError, match="add_relu"):
            f()
    with pytest.raises(TypeError, match="QActivation"):
        qact.relu(torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="shapes differ"):
        qact.add(q, qact.from_int_repr(_levels((2, 3, 2, 1)), 0.1, 0))


def test_add_defaults_and_stubs(monkeypatch):
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.quantization import qact
    seen = []

    def fake_add(a, a_shape, pa, b, b_shape, pb, po, relu=False):
        seen.append((pa, pb, po, relu))
        f = U.add_relu if relu else U.add
        return U.block(f(U.unblock(a, a_shape), pa, U.unblock(b, b_shape), pb, po), po[1])

    monkeypatch.setattr(F, "q8_act_add", fake_add)
    a, b = qact.from_int_repr(_levels((2, 20, 3, 3), 1), 0.05, 100), qact.from_int_repr(_levels((2, 20, 3, 3), 2), 0.073, 57)
    r = qact.add_relu(a, b)
    assert r.pair == (0.073, 0) and seen[-1] == ((0.05, 100), (0.073, 57), (0.073, 0), True)      # the reference QResNet's max(scales), zero point 0
    assert torch.equal(r.int_repr(), U.add_relu(a.int_repr(), a.pair, b.int_repr(), b.pair, (0.073, 0)))
    assert qact.add(a, b, 0.2, 31).pair == (0.2, 31) and seen[-1][3] is False
    ff = qact.QFunctional(0.11, 5)
    assert ff.add(a, b).pair == (0.11, 5) and ff.add_relu(a, b).pair == (0.11, 5) and seen[-1] == ((0.05, 100), (0.073, 57), (0.11, 5), True)
    assert qact.QFunctional().add_relu(a, b).pair == (0.073, 0)
    monkeypatch.setattr(F, "q8_act_quantize", lambda x, s, z: U.block(torch.clamp(torch.round(x / s) + z, 0, 255).to(torch.uint8), z))
    monkeypatch.setattr(F, "q8_act_dequantize", lambda data, shape, s, z: U.deq(U.unblock(data, shape), (s, z)))
    x = torch.randn(2, 3, 4, 4)
    q = qact.QuantStub(0.05, 128)(x)
    assert isinstance(q, qact.QActivation) and q.pair == (0.05, 128) and qact.QuantStub(0.05, 128)(q) is q
    d = qact.DeQuantStub()(q)
    assert d.dtype == torch.float32 and d.shape == x.shape and float((d - x).abs().max()) <= 0.026 and qact.DeQuantStub()(x) is x
    assert torch.equal(q.dequantize(), d)


# ---------------------------------------------------------------------------- the layers
def test_layers_take_the_carrier_and_refuse_the_cpu():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.quantization import qact
    conv = L.QuantizedConv2dReparameterization(3, 4, 3, padding=1)
    assert conv.return_quantized is False
    q = qact.from_int_repr(_levels((2, 3, 4, 4)), 0.1, 128)
    with pytest.raises(RuntimeError, match="HIP"):          # no CPU forward -- but the carrier got past the fp32 check
        conv(q)
    lin = L.QuantizedLinearFlipout(20, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        lin(qact.from_int_repr(_levels((2, 20)), 0.1, 128))


def test_u8_inference_marks_a_converted_resnet_and_refuses_others():
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    prior = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization", "moped_enable": False,
             "moped_delta": 0.5}
    net = H.resnet18(10, 8)
    dnn_to_bnn(net, prior)
    net.eval()
    with pytest.raises(RuntimeError, match="fuse_conv_bn=True"):
        H.u8_inference(net)
    bnn_to_qbnn(net)                                        # BatchNorms left in place
    with pytest.raises(RuntimeError, match="BatchNorm"):
        H.u8_inference(net)
    net = H.resnet18(10, 8)
    dnn_to_bnn(net, prior)
    net.eval()
    bnn_to_qbnn(net, fuse_conv_bn=True)
    assert H.u8_inference(net) is net and net.conv1.return_quantized and net.u8 and all(b.u8 for s in (net.layer1, net.layer4) for b in s)
    assert not net.layer1[0].conv1.return_quantized and not net.fc.return_quantized


# ---------------------------------------------------------------------------- the C ABI
def _act_fwd(L, _lib, x=1024, kind=1, stride=0, out=None, out_b=4096, z_in=128, s_in=0.1, In=20, S=1):
    pr = [_lib.bt_q8_pair(s, z, 0) for s, z in [(6 / 255, 0), (1e-4, 0), (1e-3, 0), (s_in, z_in), (0.1, 128)]]
    P = _lib.bt_q8_params(*pr, 0.01, 0.01, 256, 512, None, None)      # (aligned non-null pack addresses: nothing is launched)
    R = _lib.bt_rng(1, None, 0, 1, 0, 0)
    return L.bt_q8_linear_fwd_act(2, In, 4, S, x, kind, stride, C.byref(P), None, None, C.byref(R), out, out_b, None)


def test_forward_entry_points_refuse_before_any_launch():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    err = lambda: L.bt_last_error_string()
    assert _act_fwd(L, _lib, x=None) == -1 and b"bt_q8_linear_fwd_act" in err()
    assert _act_fwd(L, _lib, out=None, out_b=None) == -1 and b"neither out nor out_blocked" in err() and b"bt_q8_linear_fwd_act" in err()
    assert _act_fwd(L, _lib, x=1028) == -1 and b"16-byte aligned" in err()
    assert _act_fwd(L, _lib, out_b=4100) == -1 and b"out_blocked must be 16-byte aligned" in err()
    assert _act_fwd(L, _lib, stride=24) == -1 and b"multiple of 16" in err()
    assert _act_fwd(L, _lib, kind=2) == -1 and b"x_kind" in err()
    assert _act_fwd(L, _lib, z_in=256) == -1 and b"zero point" in err()
    assert _act_fwd(L, _lib, z_in=-1) == -1
    assert _act_fwd(L, _lib, s_in=0.0) == -1 and b"scale" in err()
    assert _act_fwd(L, _lib, In=65794) == -2 and b"2^31" in err()          # the existing size limits
    assert _act_fwd(L, _lib, S=70000) == -2
    # the conv and the Flipout entries: the same checks under their own names
    g = _lib.bt_conv2d_geom(1, 4, 5, 5, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    pr = [_lib.bt_q8_pair(s, z, 0) for s, z in [(6 / 255, 0), (1e-4, 0), (1e-3, 0), (0.1, 128), (0.1, 128)]]
    P = _lib.bt_q8_params(*pr, 0.01, 0.01, 256, 512, None, None)
    R = _lib.bt_rng(1, None, 0, 1, 0, 0)
    assert L.bt_q8_conv2d_fwd_act(C.byref(g), 1, 1032, 1, 0, C.byref(P), None, None, C.byref(R), None, 4096, None) == -1 and b"bt_q8_conv2d_fwd_act" in err()
    assert L.bt_q8_conv2d_fwd_act(C.byref(g), 1, 1024, 1, 0, C.byref(P), None, None, C.byref(R), None, None, None) == -1 and b"neither" in err()
    assert L.bt_q8_conv2d_fwd_act(None, 1, 1024, 1, 0, C.byref(P), None, None, C.byref(R), None, 4096, None) == -1
    fp = [_lib.bt_q8_pair(6 / 255, 0, 0), _lib.bt_q8_pair(1e-4, 0, 0)] + [_lib.bt_q8_pair(0.1, 128, 0) for _ in range(8)]
    FP = _lib.bt_q8_flip_params(*fp, 0.01, 0.01, 256, 512, None, None)
    assert L.bt_q8_flip_conv2d_fwd_act(C.byref(g), 1, 1028, 1, 0, C.byref(FP), None, None, None, None, C.byref(R), None, 4096, None) == -1
    assert b"bt_q8_flip_conv2d_fwd_act" in err() and b"16-byte aligned" in err()
    assert L.bt_q8_flip_linear_fwd_act(2, 20, 4, 1, 1024, 1, 0, C.byref(FP), None, None, None, None, C.byref(R), None, None, None) == -1
    assert b"bt_q8_flip_linear_fwd_act" in err() and b"neither" in err()


def test_element_wise_entry_points_refuse_before_any_launch():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    err = lambda: L.bt_last_error_string()
    sh = (C.c_int64 * 4)(2, 20, 3, 3)
    other = (C.c_int64 * 4)(2, 20, 3, 2)
    assert L.bt_q8_act_quantize(None, 2, 3, 4, 4, 0.1, 0, 4096, None) == -1 and b"bt_q8_act_quantize" in err()
    assert L.bt_q8_act_quantize(1024, 2, 3, 4, 4, 0.1, 0, 4100, None) == -1 and b"16-byte aligned" in err()
    assert L.bt_q8_act_quantize(1024, 2, 3, 4, 4, 0.0, 0, 4096, None) == -1 and b"scale" in err()
    assert L.bt_q8_act_quantize(1024, 2, 3, 4, 4, 0.1, 256, 4096, None) == -1 and b"zero point" in err()
    assert L.bt_q8_act_quantize(1024, 0, 3, 4, 4, 0.1, 0, 4096, None) == -1
    assert L.bt_q8_act_dequantize(1028, 2, 3, 4, 4, 0.1, 0, 4096, None) == -1 and b"bt_q8_act_dequantize" in err()
    assert L.bt_q8_act_dequantize(1024, 2, 3, 4, 4, -0.1, 0, 4096, None) == -1
    assert L.bt_q8_act_relu(1024, 2, 3, 4, 4, -1, 4096, None) == -1 and b"bt_q8_act_relu" in err()
    assert L.bt_q8_act_relu(1024, 2, 3, 4, 4, 0, 4104, None) == -1
    assert L.bt_q8_act_add(1024, sh, 0.1, 0, 2048, other, 0.1, 0, 0.1, 0, 0, 4096, None) == -1 and b"differ in shape" in err() and b"bt_q8_act_add" in err()
    assert L.bt_q8_act_add(1024, sh, 0.1, 0, 2048, sh, 0.1, 0, 0.0, 0, 0, 4096, None) == -1 and b"scale" in err()
    assert L.bt_q8_act_add(1024, sh, 0.1, 0, 2048, sh, 0.1, 300, 0.1, 0, 0, 4096, None) == -1 and b"zero point" in err()
    assert L.bt_q8_act_add(1024, sh, 0.1, 0, 2056, sh, 0.1, 0, 0.1, 0, 1, 4096, None) == -1 and b"aligned" in err()
    assert L.bt_q8_act_add(1024, sh, 0.1, 0, None, sh, 0.1, 0, 0.1, 0, 1, 4096, None) == -1
    assert L.bt_q8_act_max_pool2d(1024, 2, 3, 4, 4, 3, 3, 0, 2, 1, 1, 4096, None) == -1 and b"bt_q8_act_max_pool2d" in err()
    assert L.bt_q8_act_max_pool2d(1024, 2, 3, 4, 4, 3, 3, 2, 2, 2, 1, 4096, None) == -1
    assert L.bt_q8_act_max_pool2d(1024, 2, 3, 2, 2, 5, 5, 1, 1, 0, 0, 4096, None) == -1 and b"empty" in err()
    assert L.bt_q8_act_avg_pool(1024, 2, 3, 4, 4, 256, 4096, None) == -1 and b"bt_q8_act_avg_pool" in err()
    assert L.bt_q8_act_avg_pool(1024, 2, 3, 4096, 4096, 0, 4096, None) == -2 and b"2^23" in err()
    assert L.bt_q8_act_unblock(1024, 2, 3, 4, 4, 0, 4097, None) == -1 and b"bt_q8_act_unblock" in err()
    assert L.bt_q8_act_unblock(1024, 1 << 30, 1 << 20, 4, 4, 0, 4096, None) == -2


def test_header_binding_and_library_agree():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), name
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(handle, name), name
    assert re.search(r"#define BT_Q8_X_F32 0\b", hdr) and re.search(r"#define BT_Q8_X_U8 1\b", hdr) and (_lib.Q8_X_F32, _lib.Q8_X_U8) == (0, 1)
    assert _lib.lib().bt_version() == 302                      # additions only
    mk = open(os.path.join(ROOT, "bayesian_torch_amd", "csrc", "Makefile")).read()
    assert "bt_q8_act.hip" in mk
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integ, name


def test_alias_imports():
    import bayesian_torch.quantization as RQ
    import bayesian_torch.quantization.qact as RA
    import bayesian_torch_amd.quantization as Q
    from bayesian_torch_amd.quantization import qact
    assert RA.QActivation is qact.QActivation is Q.QActivation is RQ.QActivation
    assert RA.add_relu is qact.add_relu and RA.quantize_per_tensor is qact.quantize_per_tensor and RQ.QuantStub is qact.QuantStub
    assert RQ.DeQuantStub is qact.DeQuantStub and RQ.QFunctional is qact.QFunctional
    for name in qact.__all__:
        assert getattr(RA, name) is getattr(qact, name), name
    from bayesian_torch_amd.harness import resnet as H
    assert callable(H.u8_inference)
