"""CPU: the INT8 quantised layers without a GPU -- the model (tests/_q8_model.py) against every byte the reference produced
(tests/golden/q8_*.npz, tools/make_q8_goldens.py), quantize() / bnn_to_qbnn on CPU tensors against the reference's int images, scales
and folded biases, the module walk, the signatures, the refusals (raised on the host, before any launch), the C ABI's surface and the
alias imports. No kernels are launched."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn

import _q8_cases as QC
import _q8_model as M
from conftest import ROOT


def test_fixture_list():
    assert QC.GOLDENS == QC.EXPECTED_GOLDENS


@pytest.mark.parametrize("tag", QC.EXPECTED_GOLDENS)
def test_model_reproduces_golden_bytes(tag):
    g = QC.load(tag)
    oq, out = M.forward(g["x"], g["q_mu"], g["q_sigma"], g["s_mu"], g["s_sigma"], QC.pairs_of(g), g["eps_w"], g.get("q_mu_b"), g.get("q_sigma_b"),
                        g.get("eps_b"), QC.conv_of(tag))
    assert torch.equal(oq, g["out_q"]), int((oq != g["out_q"]).sum())
    assert torch.equal(out, g["out"])


@pytest.mark.parametrize("tag", QC.EXPECTED_GOLDENS)
def test_conversion_reproduces_golden_images(tag):
    g = QC.load(tag)
    q = QC.converted(tag, g)
    assert q.quantized_mu_weight.dtype == torch.int8 and torch.equal(q.quantized_mu_weight, g["q_mu"])
    assert torch.equal(q.quantized_sigma_weight, g["q_sigma"])
    assert float(q.quantized_mu_scale.item()) == g["s_mu"] and float(q.quantized_sigma_scale.item()) == g["s_sigma"]
    for name, key in (("quantized_mu_bias", "q_mu_b"), ("quantized_sigma_bias", "q_sigma_b")):
        have = getattr(q, name)
        assert (have is None) == (key not in g), name
        if have is not None and key == "q_mu_b":          # arithmetic only (+, -, *, /, IEEE sqrt): the same bits on every host
            assert torch.equal(have, g[key]), name
        elif have is not None:
            # log1p(exp(rho_b)) goes through the host's fp32 exp / log1p, which are not the same function on every CPU (the reference run
            # on another machine missed its own recorded tensor by one ulp in one element of 12): exact against the reference's
            # operations evaluated here, and within that one ulp of the bytes recorded on the generating host
            want = torch.log1p(torch.exp(g["rho_b"]))
            if "bn_weight" in g:
                want = want * (g["bn_weight"] / torch.sqrt((g["bn_var"] + g["bn_eps"]).double()).float())
            assert torch.equal(have, want), name
            assert int((have.view(torch.int32) - g[key].view(torch.int32)).abs().max()) <= 1, name
    assert q.bias == ("q_mu_b" in g)
    if q.quant_dict is None:      # the default branch's five pairs, as the reference derives them
        ds = 0.2 if tag.startswith("linear") else 0.1
        assert q._pairs(g["s_mu"], g["s_sigma"], 6 / 255, ds, 128) == QC.pairs_of(g)
    sd = q.state_dict()
    assert list(sd)[:4] == ["quantized_mu_weight", "quantized_sigma_weight", "quantized_mu_scale", "quantized_sigma_scale"]
    q2 = type(q)(*((q.in_features, q.out_features) if tag.startswith("linear") else (q.in_channels, q.out_channels, q.kernel_size)))
    q2.load_state_dict(sd)                 # a fresh shell takes the checkpoint, bias tensors included
    assert torch.equal(q2.quantized_mu_weight, g["q_mu"]) and float(q2.quantized_sigma_scale.item()) == g["s_sigma"]
    assert all(torch.equal(a, b) for a, b in zip(q2.state_dict().values(), sd.values())) and list(q2.state_dict()) == list(sd) and q2.bias == q.bias


def test_get_quantized_tensor_and_zero_scale():
    import bayesian_torch_amd.layers as L
    q = L.QuantizedLinearReparameterization(3, 2)
    t = torch.tensor([[0.5, -1.0, 0.25]])
    img, s = q.get_quantized_tensor(t)
    ref = torch.quantize_per_tensor(t, float(s), 0, torch.qint8)
    assert torch.equal(img, ref.int_repr()) and float(s) == float(torch.tensor(1.0) * 2 / 255)
    img, s = q.get_quantized_tensor(torch.zeros(4))
    assert float(s) == float(torch.tensor(0.1)) and int(img.abs().max()) == 0
    img, s = q.get_quantized_tensor(torch.tensor([250.0, -3.0]))        # the upper bound of 100
    assert float(s) == float(torch.tensor(100.0) * 2 / 255) and img.tolist() == [127, -4]
    sc, zp = q.get_scale_and_zero_point(t)
    assert float(zp) == 0.0 and float(sc) == float(s) * 0 + float(torch.tensor(1.0) * 2 / 255)


class _Block(nn.Module):
    def __init__(self, L, cin, planes, stride):
        super().__init__()
        self.conv1 = L.Conv2dReparameterization(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = L.Conv2dReparameterization(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = nn.Sequential(L.Conv2dReparameterization(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        self.extra = L.Conv2dReparameterization(planes, planes, 1, bias=True)       # no rule of the folding walk names it


class _Net(nn.Module):
    def __init__(self, L):
        super().__init__()
        self.conv1 = L.Conv2dReparameterization(3, 4, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(4)
        self.layer1 = nn.Sequential(_Block(L, 4, 8, 2))
        self.fc = L.LinearReparameterization(8, 3)


def _kinds(net):
    return {n: type(m).__name__ for n, m in net.named_modules() if not m._modules and n}


def test_module_walk_matches_the_reference_walk():
    """What models/bnn_to_qbnn.py:198-237 replaces on a small ResNet-style block, with and without fuse_conv_bn."""
    import bayesian_torch.layers as L
    from bayesian_torch.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch.models.dnn_to_bnn import get_kl_loss
    QC_, QL = "QuantizedConv2dReparameterization", "QuantizedLinearReparameterization"
    net = _Net(L).eval()
    assert bnn_to_qbnn(net) is None
    assert _kinds(net) == {"conv1": QC_, "bn1": "BatchNorm2d", "layer1.0.conv1": QC_, "layer1.0.bn1": "BatchNorm2d", "layer1.0.conv2": QC_,
                           "layer1.0.bn2": "BatchNorm2d", "layer1.0.downsample.0": QC_, "layer1.0.downsample.1": "BatchNorm2d", "layer1.0.extra": QC_, "fc": QL}
    assert net.layer1[0].conv1.quantized_mu_bias is None and net.layer1[0].extra.quantized_sigma_bias is not None
    assert float(get_kl_loss(net)) == 0.0 and float(net.fc.kl_loss()) == 0.0
    net = _Net(L).eval()
    ids = {n: m._layer_id for n, m in net.named_modules() if hasattr(m, "_layer_id")}
    with pytest.warns(UserWarning, match="'extra' is named by no conv/bn folding rule and stays float"):
        bnn_to_qbnn(net, fuse_conv_bn=True)
    assert _kinds(net) == {"conv1": QC_, "bn1": "Identity", "layer1.0.conv1": QC_, "layer1.0.bn1": "Identity", "layer1.0.conv2": QC_,
                           "layer1.0.bn2": "Identity", "layer1.0.downsample.0": QC_, "layer1.0.downsample.1": "Identity",
                           "layer1.0.extra": "Conv2dReparameterization", "fc": QL}      # as in the reference: a conv no rule names stays
    c = net.layer1[0].conv1
    assert c.bias is True and c.quantized_mu_bias is not None and c.quantized_sigma_bias is None and c.bn_weight is None
    assert {n: m._layer_id for n, m in net.named_modules() if hasattr(m, "_layer_id")} == ids      # the draw streams stay where they were


class _Stem(nn.Module):
    def __init__(self, conv, bn):
        super().__init__()
        self.conv1, self.bn1 = conv, bn


@pytest.mark.parametrize("tag", ["conv_c8x12k3p1_bn", "conv_c8x12k3p1_bnb_z57", "conv_c5x7k3p1"])
def test_bnn_to_qbnn_itself_reproduces_golden_images(tag):
    """The goldens through the module walk: a module with conv1 / bn1 under fuse_conv_bn=True (the BatchNorm fixtures), and without it."""
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    g = QC.load(tag)
    d, bn = QC.float_layer(tag, g)
    fold = bn is not None
    m = _Stem(d, bn if fold else nn.BatchNorm2d(g["mu_w"].shape[0]).eval())
    bnn_to_qbnn(m, fuse_conv_bn=fold)
    q = m.conv1
    assert type(q).__name__ == "QuantizedConv2dReparameterization" and type(m.bn1).__name__ == ("Identity" if fold else "BatchNorm2d")
    assert torch.equal(q.quantized_mu_weight, g["q_mu"]) and torch.equal(q.quantized_sigma_weight, g["q_sigma"])
    assert float(q.quantized_mu_scale.item()) == g["s_mu"] and float(q.quantized_sigma_scale.item()) == g["s_sigma"]
    assert (q.quantized_mu_bias is None) == ("q_mu_b" not in g) and (q.quantized_sigma_bias is None) == ("q_sigma_b" not in g)
    if "q_mu_b" in g:
        assert torch.equal(q.quantized_mu_bias, g["q_mu_b"])
    direct = QC.converted(tag, g)
    assert all(torch.equal(a, b) for a, b in zip(q.state_dict().values(), direct.state_dict().values())) and list(q.state_dict()) == list(direct.state_dict())


def test_flags_follow_the_float_layer():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    net = nn.Sequential(nn.Conv2d(3, 4, 3), nn.Flatten(), nn.Linear(4, 2))
    dnn_to_bnn(net, {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization",
                     "moped_enable": False, "moped_delta": 0.5})
    bnn_to_qbnn(net)
    assert isinstance(net[0], L.QuantizedConv2dReparameterization) and net[0].dnn_to_bnn_flag and net[2].dnn_to_bnn_flag
    assert net[0].stride == (1, 1) and net[0]._conv()["padding"] == (0, 0)


def test_signatures():
    import bayesian_torch_amd.layers as L
    sig = lambda f: list(inspect.signature(f).parameters)[1:]
    assert sig(L.QuantizedLinearReparameterization.__init__) == ["in_features", "out_features"]
    assert sig(L.QuantizedConv2dReparameterization.__init__) == ["in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "bias"]
    fwd = ["input", "enable_int8_compute", "normal_scale", "default_scale", "default_zero_point", "return_kl"]
    for cls, ds in ((L.QuantizedLinearReparameterization, 0.2), (L.QuantizedConv2dReparameterization, 0.1)):
        assert sig(cls.forward) == fwd
        p = inspect.signature(cls.forward).parameters
        assert (p["enable_int8_compute"].default, p["normal_scale"].default, p["default_scale"].default, p["default_zero_point"].default,
                p["return_kl"].default) == (True, 6 / 255, ds, 128, True)


def test_refusals():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    for mod, name in ((L.LinearFlipout(3, 2), "LinearFlipout"), (L.Conv2dFlipout(2, 2, 3), "Conv2dFlipout"), (L.Conv1dReparameterization(2, 2, 3), "Conv1dReparameterization"),
                      (L.Conv3dReparameterization(2, 2, 3, 0, 1, 0, -3.0), "Conv3dReparameterization"),
                      (L.ConvTranspose2dReparameterization(2, 2, 3), "ConvTranspose2dReparameterization"),
                      (L.LSTMReparameterization(3, 2), "LSTMReparameterization")):
        with pytest.raises(NotImplementedError, match=name):
            bnn_to_qbnn(nn.Sequential(mod))
    with pytest.raises(NotImplementedError, match="groups"):
        bnn_to_qbnn(nn.Sequential(L.Conv2dReparameterization(4, 4, 3, groups=2)))
    for fuse_named in (True, False):      # fuse_conv_bn=True: a Flipout conv refuses whether a folding rule names it or not
        m = nn.Module()
        setattr(m, "conv1" if fuse_named else "other", L.Conv2dFlipout(2, 2, 3))
        m.bn1 = nn.BatchNorm2d(2)
        with pytest.raises(NotImplementedError, match="Conv2dFlipout"):
            bnn_to_qbnn(m, fuse_conv_bn=True)
    with pytest.raises(NotImplementedError, match="groups"):
        L.QuantizedConv2dReparameterization(4, 4, 3, groups=2)
    q = L.QuantizedLinearReparameterization(3, 2)
    with pytest.raises(NotImplementedError):
        q.prepare()
    with pytest.raises(NotImplementedError, match="enable_int8_compute"):
        q(torch.zeros(1, 3), enable_int8_compute=False)
    with pytest.raises(RuntimeError, match="HIP"):      # no CPU forward
        q(torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match="no float layer"):
        q.quantize()


def _params(lib, pairs, s_mu=0.01, s_sigma=0.01):
    pr = [lib.bt_q8_pair(s, z, 0) for s, z in pairs]
    return lib.bt_q8_params(*pr, s_mu, s_sigma, 256, 512, None, None)     # (aligned non-null pack addresses: nothing is launched)


def test_c_abi_refuses_before_any_launch():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    ok = [(6 / 255, 0), (1e-4, 0), (1e-3, 0), (0.1, 128), (0.1, 128)]

    def lin(pairs, In=8, S=1, rng=True, **kw):
        P = _params(_lib, pairs, **kw)
        R = _lib.bt_rng(1, None, 0, 1, 0, 0)
        return L.bt_q8_linear_fwd(2, In, 4, S, 1024, 0, C.byref(P), None, None, C.byref(R) if rng else None, 2048, None, None)

    def conv(pairs, groups):
        P = _params(_lib, pairs)
        g = _lib.bt_conv2d_geom(1, 4, 5, 5, 4, 3, 3, 1, 1, 1, 1, 1, 1, groups)
        R = _lib.bt_rng(1, None, 0, 1, 0, 0)
        return L.bt_q8_conv2d_fwd(C.byref(g), 1, 1024, 0, C.byref(P), None, None, C.byref(R), 2048, None, None)

    edit = lambda i, s=None, z=None: [(s if (j == i and s is not None) else p[0], z if (j == i and z is not None) else p[1]) for j, p in enumerate(ok)]
    assert conv(ok, 2) == -2 and b"groups" in L.bt_last_error_string()
    for i in range(3):
        assert lin(edit(i, z=1)) == -2 and b"zero point" in L.bt_last_error_string()
    assert lin(ok, In=65794) == -2 and b"2^31" in L.bt_last_error_string()        # 65794 * 32640 >= 2^31
    for i in range(5):
        assert lin(edit(i, s=0.0)) == -1 and b"scale" in L.bt_last_error_string()
        assert lin(edit(i, s=-0.1)) == -1
    assert lin(ok, s_mu=0.0) == -1 and lin(ok, s_sigma=-1.0) == -1
    for i in (3, 4):
        assert lin(edit(i, z=-1)) == -1 and b"zero point" in L.bt_last_error_string()
        assert lin(edit(i, z=256)) == -1
    assert lin(ok, rng=False) == -1 and lin(ok, S=0) == -1
    assert L.bt_q8_pack(None, None, 1, 1, 1, None, None, None) == -1


def test_header_binding_and_library_agree():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in ("bt_q8_pack", "bt_q8_linear_fwd", "bt_q8_conv2d_fwd"):
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), name
        assert name in _lib.EXPORTS and hasattr(handle, name), name
    assert C.sizeof(_lib.bt_q8_pair) == 16 and C.sizeof(_lib.bt_q8_params) == 5 * 16 + 2 * 8 + 4 * 8
    assert _lib.lib().bt_version() == 302
    mk = open(os.path.join(ROOT, "bayesian_torch_amd", "csrc", "Makefile")).read()
    assert "bt_q8.hip" in mk


def test_alias_imports():
    import bayesian_torch.layers as RL
    import bayesian_torch.layers.variational_layers as RV
    import bayesian_torch.models.bnn_to_qbnn as RQ
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.layers.variational_layers import QuantizedConv2dReparameterization, QuantizedLinearReparameterization
    assert RL.QuantizedConv2dReparameterization is L.QuantizedConv2dReparameterization is QuantizedConv2dReparameterization is RV.QuantizedConv2dReparameterization
    assert RL.QuantizedLinearReparameterization is QuantizedLinearReparameterization
    assert callable(RQ.bnn_to_qbnn) and callable(RQ.batch_norm_folding) and callable(RQ.qbnn_conv_layer) and callable(RQ.qbnn_linear_layer)
